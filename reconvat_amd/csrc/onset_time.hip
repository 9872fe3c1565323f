// Sub-frame note onsets: per note, the amplitude of the key's first eight harmonics at 49 window positions 32 samples
// apart around the decoded frame, and the position at which most harmonics rise most steeply.  reconvat_amd/onset_time.py has the
// definition; in short, for a note (key p, frame t), c = 512 t:
//     A[m][q]  = | sum_n tab[p][q][.][n] x[c - 1024 + 32 m + n] |,  m = 0..48, n = 0..511, tab = Hann window x (cos, -sin) of q f0(p)
//     d[m][q]  = A[m + 1][q] - A[m - 1][q],  m = 1..47;    k_q = the first m with the largest d[.][q]
//     k        = the lower median of k_q over the valid harmonics (q f0 <= 7200 Hz; V(p) of them, a prefix)
//     sample   = clamp(c - 768 + 32 k - lead, 0, T - 1)
//
// Per note that is the GEMM D[m][j] = sum_n X[m][n] B[n][j] on v_mfma_f32_16x16x4_f32 with X[m][n] = x[c - 1024 + 32 m + n] a Hankel
// matrix over ONE 2048-sample window (never formed), B[n][j] = tab[p][j][n] the key's 512 x 16 slice of the table (j = 2 (q - 1) + re/im),
// M = 49 padded to 64, N = 16, K = 512: 512 MFMAs.
//
// onset_refine_k   one workgroup = one note, 4 waves, wave w = the row tile m = 16 w .. 16 w + 15.  The window is staged in LDS once,
//                  every read outside [0, T) replaced by 0 with a select (whatever memory holds there), and 512 zeros behind it for
//                  the padded rows 49..63.  Rows of 16 samples are ONS_ROW = 20 floats apart (as FIR_ROW in acoustics.hip): the 16
//                  rows of a tile start 32 samples = 40 floats apart, so the 16-byte operand reads of a lane group fall on 16
//                  different 4-bank slots.  K is permuted inside a 16-sample block (MFMA j of block b takes n = 16 b + 4 (lane >> 4)
//                  + j): a lane's four samples, and its four table values, are one 16-byte read each; the table comes straight from
//                  global memory (32 KB per key, shared by the four waves through L1 / L2).  Every MFMA starts from a ZERO
//                  accumulator -- four products of a component added in float32 -- and its four results are added to float64 sums on
//                  the vector unit, blocks and MFMAs in ascending order (as synth.hip evaluates terms in float32 and sums them in
//                  float64): the error of a component is 4 u sum |tab| |x|, not 512 u, which is what lets the float64 definition's
//                  argmax be reproduced (tests/onset_time_cases.py); the MFMAs are independent, so their latency is hidden as well.
//                  The epilogue runs in the same launch through LDS: D (float64) -> A = (float)sqrt(re^2 + im^2), rounded once;
//                  then one work item per harmonic walks m = 1..47 for the first maximum of the float32 difference d, then one work
//                  item sorts the V values and writes the sample.
// The order of every sum depends on nothing but the note: the same bits for any n and any place of the note in the list.  Plain vector
// stores only, no atomics.  The entry point never allocates and never synchronises.
#include <math.h>

#include "common.h"

#define ONS_KEYS 88
#define ONS_HARM 8
#define ONS_WIN 512
#define ONS_POS 49
#define ONS_SPAN 2048                          // samples c - 1024 .. c + 1023: what the 49 windows cover
#define ONS_STAGE 2560                         // + 512 zeros: the padded rows m = 49..63 read up to 32 * 63 + 511
#define ONS_ROW 20                             // LDS floats per 16 samples
#define ONS_XS (ONS_STAGE / 16 * ONS_ROW)      // 3200
#define ONS_DLD 17
#define ONS_ALD 9
#define ONS_D (2 * 64 * ONS_DLD)               // 1088 doubles
#define ONS_A 444                              // 49 * 9 = 441, rounded up
#define ONS_MAX_FRAME ((1 << 22) - 1)
#define ONS_CHUNK (1L << 20)                   // notes per launch

struct OnsArgs {
    const float* audio;
    long T;
    const float* table;
    const int* notes;
    int* out_sample;
    float* out_amp;
    int lead;
    unsigned char n_valid[ONS_KEYS];
};

__global__ __launch_bounds__(256) void onset_refine_k(OnsArgs a) {
    __shared__ __attribute__((aligned(16))) float ons_lds[ONS_XS + ONS_D + ONS_A + ONS_HARM];
    float* xs = ons_lds;
    double* ds = (double*)(ons_lds + ONS_XS);                              // (ONS_XS floats = 12800 bytes: 8-byte aligned)
    float* as = ons_lds + ONS_XS + ONS_D;
    int* ks = (int*)(as + ONS_A);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const long note = blockIdx.x;
    const int p = a.notes[2 * note], t = a.notes[2 * note + 1];
    if (p < 0 || p >= ONS_KEYS || t < 0 || t > ONS_MAX_FRAME) {        // (the same for the whole workgroup) not a note: no table access
        if (tid == 0) a.out_sample[note] = -1;
        if (a.out_amp)
            for (int i = tid; i < ONS_POS * ONS_HARM; i += 256) a.out_amp[note * (ONS_POS * ONS_HARM) + i] = 0.f;
        return;
    }
    const long c = 512L * t, g0 = c - ONS_SPAN / 2;
    for (int i = tid; i < ONS_STAGE; i += 256) {
        const long g = g0 + i;
        const bool in = i < ONS_SPAN && g >= 0 && g < a.T;
        const float v = a.audio[in ? g : 0];
        xs[(i >> 4) * ONS_ROW + (i & 15)] = in ? v : 0.f;
    }
    __syncthreads();

    const float* xa = xs + 2 * (16 * wave + li) * ONS_ROW + 4 * kq;                   // + blk * ONS_ROW
    const float* ba = a.table + ((long)p * 16 + li) * ONS_WIN + 4 * kq;               // + 16 blk
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int blk = 0; blk < ONS_WIN / 16; ++blk) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xa + blk * ONS_ROW);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(ba + 16 * blk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 part = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[j], bv[j], zero, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] += (double)part[i];
        }
    }
    // lane (column li, row group kq) holds D[16 wave + 4 kq + i][li] as element i
#pragma unroll
    for (int i = 0; i < 4; ++i) ds[(16 * wave + 4 * kq + i) * ONS_DLD + li] = sum[i];
    __syncthreads();

    const int V = a.n_valid[p];
    for (int i = tid; i < ONS_POS * ONS_HARM; i += 256) {
        const int m = i >> 3, q = i & 7;
        const double re = ds[m * ONS_DLD + 2 * q], im = ds[m * ONS_DLD + 2 * q + 1];
        const float amp = q < V ? (float)sqrt(re * re + im * im) : 0.f;
        as[m * ONS_ALD + q] = amp;
        if (a.out_amp) a.out_amp[note * (ONS_POS * ONS_HARM) + i] = amp;
    }
    __syncthreads();
    if (tid < ONS_HARM) {
        float best = as[2 * ONS_ALD + tid] - as[tid];
        int k = 1;
        for (int m = 2; m < ONS_POS - 1; ++m) {
            const float d = as[(m + 1) * ONS_ALD + tid] - as[(m - 1) * ONS_ALD + tid];
            if (d > best) { best = d; k = m; }
        }
        ks[tid] = k;
    }
    __syncthreads();
    if (tid == 0) {
        int s[ONS_HARM];
#pragma unroll
        for (int q = 0; q < ONS_HARM; ++q) s[q] = q < V ? ks[q] : ONS_POS;            // the invalid ones sort to the end
#pragma unroll
        for (int i = 1; i < ONS_HARM; ++i)
#pragma unroll
            for (int j = ONS_HARM - 1; j >= i; --j) {
                const int lo = min(s[j - 1], s[j]), hi = max(s[j - 1], s[j]);
                s[j - 1] = lo; s[j] = hi;
            }
        int k = s[0];
#pragma unroll
        for (int q = 1; q < ONS_HARM; ++q) k = q == (V - 1) / 2 ? s[q] : k;
        const long u = c - (ONS_WIN + ONS_WIN / 2) + 32L * k - a.lead;
        a.out_sample[note] = (int)(u < 0 ? 0 : (u > a.T - 1 ? a.T - 1 : u));
    }
}

static inline bool ons_aligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) == 0; }

extern "C" {

int rv_onset_refine(const float* audio, long T, const float* table, const int* notes, long n, int lead, int* out_sample, float* out_amp,
                    void* stream) {
    RV_CHECK_ARG(n >= 0 && n < (1L << 31), "rv_onset_refine: %ld notes outside [0, 2^31)", n);
    RV_CHECK_ARG(T >= 1 && T < (1L << 31), "rv_onset_refine: %ld samples outside [1, 2^31)", T);
    RV_CHECK_ARG(lead >= 0 && lead < (1 << 30), "rv_onset_refine: lead %d outside [0, 2^30)", lead);
    if (n == 0) return RV_OK;
    RV_CHECK_ARG(audio && table && notes && out_sample, "rv_onset_refine: null pointer");
    RV_CHECK_ARG(ons_aligned(table, 15), "rv_onset_refine: table must be 16-byte aligned");
    RV_CHECK_ARG(ons_aligned(audio, 3) && ons_aligned(notes, 3) && ons_aligned(out_sample, 3) && ons_aligned(out_amp, 3),
                 "rv_onset_refine: every buffer must be 4-byte aligned");
    OnsArgs a;
    a.audio = audio; a.T = T; a.table = table; a.lead = lead;
    for (int p = 0; p < ONS_KEYS; ++p) {
        const double f0 = 440.0 * exp2((double)(p + 21 - 69) / 12.0);
        int v = 0;
        for (int q = 1; q <= ONS_HARM; ++q) v += (double)q * f0 <= 7200.0;
        a.n_valid[p] = (unsigned char)v;
    }
    for (long i0 = 0; i0 < n; i0 += ONS_CHUNK) {                                      // the grid's x limit: one launch per 2^20 notes
        const long m = n - i0 < ONS_CHUNK ? n - i0 : ONS_CHUNK;
        a.notes = notes + 2 * i0;
        a.out_sample = out_sample + i0;
        a.out_amp = out_amp ? out_amp + i0 * (ONS_POS * ONS_HARM) : nullptr;
        hipLaunchKernelGGL(onset_refine_k, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream, a);
        RV_LAUNCH_CHECK("rv_onset_refine");
    }
    return RV_OK;
}

}  // extern "C"
