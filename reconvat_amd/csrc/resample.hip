// Rational-ratio polyphase FIR resampler with the channel downmix fused in: what turns a 44.1 / 48 kHz stereo
// recording into the 16 kHz mono stream every model here consumes.
//
//   y[m] = sum_n x[n] h[m M - n L],   x[n] = mean over channels of input frame n (0 outside the signal),   L/M = sr_out/sr_in
//
// The host (reconvat_amd/resample.py::design_filter) lays the Kaiser-windowed sinc h out as a polyphase bank
//   bank[p][u] = h[p + (F - u) L]   (0 where |.| > half),  p < L, u < Kp, F = half / L, Kp = taps per phase rounded up to 4
// so that with q = m M, n0 = q / L, p = q % L:   y[m] = sum_u bank[p][u] x[n0 - F + u]   -- both operands ascending in u.
//
// One workgroup owns TILE = Lr * R consecutive outputs, Lr = the multiple of L next to 256 (so outputs Lr apart share their phase):
//   1. the input span of the tile is staged ONCE in LDS as float: int -> float conversion, downmix and the zero extension at
//      both signal ends happen on that load (every global read is predicated on 0 <= n < T_in);
//   2. work item w < Lr computes the R outputs w, w + Lr, .. of the tile: one 16-byte load of four coefficients of ITS bank row
//      feeds 4 R FMAs against LDS reads.  The bank is not assumed to fit in LDS (226 KB at 44.1 -> 16 kHz, 2.8 MB at
//      44056 -> 16 kHz): rows are streamed from L2 / L1, R outputs per coefficient load cut that traffic by R.
// Every output is ONE accumulator summed u = 0 .. Kp-1 in ascending order with fmaf: the bits do not depend on R, on the tile or
// on how the caller cut the signal into chunks (a chunk passes its slice and `in_offset`; out-of-slice reads only ever fall
// outside the signal).  No atomics, no allocation, no synchronisation.
#include "common.h"

#define RV_RESAMPLE_MAX_COEFFS (1L << 22)      // bank cap: L * Kp floats (16 MiB); 44056 -> 16000 needs 0.71 M
#define RV_RESAMPLE_MAX_SPAN 12288             // floats of LDS per tile (48 KiB)
#define RV_RESAMPLE_MAX_RATIO 65536            // L, M
#define RV_RESAMPLE_MAX_CHANNELS 64

struct ResampleArgs {
    const void* x; const float* bank; void* y;
    long T_in, in_offset, m_start, n_out;
    int C, L, M, F, Kp, Lr, tile, span, stepx;
    float scale;                               // sample scale / C
};

template <typename Tin> __device__ __forceinline__ float load_frame(const Tin* x, long n, int C, float scale);
template <> __device__ __forceinline__ float load_frame<short>(const short* x, long n, int C, float scale) {
    const short* f = x + n * C;
    int s = 0;                                 // |s| <= 64 * 2^15: exact
    for (int c = 0; c < C; ++c) s += f[c];
    return (float)s * scale;
}
template <> __device__ __forceinline__ float load_frame<int>(const int* x, long n, int C, float scale) {
    const int* f = x + n * C;
    long s = 0;
    for (int c = 0; c < C; ++c) s += f[c];
    return (float)s * scale;
}
template <> __device__ __forceinline__ float load_frame<float>(const float* x, long n, int C, float scale) {
    const float* f = x + n * C;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += f[c];
    return s * scale;
}

template <int R, typename Tin, bool OUT_I16> __global__ __launch_bounds__(256) void resample_k(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const long t0 = (long)blockIdx.x * a.tile;                 // first output of the tile, relative to m_start
    const long q0 = (a.m_start + t0) * a.M;
    const long n_base = q0 / a.L - a.F;                        // signal index of xs[0]
    const int p0 = (int)(q0 % a.L);
    const Tin* x = reinterpret_cast<const Tin*>(a.x);
    for (int s = threadIdx.x; s < a.span; s += 256) {
        const long n = n_base + s - a.in_offset;
        xs[s] = (n >= 0 && n < a.T_in) ? load_frame<Tin>(x, n, a.C, a.scale) : 0.f;
    }
    __syncthreads();
    const long left = a.n_out - t0;                            // outputs of this tile that exist
    for (int w = threadIdx.x; w < a.Lr && w < left; w += 256) {
        const long t = (long)p0 + (long)w * a.M;
        const int off = (int)(t / a.L), p = (int)(t % a.L);
        const f32x4* row = reinterpret_cast<const f32x4*>(a.bank + (long)p * a.Kp);
        const float* xr = xs + off;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        for (int u = 0; u < a.Kp; u += 4) {
            const f32x4 c = row[u >> 2];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* xv = xr + r * a.stepx + u;
                acc[r] = fmaf(c[0], xv[0], acc[r]);
                acc[r] = fmaf(c[1], xv[1], acc[r]);
                acc[r] = fmaf(c[2], xv[2], acc[r]);
                acc[r] = fmaf(c[3], xv[3], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long i = t0 + w + (long)r * a.Lr;
            if (i < a.n_out) {
                if (OUT_I16) {
                    const float v = fminf(fmaxf(rintf(acc[r] * 32768.0f), -32768.0f), 32767.0f);     // round half to even, saturate
                    reinterpret_cast<short*>(a.y)[i] = (short)(int)v;
                } else {
                    reinterpret_cast<float*>(a.y)[i] = acc[r];
                }
            }
        }
    }
}

template <int R, typename Tin> static void launch_r(const ResampleArgs& a, int out_dtype, unsigned grid, hipStream_t st) {
    const size_t lds = (size_t)a.span * sizeof(float);
    if (out_dtype == 1) hipLaunchKernelGGL((resample_k<R, Tin, true>), dim3(grid), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((resample_k<R, Tin, false>), dim3(grid), dim3(256), lds, st, a);
}

template <typename Tin> static void launch_t(const ResampleArgs& a, int R, int out_dtype, unsigned grid, hipStream_t st) {
    if (R == 4) launch_r<4, Tin>(a, out_dtype, grid, st);
    else if (R == 2) launch_r<2, Tin>(a, out_dtype, grid, st);
    else launch_r<1, Tin>(a, out_dtype, grid, st);
}

// LDS floats of a tile of Lr * R outputs: the furthest first-row offset, the R - 1 row steps and one row of taps.
static long tile_span(int L, int M, int Kp, int Lr, int R) {
    return ((long)(L - 1) + (long)(Lr - 1) * M) / L + (long)(R - 1) * ((long)Lr / L * M) + Kp;
}

extern "C" {

long rv_resample_max_coeffs(void) { return RV_RESAMPLE_MAX_COEFFS; }

// x: [T_in, C] interleaved frames of in_dtype (0 int16, 1 int32, 2 float32), the slice [in_offset, in_offset + T_in) of the signal;
// the caller guarantees that every sample of the SIGNAL that outputs [m_start, m_start + n_out) touch lies in that slice (frames
// outside it are read as zero, which is right only beyond the signal's ends).  bank: [L, Kp] float32 as laid out above, 16-byte
// aligned.  y: n_out samples of out_dtype (0 float32, 1 int16 = saturated round-half-even of 32768 y); y[0] is output m_start.
int rv_resample(const void* x, int in_dtype, long T_in, int C, long in_offset, const float* bank, int L, int M, int F, int Kp, void* y,
                int out_dtype, long m_start, long n_out, void* stream) {
    RV_CHECK_ARG(x && bank && y, "rv_resample: null pointer");
    RV_CHECK_ARG(T_in >= 1 && n_out >= 1 && in_offset >= 0 && m_start >= 0, "rv_resample: empty signal or negative offset");
    RV_CHECK_ARG(C >= 1 && C <= RV_RESAMPLE_MAX_CHANNELS, "rv_resample: channels %d not in 1..%d", C, RV_RESAMPLE_MAX_CHANNELS);
    RV_CHECK_ARG(in_dtype >= 0 && in_dtype <= 2 && out_dtype >= 0 && out_dtype <= 1, "rv_resample: unknown sample type");
    RV_CHECK_ARG(L >= 1 && M >= 1 && L <= RV_RESAMPLE_MAX_RATIO && M <= RV_RESAMPLE_MAX_RATIO, "rv_resample: ratio %d/%d out of range", L, M);
    RV_CHECK_ARG(Kp >= 4 && (Kp & 3) == 0 && F >= 0 && F < Kp, "rv_resample: bad bank shape (F %d, Kp %d)", F, Kp);
    RV_CHECK_ARG((long)L * Kp <= RV_RESAMPLE_MAX_COEFFS, "rv_resample: bank of %ld coefficients over the cap of %ld", (long)L * Kp,
                 RV_RESAMPLE_MAX_COEFFS);
    RV_CHECK_ARG((((uintptr_t)bank) & 15) == 0, "rv_resample: bank must be 16-byte aligned");
    RV_CHECK_ARG(m_start + n_out <= (1L << 40) && in_offset + T_in <= (1L << 40), "rv_resample: signal too long");
    ResampleArgs a;
    a.x = x; a.bank = bank; a.y = y;
    a.T_in = T_in; a.in_offset = in_offset; a.m_start = m_start; a.n_out = n_out;
    a.C = C; a.L = L; a.M = M; a.F = F; a.Kp = Kp;
    a.Lr = cdiv(256, L) * L;
    int R = 4;
    while (R > 1 && tile_span(L, M, Kp, a.Lr, R) > RV_RESAMPLE_MAX_SPAN) R >>= 1;
    const long span = tile_span(L, M, Kp, a.Lr, R);
    RV_CHECK_ARG(span <= RV_RESAMPLE_MAX_SPAN, "rv_resample: input tile of %ld floats over the LDS budget of %d", span, RV_RESAMPLE_MAX_SPAN);
    a.span = (int)span; a.tile = a.Lr * R; a.stepx = a.Lr / L * M;
    a.scale = (in_dtype == 0 ? 1.0f / 32768.0f : in_dtype == 1 ? 1.0f / 2147483648.0f : 1.0f) / (float)C;
    const long grid = (n_out + a.tile - 1) / a.tile;
    RV_CHECK_ARG(grid <= 0x7fffffffL, "rv_resample: too many tiles in one call");
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == 0) launch_t<short>(a, R, out_dtype, (unsigned)grid, st);
    else if (in_dtype == 1) launch_t<int>(a, R, out_dtype, (unsigned)grid, st);
    else launch_t<float>(a, R, out_dtype, (unsigned)grid, st);
    RV_LAUNCH_CHECK("rv_resample");
    return RV_OK;
}

}  // extern "C"
