// Constant-Q front end for gfx950: reflect pad + banded complex "conv1d" (stride hop) + |.| + log(. + 1e-5), written
// time-major [B, T, n_bins], then a per-clip min-max normalisation pass.
//
// Reference: nnAudio CQT1992v2 (model/Spectrogram.py:1293-1326): two dense conv1d against [176, 1, 32768] kernels
// (236 GFLOP for 16 clips of 640 frames), 88 % of whose taps are zeros.  Here the bank is a banded GEMM per 16-bin group:
//     P[f][c] = sum_{t in window_g} x_pad[f * hop + t] * W_g[c][t - tw_g],   c = 0..15 real, 16..31 imaginary
// over the group's tap window only (the union of its rows' supports: 35 GFLOP for the same 16 clips), on
// v_mfma_f32_16x16x4_f32.  The A operand is Hankel: frame f, tap t reads x_pad[f * hop + t], so no im2col is formed --
// every lane fetches four consecutive taps of one frame with ONE 16-byte load straight from the padded audio (L1 / L2
// resident: a 64-frame tile of one slice reads 63 * 512 + 2048 floats that every wave of the tile shares).
//
// Balance: the groups' windows are 19 856 .. 196 taps wide, so the work is split along K into slices of at most 2048 taps
// (host tables: one work item per (group, slice)).  A workgroup = one clip x 64 frames x one item; its four waves take the
// 16-tap blocks of the slice round-robin and are summed in LDS in wave order; the items of a group are summed in item
// order by the epilogue kernel.  No float atomics: two calls are bit-identical.
#include "common.h"

#define CQT_FT 64        // frames per workgroup (four 16-frame MFMA tiles per wave)

struct CqtArgs {
    const float* xpad; long lp;   // [B][lp] reflect-padded audio
    const float* w; long w_floats;  // packed taps, per group [32][K_g]
    const int* items;             // [n_items][8]: group, first tap, taps, weight offset, K_g
    float* part;                  // [B][n_items][T][32] per-item partial sums
    int n_items, T, hop, kernel_width;
};

__device__ __forceinline__ unsigned cqt_f2ord(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cqt_ord2f(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ void cqt_pad_k(const float* x, long stride, int nsamp, int half, long valid, float* xpad, long lp) {
    const int b = blockIdx.y;
    const float* src = x + (long)b * stride;
    float* dst = xpad + (long)b * lp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < lp; i += (long)gridDim.x * blockDim.x) {
        long j = i - half;
        if (j < 0) j = -j;
        if (j >= nsamp) j = 2L * (nsamp - 1) - j;
        dst[i] = i < valid ? src[j] : 0.f;     // (the tail that rounds lp up to a multiple of 4 is never multiplied)
    }
}

// Operand layout of one v_mfma_f32_16x16x4_f32 (lane l: li = l & 15, kq = l >> 4): the A operand is the weight tile
// (row = column c of the group, k), the B operand the audio tile (k, column = frame); D[c][frame] lands as four
// consecutive c of one frame per lane.  K is permuted inside a 16-tap block -- MFMA j of the block takes tap 4 kq + j --
// so that a lane's four taps of the block are one 16-byte load for each operand.
__global__ __launch_bounds__(256) void cqt_band_k(CqtArgs a) {
    __shared__ f32x4 red[4][8][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int f0 = blockIdx.x * CQT_FT, item = blockIdx.y, b = blockIdx.z;
    const int* it = a.items + item * 8;
    const int tap0 = it[1], woff = it[3], kg = it[4];
    int ntap = it[2];
    // a table entry outside the bank multiplies nothing (zero partials) instead of reading past the audio or the taps
    if (tap0 < 0 || ntap < 0 || ((tap0 | ntap | woff | kg) & 15) != 0 || (long)tap0 + ntap > a.kernel_width || ntap > kg || woff < 0 ||
        (long)woff + 31L * kg + ntap > a.w_floats)
        ntap = 0;
    const float* xb = a.xpad + (long)b * a.lp + tap0 + 4 * kq;
    const float* xr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) xr[s] = xb + (long)min(f0 + 16 * s + li, a.T - 1) * a.hop;   // frames past T: re-read T-1
    const float* wr0 = a.w + woff + (long)li * kg + 4 * kq;                                  // real rows
    const float* wr1 = wr0 + 16L * kg;                                                       // imaginary rows
    f32x4 acc[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s][0] = acc[s][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nblk = ntap >> 4;
    int blk = wave;
    f32x4 xa[4], wa[2];
    if (blk < nblk) {
#pragma unroll
        for (int s = 0; s < 4; ++s) xa[s] = *reinterpret_cast<const f32x4*>(xr[s] + 16 * blk);
        wa[0] = *reinterpret_cast<const f32x4*>(wr0 + 16 * blk);
        wa[1] = *reinterpret_cast<const f32x4*>(wr1 + 16 * blk);
    }
    for (; blk < nblk; blk += 4) {
        f32x4 xn[4], wn[2];
        const int nx = blk + 4 < nblk ? blk + 4 : blk;                   // prefetch the wave's next block (last: reload)
#pragma unroll
        for (int s = 0; s < 4; ++s) xn[s] = *reinterpret_cast<const f32x4*>(xr[s] + 16 * nx);
        wn[0] = *reinterpret_cast<const f32x4*>(wr0 + 16 * nx);
        wn[1] = *reinterpret_cast<const f32x4*>(wr1 + 16 * nx);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    acc[s][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[h][j], xa[s][j], acc[s][h], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) xa[s] = xn[s];
        wa[0] = wn[0]; wa[1] = wn[1];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) red[wave][s * 2 + h][lane] = acc[s][h];
    __syncthreads();
    f32x4* part = reinterpret_cast<f32x4*>(a.part + (((long)b * a.n_items + item) * a.T) * 32);
#pragma unroll
    for (int e = tid; e < 512; e += 256) {
        const int sh = e >> 6, l = e & 63, s = sh >> 1, h = sh & 1;
        f32x4 v = red[0][sh][l];
        v += red[1][sh][l];
        v += red[2][sh][l];
        v += red[3][sh][l];
        const int f = f0 + 16 * s + (l & 15);
        if (f < a.T) part[(long)f * 8 + h * 4 + (l >> 4)] = v;     // columns 16 h + 4 (l >> 4) .. + 3 of frame f
    }
}

// per (clip, frame, bin): sum the group's items in order (group g = bin / 16), scale by sqrt(l_k), magnitude, log; per-clip min / max
__global__ __launch_bounds__(256) void cqt_finish_k(const float* part, const int* groups, const float* scale, int n_items, int T,
                                                    int n_bins, int do_log, float* out, unsigned* minmax) {
    __shared__ float red[2][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long per = (long)T * n_bins;
    const long i = (long)blockIdx.x * 256 + tid;
    float mn = INFINITY, mx = -INFINITY;
    if (i < per) {
        const int f = (int)(i / n_bins), k = (int)(i - (long)f * n_bins);
        const int g = k >> 4, c = k & 15;
        const int i0 = groups[2 * g];
        int ni = groups[2 * g + 1];
        if (i0 < 0 || ni < 0 || i0 + ni > n_items) ni = 0;
        const float* p = part + (((long)b * n_items + i0) * T + f) * 32 + c;
        float re = 0.f, im = 0.f;
        for (int q = 0; q < ni; ++q) {
            re += p[(long)q * T * 32];
            im += p[(long)q * T * 32 + 16];
        }
        const float sc = scale[k];
        re *= sc; im *= sc;
        const float m = sqrtf(re * re + im * im);
        const float v = do_log ? logf(m + 1e-5f) : m;
        out[(long)b * per + i] = v;
        mn = v; mx = v;
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        atomicMin(&minmax[2 * b], cqt_f2ord(mn));
        atomicMax(&minmax[2 * b + 1], cqt_f2ord(mx));
    }
}

__global__ void cqt_init_minmax_k(unsigned* mm, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { mm[2 * i] = 0xffffffffu; mm[2 * i + 1] = 0u; }
}

__global__ __launch_bounds__(256) void cqt_normalise_k(float* out, const unsigned* mm, long per_clip) {
    const int b = blockIdx.y;
    const float mn = cqt_ord2f(mm[2 * b]), mx = cqt_ord2f(mm[2 * b + 1]);
    const float den = mx - mn;             // no epsilon, as model/utils.py:100
    float* o = out + (long)b * per_clip;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_clip; i += (long)gridDim.x * blockDim.x)
        o[i] = (o[i] - mn) / den;
}

static long cqt_align(long bytes) { return (bytes + 255) & ~255L; }
static long cqt_lp(int T, int hop, int kernel_width) { return (((long)(T - 1) * hop + kernel_width) + 3) & ~3L; }

extern "C" {

// bytes of the workspace rv_cqt_lognorm_fwd needs: padded audio, per-item partial sums, 2*B uint32 min / max
long rv_cqt_workspace_bytes(int B, int nsamp, int n_items, int hop, int kernel_width) {
    if (B < 1 || nsamp < 1 || n_items < 1 || hop < 1 || kernel_width < 1) return -1;
    const int T = 1 + nsamp / hop;
    return cqt_align((long)B * cqt_lp(T, hop, kernel_width) * 4) + cqt_align((long)B * n_items * T * 32 * 4) + cqt_align(8L * B);
}

// audio [B, nsamp] (row stride audio_stride floats) -> out [B, T, n_bins], T = 1 + nsamp/hop (center=True, reflect pad
// kernel_width/2).  w / items / groups / scale: the packed tables of reconvat_amd.frontend.CQT1992v2.tables().
// do_log: log(|cqt| + 1e-5); normalise: per-clip min-max ("imagewise").
int rv_cqt_lognorm_fwd(const float* audio, long audio_stride, int B, int nsamp, const float* w, long w_floats, const int* items, int n_items,
                       const int* groups, int n_groups, const float* scale, int n_bins, int kernel_width, int hop, int do_log,
                       int normalise, float* out, int T, void* workspace, long workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RV_CHECK_ARG(audio && w && items && groups && scale && out && workspace, "rv_cqt_lognorm_fwd: null pointer");
    RV_CHECK_ARG(B >= 1 && B <= 65535, "rv_cqt_lognorm_fwd: batch %d out of range", B);
    RV_CHECK_ARG(kernel_width >= 16 && kernel_width % 16 == 0, "rv_cqt_lognorm_fwd: kernel_width %d must be a multiple of 16", kernel_width);
    RV_CHECK_ARG(nsamp > kernel_width / 2, "rv_cqt_lognorm_fwd: signal of %d samples not longer than the reflect padding (%d)",
                 nsamp, kernel_width / 2);
    RV_CHECK_ARG(hop >= 4 && hop % 4 == 0, "rv_cqt_lognorm_fwd: hop %d must be a positive multiple of 4", hop);
    RV_CHECK_ARG(T == 1 + nsamp / hop, "rv_cqt_lognorm_fwd: T=%d but 1 + nsamp/hop = %d", T, 1 + nsamp / hop);
    RV_CHECK_ARG(audio_stride >= nsamp, "rv_cqt_lognorm_fwd: row stride %ld < nsamp %d", audio_stride, nsamp);
    RV_CHECK_ARG(n_bins >= 1 && n_groups == (n_bins + 15) / 16, "rv_cqt_lognorm_fwd: %d groups for %d bins", n_groups, n_bins);
    RV_CHECK_ARG(w_floats >= 32, "rv_cqt_lognorm_fwd: empty tap table");
    RV_CHECK_ARG(n_items >= n_groups && n_items <= 65535, "rv_cqt_lognorm_fwd: %d work items", n_items);
    RV_CHECK_ARG((((uintptr_t)w) & 15) == 0 && (((uintptr_t)workspace) & 15) == 0, "rv_cqt_lognorm_fwd: w / workspace not 16-byte aligned");
    const long need = rv_cqt_workspace_bytes(B, nsamp, n_items, hop, kernel_width);
    RV_CHECK_ARG(workspace_bytes >= need, "rv_cqt_lognorm_fwd: workspace of %ld bytes, %ld needed", workspace_bytes, need);
    const long lp = cqt_lp(T, hop, kernel_width);
    char* ws = (char*)workspace;
    float* xpad = (float*)ws;
    float* part = (float*)(ws + cqt_align((long)B * lp * 4));
    unsigned* mm = (unsigned*)(ws + cqt_align((long)B * lp * 4) + cqt_align((long)B * n_items * T * 32 * 4));
    // every item's tap window lies inside [0, kernel_width) and its taps inside w (checked per item on the device, where the
    // tables live), hence every audio read is < (T - 1) * hop + kernel_width <= lp
    hipLaunchKernelGGL(cqt_pad_k, dim3(cdiv(lp, 1024), B), dim3(256), 0, st, audio, audio_stride, nsamp, kernel_width / 2,
                       (long)(T - 1) * hop + kernel_width, xpad, lp);
    RV_LAUNCH_CHECK("rv_cqt_lognorm_fwd(pad)");
    CqtArgs a;
    a.xpad = xpad; a.lp = lp; a.w = w; a.w_floats = w_floats; a.kernel_width = kernel_width; a.items = items; a.part = part; a.n_items = n_items; a.T = T; a.hop = hop;
    hipLaunchKernelGGL(cqt_band_k, dim3(cdiv(T, CQT_FT), n_items, B), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_cqt_lognorm_fwd(band)");
    hipLaunchKernelGGL(cqt_init_minmax_k, dim3(cdiv(B, 64)), dim3(64), 0, st, mm, B);
    const long per = (long)T * n_bins;
    hipLaunchKernelGGL(cqt_finish_k, dim3(cdiv(per, 256), B), dim3(256), 0, st, part, groups, scale, n_items, T, n_bins, do_log,
                       out, mm);
    RV_LAUNCH_CHECK("rv_cqt_lognorm_fwd(finish)");
    if (normalise) {
        hipLaunchKernelGGL(cqt_normalise_k, dim3(cdiv(per, 1024), B), dim3(256), 0, st, out, mm, per);
        RV_LAUNCH_CHECK("rv_cqt_lognorm_fwd(normalise)");
    }
    return RV_OK;
}

}  // extern "C"
