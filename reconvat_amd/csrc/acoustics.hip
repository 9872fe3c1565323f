// Acoustic augmentation of the device feed: one long FIR per item plus counter-based white noise,
//
//   y[b][m] = sum_{j < W} h[b][j] x[b][m + lead - j] + noise_b[m],   m = 0 .. n-1,   x[b][.] = 0 outside [0, n)
//
// (reconvat_amd/acoustics.py has the definition).  A 0.25 .. 0.5 s room tail is W = 4160 .. 8256 taps: 2 W n flops per item, on
// v_mfma_f32_16x16x4_f32 with no wasted product.  For outputs m = 16 a + b' and s = b' + lead - j:
//     y[16 a + b'] = sum_s h[b' + lead - s] x[16 a + s]
// A[b'][s] = h[b' + lead - s] is a 16-row Toeplitz matrix (zero outside [0, W)), B[s][a] = x[16 a + s] a Hankel matrix with column
// stride 16, D[b'][a] a GEMM with M = 16, one column per 16 outputs and K = W + 16.  Neither matrix is ever formed.
//
// One workgroup = one item x FIR_TILE = 2048 consecutive outputs (128 columns = 8 MFMA column tiles), 4 waves.  Staged in LDS:
//   hr   the item's filter reversed between two zero margins: hr[16 + u] = h[W - 1 - u], so that with t = s - (lead - W) the Toeplitz
//        operand is A[b'][t] = hr[15 + t - b'] -- a lane's four taps of a block are four ascending dwords;
//   xs   the tile's window x[tile0 + lead - W + i], i < FIR_TILE + W, every read outside [0, n) of the item's OWN row replaced by 0
//        with a select (whatever memory holds there); rows of 16 floats are 20 apart, so that the 16-byte Hankel reads of the 16
//        columns of a tile spread over the banks.  B[t][a] = xs[16 a + t]: four consecutive t are one 16-byte read.
// K is permuted inside a 16-tap block as in cqt_band_k (MFMA j of the block takes tap 4 kq + j).  The waves split K: wave w takes
// blocks w, w + 4, .. for all 8 column tiles (one Toeplitz fetch feeds 32 MFMAs), and the four partial tiles are summed in LDS in
// wave order 0, 1, 2, 3.  The order of every output's sum depends on W, lead and m alone: not on B, not on the item's place in the
// batch, not on n.  No atomics.  The noise is one float32 multiply and one float32 add in the epilogue; stores are plain.
#include "common.h"

#define FIR_TILE 2048            // outputs per workgroup
#define FIR_CT (FIR_TILE / 256)  // MFMA column tiles (16 columns x 16 outputs) per workgroup
#define FIR_ROW 20               // LDS floats per 16-sample row of the window
#define FIR_MAX_W 8256

struct FirArgs {
    const float* x; long x_stride;
    const float* h;
    const unsigned* seed; const float* amp;
    float* y; long y_stride;
    long n;
    int W, lead;
};

__device__ __forceinline__ unsigned fir_lowbias32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ static inline int fir_xs_floats(int W) { return (FIR_TILE + W) / 16 * FIR_ROW; }
static inline int fir_lds_floats(int W) {
    const int need = fir_xs_floats(W) + W + 32, red = 4 * FIR_CT * 64 * 4;
    return need > red ? need : red;
}

__global__ __launch_bounds__(256) void fir_items_k(FirArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fir_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int W = a.W, item = blockIdx.y;
    const long tile0 = (long)blockIdx.x * FIR_TILE;
    float* xs = fir_lds;
    float* hr = fir_lds + fir_xs_floats(W);
    // the reversed filter between its zero margins
    const float* h = a.h + (long)item * W;
    for (int i = tid; i < W + 32; i += 256) {
        const int u = i - 16;
        hr[i] = (u >= 0 && u < W) ? h[W - 1 - u] : 0.f;
    }
    // the window: sample tile0 + lead - W + i of the item's row, zero outside [0, n)
    const float* xrow = a.x + (long)item * a.x_stride;
    const long g0 = tile0 + a.lead - W;
    for (int i = tid; i < FIR_TILE + W; i += 256) {
        const long g = g0 + i;
        const bool in = g >= 0 && g < a.n;
        const float v = xrow[in ? g : 0];
        xs[(i >> 4) * FIR_ROW + (i & 15)] = in ? v : 0.f;
    }
    __syncthreads();

    f32x4 acc[FIR_CT];
#pragma unroll
    for (int c = 0; c < FIR_CT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nblk = (W + 16) >> 4;
    const float* ha = hr + 15 - li + 4 * kq;                       // + 16 blk + j
    const float* xa = xs + li * FIR_ROW + 4 * kq;                  // + (16 c + blk) FIR_ROW
    int blk = wave;
    f32x4 xv[FIR_CT], hv;
    if (blk < nblk) {
#pragma unroll
        for (int c = 0; c < FIR_CT; ++c) xv[c] = *reinterpret_cast<const f32x4*>(xa + (16 * c + blk) * FIR_ROW);
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = ha[16 * blk + j];
    }
    for (; blk < nblk; blk += 4) {
        f32x4 xn[FIR_CT], hn;
        const int nx = blk + 4 < nblk ? blk + 4 : blk;             // prefetch the wave's next block (last: reload)
#pragma unroll
        for (int c = 0; c < FIR_CT; ++c) xn[c] = *reinterpret_cast<const f32x4*>(xa + (16 * c + nx) * FIR_ROW);
#pragma unroll
        for (int j = 0; j < 4; ++j) hn[j] = ha[16 * nx + j];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < FIR_CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[j], xv[c][j], acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < FIR_CT; ++c) xv[c] = xn[c];
        hv = hn;
    }
    __syncthreads();                                               // every wave is done with xs / hr: the partial tiles go there
    f32x4* red = reinterpret_cast<f32x4*>(fir_lds);                // [4 waves][FIR_CT][64 lanes]
#pragma unroll
    for (int c = 0; c < FIR_CT; ++c) red[(wave * FIR_CT + c) * 64 + lane] = acc[c];
    __syncthreads();
    // output o of the tile = 256 c + 16 column + row: lane (column, row >> 2) of tile c holds it as element row & 3
    const float* redf = fir_lds;
    float* yrow = a.y + (long)item * a.y_stride;
    const bool noisy = a.seed != nullptr;
    const unsigned seed = noisy ? a.seed[item] : 0u;
    const float amp = noisy ? a.amp[item] : 0.f;
    for (int o = tid; o < FIR_TILE; o += 256) {
        const long m = tile0 + o;
        if (m >= a.n) break;
        const int c = o >> 8, col = (o >> 4) & 15, row = o & 15;
        const int at = ((c * 64 + col + 16 * (row >> 2)) << 2) + (row & 3);
        float v = redf[at];
        v += redf[at + 1 * FIR_CT * 256];
        v += redf[at + 2 * FIR_CT * 256];
        v += redf[at + 3 * FIR_CT * 256];
        if (noisy) {
            const unsigned r = fir_lowbias32(seed ^ fir_lowbias32((unsigned)m + 0x9E3779B9u));
            const int t = (int)(r & 0xFFFFu) + (int)(r >> 16) - 65535;
            v = __fadd_rn(v, __fmul_rn((float)t, amp));
        }
        yrow[m] = v;
    }
}

extern "C" {

// x [B] rows of n samples (row stride x_stride floats), h [B][W] one filter per item (16-byte aligned), y [B] rows of n samples (row
// stride y_stride); x and y must not overlap.  seed / amp [B], both null: no noise.
int rv_fir_items(const float* x, long x_stride, const float* h, int W, int lead, const unsigned* seed, const float* amp, int B, long n,
                 float* y, long y_stride, void* stream) {
    RV_CHECK_ARG(x && h && y, "rv_fir_items: null pointer");
    RV_CHECK_ARG((seed == nullptr) == (amp == nullptr), "rv_fir_items: seed and amp go together (both or neither)");
    RV_CHECK_ARG(W >= 16 && W <= FIR_MAX_W && W % 16 == 0, "rv_fir_items: W %d must be a multiple of 16 in [16, %d]", W, FIR_MAX_W);
    RV_CHECK_ARG(lead >= 0 && lead < W, "rv_fir_items: lead %d outside [0, %d)", lead, W);
    RV_CHECK_ARG(n >= 1 && n < (1L << 31), "rv_fir_items: n %ld outside [1, 2^31)", n);
    RV_CHECK_ARG(x_stride >= n && y_stride >= n, "rv_fir_items: row stride (%ld, %ld) smaller than n %ld", x_stride, y_stride, n);
    RV_CHECK_ARG(B >= 1 && B <= 65535, "rv_fir_items: batch %d outside [1, 65535]", B);
    RV_CHECK_ARG((((uintptr_t)h) & 15) == 0, "rv_fir_items: h must be 16-byte aligned");
    const int lds = fir_lds_floats(W) * (int)sizeof(float);        // at most 85 KB (W = 8256)
    static int granted = 0;
    if (lds > 64 * 1024 && !granted) {
        if (hipFuncSetAttribute((const void*)fir_items_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                fir_lds_floats(FIR_MAX_W) * (int)sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            rv_set_error("rv_fir_items: the device refused %d bytes of LDS per workgroup", lds);
            return RV_EUNSUPPORTED;
        }
        granted = 1;
    }
    FirArgs a;
    a.x = x; a.x_stride = x_stride; a.h = h; a.seed = seed; a.amp = amp; a.y = y; a.y_stride = y_stride; a.n = n; a.W = W; a.lead = lead;
    hipLaunchKernelGGL(fir_items_k, dim3((unsigned)((n + FIR_TILE - 1) / FIR_TILE), B), dim3(256), (size_t)lds, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK("rv_fir_items");
    return RV_OK;
}

}  // extern "C"
