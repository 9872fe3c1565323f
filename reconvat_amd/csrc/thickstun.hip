// Thickstun CNN baseline (reference model/Thickstun_model.py:17-35, 57-61) in its window-sharing form.
//
// The reference turns every frame into its own 229 x 25 window and runs Conv2d(1,128,(128,1),stride=(2,1)), Conv2d(128,4096,(1,25)) and
// Linear(4096*51, 88) on a batch of T windows.  The windows overlap by 24 frames and the first convolution is 1 wide in time, so
//   z2 = relu(CNN_freq(.)) is computed ONCE per frame of the zero-padded spectrogram, stored channels-last [B, 51, T+24, 128], and
//   z3[b,t,f,n] = relu(bias[n] + sum_{j<25} sum_{c<128} z2[b,f,t+j,c] * W[n,c,j])
// is a GEMM whose A operand is a Hankel view of z2: the 25 x 128 inputs of output row (b,f,t) are the contiguous 3200 floats that start at
// ((b*51+f)*(T+24)+t)*128.  z3 is stored [B, T, 51, 4096] so that a frame's 208 896 features are contiguous for the linear layer.
//
//   rv_thick_freq_fwd    spectrogram -> z2 (bias + ReLU, padded frames = relu(bias))
//   rv_thick_freq_bwd    weight / bias gradient of CNN_freq from dz2 (ReLU mask of z2 in the operand load), fixed-order partial sums
//   rv_thick_tconv_fwd   the Hankel GEMM with the A operand stationary in LDS, bias + ReLU epilogue
//   rv_thick_linear_dz   dz3 = (z3 > 0) * (dY @ W): the input gradient of the linear layer with the ReLU mask of z3 in its epilogue
//
// The input- and weight-gradient GEMMs of the time convolution and the other two linear GEMMs run on rv_gemm (gemm.hip) through strided
// views (reconvat_amd/ops.py, thick_*).  All arithmetic is f32 on v_mfma_f32_16x16x4_f32 (the frequency convolution, 0.04 % of a step, on the
// vector ALU).  Element counts exceed 2^31 (z3 has 133 693 440 * B elements): every global index is a long.
#include "common.h"
#include <mutex>

#define TK_F 51          // output rows of the frequency convolution: (229 - 128) / 2 + 1
#define TK_BINS 229
#define TK_C 128         // channels of z2 = taps of the frequency convolution
#define TK_TAPS 25
#define TK_LDA 132       // LDS row stride of a staged z2 row (128 + 4: the 16 lanes of a ds_read_b128 group fall on distinct 16-byte slots)

// ---- frequency convolution ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (padded frame, clip), one thread per output channel: the thread keeps its 128 taps in registers, the frame sits in LDS.
__global__ __launch_bounds__(TK_C) void thick_freq_fwd_k(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ z2, int Tin, int pad) {
    __shared__ float xs[TK_BINS + 3];
    const int c = threadIdx.x, tp = blockIdx.x, b = blockIdx.y;
    const int Tp = Tin + 2 * pad, t = tp - pad;
    const float bc = bias[c];
    float* out = z2 + ((long)b * TK_F * Tp + tp) * TK_C + c;
    const long fs = (long)Tp * TK_C;
    if (t < 0 || t >= Tin) {                      // a zero frame of the reference's F.pad: the convolution of zeros is the bias
        const float v = fmaxf(bc, 0.f);
        for (int f = 0; f < TK_F; ++f) out[f * fs] = v;
        return;
    }
    const float* xr = x + ((long)b * Tin + t) * TK_BINS;
    for (int i = c; i < TK_BINS; i += TK_C) xs[i] = xr[i];
    float wr[TK_C];
#pragma unroll
    for (int k = 0; k < TK_C; ++k) wr[k] = w[c * TK_C + k];
    __syncthreads();
    for (int f = 0; f < TK_F; ++f) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < TK_C; ++k) acc = fmaf(xs[2 * f + k], wr[k], acc);
        out[f * fs] = fmaxf(acc + bc, 0.f);
    }
}

// Weight / bias gradient, first half: workgroup q owns TK_FR consecutive padded frames and parks its partial sums
//   part[q][tap][c] = sum_{frames, f} dz2m[b,f,tp,c] * x[b,t,2f+tap],   partb[q][c] = sum dz2m      (dz2m = dz2 where z2 > 0)
// thread = (channel, half of the taps); the second kernel adds the partials in q order (no float atomics: run-to-run reproducible).
#define TK_FR 8
__global__ __launch_bounds__(256) void thick_freq_bwd_k(const float* __restrict__ dz2, const float* __restrict__ z2, const float* __restrict__ x,
                                                        float* __restrict__ part, int B, int Tin, int pad) {
    __shared__ float xs[TK_BINS + 3];
    const int tid = threadIdx.x, c = tid & (TK_C - 1), half = tid >> 7;
    const int Tp = Tin + 2 * pad;
    const long nfr = (long)B * Tp;
    float acc[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) acc[k] = 0.f;
    float bsum = 0.f;
    for (int i = 0; i < TK_FR; ++i) {
        const long q = (long)blockIdx.x * TK_FR + i;
        if (q >= nfr) break;                                   // (uniform over the workgroup)
        const int b = (int)(q / Tp), tp = (int)(q - (long)b * Tp), t = tp - pad;
        const bool real = t >= 0 && t < Tin;
        __syncthreads();
        if (real && tid < TK_BINS) xs[tid] = x[((long)b * Tin + t) * TK_BINS + tid];
        __syncthreads();
        const long base = ((long)b * TK_F * Tp + tp) * TK_C + c;
        for (int f = 0; f < TK_F; ++f) {
            const long o = base + (long)f * Tp * TK_C;
            const float d = z2[o] > 0.f ? dz2[o] : 0.f;
            if (half == 0) bsum += d;
            if (real) {
#pragma unroll
                for (int k = 0; k < 64; ++k) acc[k] = fmaf(d, xs[2 * f + half * 64 + k], acc[k]);
            }
        }
    }
    float* mine = part + (long)blockIdx.x * (TK_C * TK_C + TK_C);
#pragma unroll
    for (int k = 0; k < 64; ++k) mine[(half * 64 + k) * TK_C + c] = acc[k];
    if (half == 0) mine[TK_C * TK_C + c] = bsum;
}

__global__ __launch_bounds__(256) void thick_freq_bwd_fold_k(const float* __restrict__ part, int nq, float* __restrict__ dw, float* __restrict__ db,
                                                             int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;             // [tap][c] for i < 16384, then the bias
    if (i >= TK_C * TK_C + TK_C) return;
    float s = 0.f;
    for (int q = 0; q < nq; ++q) s += part[(long)q * (TK_C * TK_C + TK_C) + i];
    float* dst = i < TK_C * TK_C ? dw + (i & (TK_C - 1)) * TK_C + (i >> 7) : db + (i - TK_C * TK_C);
    *dst = accumulate ? *dst + s : s;
}

// ---- time convolution, forward -----------------------------------------------------------------------------------------------------------------
// A workgroup owns TT consecutive t of one (b, f).  Those outputs read only TT + 24 rows of z2 for ALL 3200 values of k: the rows are staged in
// LDS once ((TT + 24) x 132 floats; 80 256 bytes at TT = 128, two workgroups per CU) and only the weights are streamed, straight from global
// memory into MFMA operands.  Four waves, each TT x 32 outputs of a 128-column pass; blockIdx.z splits the 4096 columns.
// Weights come as wj[j][n][c] (rv_pack_weights, plain, taps = 25): lane (li, g) of a wave loads the 16 bytes wj[j][n0 + li][c0 + 4g .. +3] and
// feeds them to four consecutive MFMAs, i.e. MFMA s of a 16-wide k chunk multiplies k = c0 + 4g + s -- any assignment of k to (g, s) is a valid
// GEMM as long as both operands use the same one; the A fragment is the matching ds_read_b128 of row t + j.
// The D^T = W A^T form of gemm.hip: an accumulator lane holds four consecutive n of one t (16-byte stores).
// Every output element sees the same k order whatever tile it falls in, so a chunked evaluation equals the unchunked one bit for bit.
template <int TT>
__global__ __launch_bounds__(256) void thick_tconv_fwd_k(const float* __restrict__ z2, const float* __restrict__ wj, const float* __restrict__ bias,
                                                         float* __restrict__ z3, int T, int N, int ncols) {
    constexpr int TY = TT / 16, ROWS = TT + TK_TAPS - 1;
    extern __shared__ __attribute__((aligned(16))) float tk_as[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const int t0 = blockIdx.x * TT, bf = blockIdx.y, b = bf / TK_F, f = bf - b * TK_F;
    const int Tp = T + TK_TAPS - 1;
    const float* src = z2 + ((long)bf * Tp + t0) * TK_C;
    for (int idx = tid; idx < ROWS * (TK_C / 4); idx += 256) {
        const int row = idx >> 5, c4 = (idx & 31) * 4;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (t0 + row < Tp) v = *reinterpret_cast<const f32x4*>(src + (long)row * TK_C + c4);
        *reinterpret_cast<f32x4*>(tk_as + row * TK_LDA + c4) = v;
    }
    __syncthreads();
    constexpr int NCH = TK_TAPS * (TK_C / 16);                 // 200 chunks of 16 k
    for (int np = 0; np < ncols; np += 128) {
        const int n_base = blockIdx.z * ncols + np + wave * 32;
        f32x4 acc[2][TY], tap[2][TY];      // tap: the 128 products of one tap; acc: the 25 tap sums (blocked summation: rounding grows with
                                           // sqrt(128) + sqrt(25) instead of sqrt(3200) steps)
#pragma unroll
        for (int xx = 0; xx < 2; ++xx)
#pragma unroll
            for (int y = 0; y < TY; ++y) acc[xx][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* w0 = wj + (long)(n_base + li) * TK_C + 4 * g;
        const long wx = 16L * TK_C, wjs = (long)N * TK_C;
        f32x4 wn[2];
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) wn[xx] = *reinterpret_cast<const f32x4*>(w0 + xx * wx);
        for (int kc = 0; kc < NCH; ++kc) {
            if ((kc & 7) == 0) {
#pragma unroll
                for (int xx = 0; xx < 2; ++xx)
#pragma unroll
                    for (int y = 0; y < TY; ++y) tap[xx][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            f32x4 wc[2] = {wn[0], wn[1]};
            if (kc + 1 < NCH) {                                // the next chunk's weights leave while this one is multiplied
                const float* wp = w0 + (long)((kc + 1) >> 3) * wjs + ((kc + 1) & 7) * 16;
#pragma unroll
                for (int xx = 0; xx < 2; ++xx) wn[xx] = *reinterpret_cast<const f32x4*>(wp + xx * wx);
            }
            const int j = kc >> 3, c0 = (kc & 7) * 16;
            f32x4 av[TY];
#pragma unroll
            for (int y = 0; y < TY; ++y) av[y] = *reinterpret_cast<const f32x4*>(tk_as + (y * 16 + li + j) * TK_LDA + c0 + 4 * g);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int xx = 0; xx < 2; ++xx)
#pragma unroll
                    for (int y = 0; y < TY; ++y)
                        tap[xx][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[xx][s], av[y][s], tap[xx][y], 0, 0, 0);
            if ((kc & 7) == 7) {
#pragma unroll
                for (int xx = 0; xx < 2; ++xx)
#pragma unroll
                    for (int y = 0; y < TY; ++y) acc[xx][y] += tap[xx][y];
            }
        }
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) {
            const int nb = n_base + xx * 16 + 4 * g;
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + nb);
#pragma unroll
            for (int y = 0; y < TY; ++y) {
                const int t = t0 + y * 16 + li;
                if (t >= T) continue;
                f32x4 v = acc[xx][y] + bv;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                *reinterpret_cast<f32x4*>(z3 + (((long)b * T + t) * TK_F + f) * N + nb) = v;
            }
        }
    }
}

template <int TT>
static void launch_tconv_fwd(const float* z2, const float* wj, const float* bias, float* z3, int B, int T, int N, int ns, hipStream_t st) {
    constexpr size_t lds = (size_t)(TT + TK_TAPS - 1) * TK_LDA * sizeof(float);
    static std::once_flag once;
    std::call_once(once, [] { (void)hipFuncSetAttribute((const void*)thick_tconv_fwd_k<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    hipLaunchKernelGGL((thick_tconv_fwd_k<TT>), dim3(cdiv(T, TT), TK_F * B, ns), dim3(256), lds, st, z2, wj, bias, z3, T, N, N / ns);
}

// ---- linear layer, input gradient --------------------------------------------------------------------------------------------------------------
// dz3[m][k] = z3[m][k] > 0 ? sum_n dy[m][n] * wt[k][n] : 0.   dy: [M, N] (N = 88 logit gradients), wt: [K, N] (the linear weight in z3's feature
// order, transposed), z3 / dz3: [M, K].  64 x 256 outputs per workgroup, the reduction (N <= 96) in chunks of 16 with the k assignment of
// thick_tconv_fwd_k; the mask costs one extra read of z3 in the epilogue instead of a separate pass over dz3.
#define TK_LDD 100
__global__ __launch_bounds__(256) void thick_linear_dz_k(const float* __restrict__ dy, const float* __restrict__ wt, const float* __restrict__ z3,
                                                         float* __restrict__ dz3, long M, long K, int N) {
    __shared__ __attribute__((aligned(16))) float ds[64 * TK_LDD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
    const long m0 = (long)blockIdx.y * 64, c0 = (long)blockIdx.x * 256 + wave * 64;
    for (int idx = tid; idx < 64 * 96; idx += 256) {
        const int row = idx / 96, n = idx - row * 96;
        ds[row * TK_LDD + n] = (m0 + row < M && n < N) ? dy[(m0 + row) * N + n] : 0.f;
    }
    __syncthreads();
    f32x4 acc[4][4];
#pragma unroll
    for (int xx = 0; xx < 4; ++xx)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[xx][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nch = (N + 15) / 16;
    for (int kc = 0; kc < nch; ++kc) {
        const int k = kc * 16 + 4 * g;
        f32x4 wv[4], dv[4];
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
            const long col = c0 + xx * 16 + li;
            wv[xx] = (col < K && k < N) ? *reinterpret_cast<const f32x4*>(wt + col * N + k) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int y = 0; y < 4; ++y) dv[y] = *reinterpret_cast<const f32x4*>(ds + (y * 16 + li) * TK_LDD + k);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int xx = 0; xx < 4; ++xx)
#pragma unroll
                for (int y = 0; y < 4; ++y)
                    acc[xx][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[xx][s], dv[y][s], acc[xx][y], 0, 0, 0);
    }
#pragma unroll
    for (int xx = 0; xx < 4; ++xx)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const long m = m0 + y * 16 + li, col = c0 + xx * 16 + 4 * g;
            if (m >= M || col >= K) continue;
            const f32x4 z = *reinterpret_cast<const f32x4*>(z3 + m * K + col);
            f32x4 v = acc[xx][y];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = z[r] > 0.f ? v[r] : 0.f;
            *reinterpret_cast<f32x4*>(dz3 + m * K + col) = v;
        }
}

extern "C" {

int rv_thick_freq_fwd(const float* x, const float* w, const float* bias, float* z2, int B, int Tin, int pad, void* stream) {
    RV_CHECK_ARG(x && w && bias && z2, "rv_thick_freq_fwd: null pointer");
    RV_CHECK_ARG(B > 0 && B < 65536 && Tin > 0 && pad >= 0, "rv_thick_freq_fwd: bad shape B=%d T=%d pad=%d", B, Tin, pad);
    hipLaunchKernelGGL(thick_freq_fwd_k, dim3(Tin + 2 * pad, B), dim3(TK_C), 0, (hipStream_t)stream, x, w, bias, z2, Tin, pad);
    RV_LAUNCH_CHECK("rv_thick_freq_fwd");
    return RV_OK;
}

long rv_thick_freq_bwd_workspace_bytes(int B, int Tin, int pad) {
    return (long)cdiv((long)B * (Tin + 2 * pad), TK_FR) * (TK_C * TK_C + TK_C) * 4;
}

int rv_thick_freq_bwd(const float* dz2, const float* z2, const float* x, float* dw, float* db, int B, int Tin, int pad, int accumulate,
                      void* ws, long ws_bytes, void* stream) {
    RV_CHECK_ARG(dz2 && z2 && x && dw && db && ws, "rv_thick_freq_bwd: null pointer");
    RV_CHECK_ARG(B > 0 && Tin > 0 && pad >= 0, "rv_thick_freq_bwd: bad shape B=%d T=%d pad=%d", B, Tin, pad);
    RV_CHECK_ARG(ws_bytes >= rv_thick_freq_bwd_workspace_bytes(B, Tin, pad), "rv_thick_freq_bwd: workspace too small");
    const int nq = cdiv((long)B * (Tin + 2 * pad), TK_FR);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(thick_freq_bwd_k, dim3(nq), dim3(256), 0, st, dz2, z2, x, (float*)ws, B, Tin, pad);
    RV_LAUNCH_CHECK("rv_thick_freq_bwd");
    hipLaunchKernelGGL(thick_freq_bwd_fold_k, dim3(cdiv(TK_C * TK_C + TK_C, 256)), dim3(256), 0, st, (const float*)ws, nq, dw, db, accumulate);
    RV_LAUNCH_CHECK("rv_thick_freq_bwd(fold)");
    return RV_OK;
}

int rv_thick_tconv_fwd(const float* z2, const float* wj, const float* bias, float* z3, int B, int T, int N, void* stream) {
    RV_CHECK_ARG(z2 && wj && bias && z3, "rv_thick_tconv_fwd: null pointer");
    RV_CHECK_ARG(B > 0 && T > 0 && (long)B * TK_F < 65536, "rv_thick_tconv_fwd: bad shape B=%d T=%d", B, T);
    RV_CHECK_ARG(N > 0 && N % 128 == 0, "rv_thick_tconv_fwd: N=%d must be a multiple of 128", N);
    RV_CHECK_ARG(((uintptr_t)z2 & 15) == 0 && ((uintptr_t)wj & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)z3 & 15) == 0,
                 "rv_thick_tconv_fwd: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int ns = 1;                                               // column slices over blockIdx.z: enough workgroups to cover the chip a few times
    while (ns < 8 && (N / 128) % (2 * ns) == 0) ns *= 2;
    if (T > 64) launch_tconv_fwd<128>(z2, wj, bias, z3, B, T, N, ns, st);
    else if (T > 16) launch_tconv_fwd<64>(z2, wj, bias, z3, B, T, N, ns, st);
    else launch_tconv_fwd<16>(z2, wj, bias, z3, B, T, N, ns, st);
    RV_LAUNCH_CHECK("rv_thick_tconv_fwd");
    return RV_OK;
}

int rv_thick_linear_dz(const float* dy, const float* wt, const float* z3, float* dz3, long M, long K, int N, void* stream) {
    RV_CHECK_ARG(dy && wt && z3 && dz3, "rv_thick_linear_dz: null pointer");
    RV_CHECK_ARG(M > 0 && K > 0 && K % 4 == 0 && N > 0 && N <= 96 && N % 4 == 0, "rv_thick_linear_dz: bad shape M=%ld K=%ld N=%d", M, K, N);
    RV_CHECK_ARG(cdiv(M, 64) < 65536, "rv_thick_linear_dz: M=%ld too large for one launch", M);
    RV_CHECK_ARG(((uintptr_t)wt & 15) == 0 && ((uintptr_t)z3 & 15) == 0 && ((uintptr_t)dz3 & 15) == 0,
                 "rv_thick_linear_dz: operands must be 16-byte aligned");
    hipLaunchKernelGGL(thick_linear_dz_k, dim3(cdiv(K, 256), cdiv(M, 64)), dim3(256), 0, (hipStream_t)stream, dy, wt, z3, dz3, M, K, N);
    RV_LAUNCH_CHECK("rv_thick_linear_dz");
    return RV_OK;
}

}  // extern "C"
