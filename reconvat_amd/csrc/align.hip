// Score-to-recording alignment: banded dynamic time warping over unit-norm feature rows.  reconvat_amd/align.py has
// the definition; in short, for a pair with N recording frames (rows i) and M score frames (columns j), row i owns the columns
// lo[i] .. lo[i] + W - 1 (cut off at M; lo non-decreasing, lo[0] = 0) and
//     c[i][k]  = rint(clip(1 - <x_i, y_{lo[i] + k}>, 0, 1) * 4095)                       uint16 [N][W], 0xFFFF where lo[i] + k >= M
//     D[0][0]  = 2 c,   D[i][j] = min(D[i-1][j-1] + 2 c, D[i-1][j] + c, D[i][j-1] + c)   uint32, a predecessor outside the band = inf
//     dirs     = 0 diagonal, 1 from (i-1, j), 2 from (i, j-1), 3 unreachable / start; ties go to the lowest code
// and the path is walked back from (N-1, M-1).  Twelve-bit costs and N + M <= 2^18 keep every sum below 2^30.
//
// Both kernels are batched over P pairs through one int64 descriptor table ON THE DEVICE, ALIGN_DESC words per pair:
//     N, M, W, then the ELEMENT offsets of X, Y (in feats), lo, cost, dirs and out in their buffers.
// The host cannot see the table, so every buffer arrives with its length and a kernel checks each pair's row against them
// (align_sizes_ok, align_fits): a pair that does not fit touches nothing but the status word of its output header, if that is in range.
//
// align_cost_k   a banded GEMM on v_mfma_f32_16x16x4_f32.  One workgroup = 32 rows of one pair, 4 waves; a wave multiplies the 32
//                rows with 32 consecutive columns (2 x 2 accumulator tiles), column tiles lo[i0] + 32 t dealt round-robin to the
//                waves (and to gridDim.y workgroups) up to lo[i_last] + W.  Operands come straight from global memory (a tile is
//                re-read from L1 / L2: the whole product is a few GFLOP), 16 K per step with the K permutation of cqt.hip (MFMA j of
//                a step takes element 4 kq + j of both operands), a guarded K tail, row and column indices clamped into the matrix
//                for the loads and masked in the epilogue.  Columns >= M inside a row's band get 0xFFFF.
// align_dtw_k    recurrence and backtrack, one workgroup per pair, anti-diagonal wavefront.  On diagonal d = i + j the rows inside the
//                band are one interval [imin, imax] (i + lo[i] and i + min(lo[i] + W, M) both strictly increase), at most W rows, both
//                ends moving forward only: every work item advances its own copy of the two ends.  Three diagonals of uint32 live in
//                LDS as rings indexed by i mod L, L = max W + 1; row i belongs to work item i mod blockDim for as long as it is in the
//                interval, so its cost and direction bytes are one sequential stream per work item and lo[i], lo[i-1] stay in
//                registers.  A predecessor is read only after its band membership is checked against lo, so a stale ring slot is
//                never used.  One barrier per diagonal.  Then one lane walks the direction bytes back.
// Plain stores, no atomics, no allocation, no synchronisation.
#include "common.h"

#define ALIGN_DESC 9
#define ALIGN_MAX_W 8192
#define ALIGN_MAX_NM (1 << 18)
#define ALIGN_MAX_D 4096
#define ALIGN_INF 0xFFFFFFFFu
#define ALIGN_PHASES 4                     // partial sums per cost cell (the pairwise add below is written for 4)
#define ALIGN_HEAD 4                       // out header: total (uint32 bits), path length, status (0 ok, -1 bad row), 0

struct AlignPair {
    long N, M, W, x, y, lo, cost, dirs, out;
};

__device__ __forceinline__ AlignPair align_load_pair(const long* desc, int p) {
    const long* r = desc + (long)p * ALIGN_DESC;
    AlignPair a;
    a.N = r[0]; a.M = r[1]; a.W = r[2]; a.x = r[3]; a.y = r[4]; a.lo = r[5]; a.cost = r[6]; a.dirs = r[7]; a.out = r[8];
    return a;
}

__device__ __forceinline__ bool align_fits(long off, long count, long total) { return off >= 0 && count >= 0 && off <= total - count; }

// the sizes of a pair (every product below stays under 2^18 * 8192 * 4096 < 2^63)
__device__ __forceinline__ bool align_sizes_ok(const AlignPair& a, int max_w, int max_nm) {
    return a.N >= 1 && a.M >= 1 && a.N + a.M <= (long)max_nm && a.W >= 1 && a.W <= (long)max_w && a.W <= a.M;
}

struct CostArgs {
    const long* desc;
    const float* feats; long n_feats;
    const int* lo; long n_lo;
    unsigned short* cost; long n_cost;
    int D, max_n, max_w;
};

__device__ __forceinline__ int align_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void align_cost_k(CostArgs g) {
    const AlignPair a = align_load_pair(g.desc, blockIdx.z);
    const int D = g.D;
    if (!align_sizes_ok(a, g.max_w, ALIGN_MAX_NM) || a.N > (long)g.max_n || !align_fits(a.x, a.N * D, g.n_feats) ||
        !align_fits(a.y, a.M * D, g.n_feats) || !align_fits(a.lo, a.N, g.n_lo) || !align_fits(a.cost, a.N * a.W, g.n_cost))
        return;
    const int N = (int)a.N, M = (int)a.M, W = (int)a.W;
    const int i0 = (int)blockIdx.x * 32;
    if (i0 >= N) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int* lo = g.lo + a.lo;
    const float* X = g.feats + a.x;
    const float* Y = g.feats + a.y;
    unsigned short* cost = g.cost + a.cost;
    const int i_last = min(i0 + 31, N - 1);
    const int c_begin = align_clampi(lo[i0], 0, M - 1);
    const int c_end = align_clampi(lo[i_last], 0, M - 1) + W;                                  // one past the tile's last band column
    // the lane's two operand rows of X (clamped: rows past N are computed and never stored) and the band starts of its output rows
    const float* xr0 = X + (long)min(i0 + li, N - 1) * D;
    const float* xr1 = X + (long)min(i0 + 16 + li, N - 1) * D;
    int lo_out[2][4];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) lo_out[ti][r] = lo[min(i0 + 16 * ti + 4 * kq + r, N - 1)];
    const int Dm = D & ~15;
    for (int t = wave + 4 * (int)blockIdx.y;; t += 4 * (int)gridDim.y) {
        const long cl = (long)c_begin + 32L * t;
        if (cl >= c_end) break;
        const int c = (int)cl;
        const float* yr0 = Y + (long)min(c + li, M - 1) * D;
        const float* yr1 = Y + (long)min(c + 16 + li, M - 1) * D;
        // ALIGN_PHASES partial sums per element, K steps dealt round-robin and added pairwise at the end: each chain is a quarter as long
        // and a quarter as large, which brings the rounding of the sum down to that of a pairwise float32 sum (tests/test_align_gpu.py)
        f32x4 part[ALIGN_PHASES][2][2];
#pragma unroll
        for (int ph = 0; ph < ALIGN_PHASES; ++ph)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) part[ph][ti][tj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < M) {                                                                           // a tile of dead columns multiplies nothing
            for (int k0 = 0; k0 < Dm; k0 += 16 * ALIGN_PHASES) {
#pragma unroll
                for (int ph = 0; ph < ALIGN_PHASES; ++ph) {
                    const int k = k0 + 16 * ph + 4 * kq;
                    if (k0 + 16 * ph >= Dm) break;                                             // (wave-uniform)
                    float xa[2][4], yb[2][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { xa[0][j] = xr0[k + j]; xa[1][j] = xr1[k + j]; yb[0][j] = yr0[k + j]; yb[1][j] = yr1[k + j]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                            for (int tj = 0; tj < 2; ++tj)
                                part[ph][ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ti][j], yb[tj][j], part[ph][ti][tj], 0, 0, 0);
                }
            }
            if (Dm < D) {                                                                      // K tail: elements past D are zeros
                const int k = Dm + 4 * kq;
                float xa[2][4], yb[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = k + j < D;
                    const int kk = in ? k + j : 0;
                    xa[0][j] = in ? xr0[kk] : 0.f; xa[1][j] = in ? xr1[kk] : 0.f;
                    yb[0][j] = in ? yr0[kk] : 0.f; yb[1][j] = in ? yr1[kk] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                        for (int tj = 0; tj < 2; ++tj)
                            part[ALIGN_PHASES - 1][ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ti][j], yb[tj][j], part[ALIGN_PHASES - 1][ti][tj], 0, 0, 0);
            }
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = (part[0][ti][tj] + part[1][ti][tj]) + (part[2][ti][tj] + part[3][ti][tj]);
        // element r of tile (ti, tj): row i0 + 16 ti + 4 kq + r, column c + 16 tj + li
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = i0 + 16 * ti + 4 * kq + r;
                    const long col = cl + 16 * tj + li;
                    const long kk = col - lo_out[ti][r];
                    if (i < N && kk >= 0 && kk < W) {
                        const float v = fminf(fmaxf(1.0f - acc[ti][tj][r], 0.0f), 1.0f);
                        cost[(long)i * W + kk] = col < M ? (unsigned short)(int)rintf(v * 4095.0f) : (unsigned short)0xFFFF;
                    }
                }
    }
}

struct DtwArgs {
    const long* desc;
    const int* lo; long n_lo;
    const unsigned short* cost; long n_cost;
    unsigned char* dirs; long n_dirs;
    int* out; long n_out;
    int max_w, max_nm, L;
};

__global__ __launch_bounds__(1024) void align_dtw_k(DtwArgs g) {
    extern __shared__ unsigned align_lds[];
    const AlignPair a = align_load_pair(g.desc, blockIdx.x);
    const int tid = threadIdx.x, bs = blockDim.x;
    const bool head_ok = align_fits(a.out, ALIGN_HEAD, g.n_out);
    if (!align_sizes_ok(a, g.max_w, g.max_nm) || !align_fits(a.lo, a.N, g.n_lo) || !align_fits(a.cost, a.N * a.W, g.n_cost) ||
        !align_fits(a.dirs, a.N * a.W, g.n_dirs) || !align_fits(a.out, ALIGN_HEAD + 2 * (a.N + a.M), g.n_out)) {
        if (head_ok && tid == 0) {
            int* h = g.out + a.out;
            h[0] = (int)ALIGN_INF; h[1] = 0; h[2] = -1; h[3] = 0;
        }
        return;
    }
    const int N = (int)a.N, M = (int)a.M, W = (int)a.W, L = g.L;
    const int* __restrict__ lo = g.lo + a.lo;
    const unsigned short* __restrict__ cost = g.cost + a.cost;
    unsigned char* dirs = g.dirs + a.dirs;
    int* head = g.out + a.out;
    int* row_lo = head + ALIGN_HEAD;
    int* row_hi = row_lo + N;
    int* col_lo = row_hi + N;
    int* col_hi = col_lo + M;
    unsigned* ring0 = align_lds;                       // diagonal d
    unsigned* ring1 = align_lds + L;                   // diagonal d - 1
    unsigned* ring2 = align_lds + 2 * L;               // diagonal d - 2

    int imin = 0, imax = -1;                           // the interval of diagonal d, every work item its own copy
    int ci = -1, lo_i = 0, lo_p = 0, hi_p = 0;         // the row this work item last handled, its band start and the previous row's band
    const int n_diag = N + M - 1;
    for (int d = 0; d < n_diag; ++d) {
        while (imax + 1 < N) {                         // rows enter when i + lo[i] <= d
            const int l = align_clampi(lo[imax + 1], 0, M - 1);
            if (imax + 1 + l > d) break;
            ++imax;
        }
        while (imin < N) {                             // and leave when i + min(lo[i] + W, M) <= d
            const int l = align_clampi(lo[imin], 0, M - 1);
            if (imin + min(l + W, M) > d) break;
            ++imin;
        }
        int first = imin + (tid - imin % bs + bs) % bs;              // the lowest row >= imin that is tid mod bs
        for (int i = first; i <= imax; i += bs) {
            if (i != ci) {
                ci = i;
                lo_i = align_clampi(lo[i], 0, M - 1);
                lo_p = i ? align_clampi(lo[i - 1], 0, M - 1) : 0;
                hi_p = i ? min(lo_p + W, M) : 0;                     // row -1 owns no column
            }
            const int j = d - i, k = j - lo_i;
            if (k < 0 || k >= W || j >= M) continue;                 // (cannot happen for a non-decreasing lo; a malformed one)
            const unsigned c = cost[(long)i * W + k];
            const int slot = i % L, slot_p = (i + L - 1) % L;
            const bool in_up = j >= lo_p && j < hi_p, in_dg = j - 1 >= lo_p && j - 1 < hi_p, in_lf = k >= 1;
            const unsigned up = in_up ? ring1[slot_p] : ALIGN_INF;
            const unsigned dg = in_dg ? ring2[slot_p] : ALIGN_INF;
            const unsigned lf = in_lf ? ring1[slot] : ALIGN_INF;
            unsigned best = dg == ALIGN_INF ? ALIGN_INF : dg + 2u * c;
            unsigned code = dg == ALIGN_INF ? 3u : 0u;
            const unsigned vu = up == ALIGN_INF ? ALIGN_INF : up + c;
            if (vu < best) { best = vu; code = 1u; }
            const unsigned vl = lf == ALIGN_INF ? ALIGN_INF : lf + c;
            if (vl < best) { best = vl; code = 2u; }
            if (d == 0) { best = 2u * c; code = 3u; }                // the start cell
            ring0[slot] = best;
            dirs[(long)i * W + k] = (unsigned char)code;
        }
        __syncthreads();
        unsigned* t = ring2; ring2 = ring1; ring1 = ring0; ring0 = t;
    }
    // ring1 now holds the last diagonal: the corner cell, if the band holds it
    const int lo_last = align_clampi(lo[N - 1], 0, M - 1);
    const int k_last = M - 1 - lo_last;
    const unsigned total = (k_last >= 0 && k_last < W && imax == N - 1) ? ring1[(N - 1) % L] : ALIGN_INF;
    if (total == ALIGN_INF) {                                        // the band does not connect the corners: no path
        for (int i = tid; i < 2 * (N + M); i += bs) row_lo[i] = -1;
        if (tid == 0) { head[0] = (int)ALIGN_INF; head[1] = 0; head[2] = 0; head[3] = 0; }
        return;
    }
    __threadfence_block();
    if (tid != 0) return;
    // one lane walks back: a row's / column's highest index is seen first, its lowest last
    int i = N - 1, j = M - 1, len = 0, li = lo_last;
    row_hi[i] = j; col_hi[j] = i;
    bool ok = true;
    for (;;) {
        row_lo[i] = j; col_lo[j] = i;
        ++len;
        if (i == 0 && j == 0) break;
        const int k = j - li;
        if (k < 0 || k >= W || len >= N + M) { ok = false; break; }  // (a reachable corner has a path inside the band)
        const unsigned code = dirs[(long)i * W + k];
        if (code > 2u || (code != 2u && i == 0) || (code != 1u && j == 0)) { ok = false; break; }
        if (code != 2u) { --i; li = align_clampi(lo[i], 0, M - 1); }
        if (code != 1u) --j;
        if (code != 2u) row_hi[i] = j;                               // a new row: this is its highest column
        if (code != 1u) col_hi[j] = i;
    }
    head[0] = (int)(ok ? total : ALIGN_INF); head[1] = ok ? len : 0; head[2] = ok ? 0 : -2; head[3] = 0;
}

static int align_check_common(const char* name, const void* desc, int P, int max_w) {
    RV_CHECK_ARG(desc != nullptr, "%s: null descriptor table", name);
    RV_CHECK_ARG(P >= 1 && P <= 65535, "%s: %d pairs outside [1, 65535]", name, P);
    RV_CHECK_ARG(max_w >= 1, "%s: max_w %d must be positive", name, max_w);
    if (max_w > ALIGN_MAX_W) {
        rv_set_error("%s: a band of %d columns; at most %d (three diagonals of it must fit the LDS of a workgroup)", name, max_w, ALIGN_MAX_W);
        return RV_EUNSUPPORTED;
    }
    return RV_OK;
}

extern "C" {

int rv_align_cost(const long* desc, int P, int D, int max_n, int max_w, const float* feats, long n_feats, const int* lo, long n_lo,
                  unsigned short* cost, long n_cost, void* stream) {
    const int rc = align_check_common("rv_align_cost", desc, P, max_w);
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(feats && lo && cost, "rv_align_cost: null pointer");
    RV_CHECK_ARG(D >= 1 && D <= ALIGN_MAX_D, "rv_align_cost: D %d outside [1, %d]", D, ALIGN_MAX_D);
    RV_CHECK_ARG(max_n >= 1 && n_feats >= 0 && n_lo >= 0 && n_cost >= 0, "rv_align_cost: max_n %d or a negative buffer length", max_n);
    if (max_n >= ALIGN_MAX_NM) {
        rv_set_error("rv_align_cost: %d rows; N + M of a pair is at most 2^18", max_n);
        return RV_EUNSUPPORTED;
    }
    CostArgs g;
    g.desc = desc; g.feats = feats; g.n_feats = n_feats; g.lo = lo; g.n_lo = n_lo; g.cost = cost; g.n_cost = n_cost;
    g.D = D; g.max_n = max_n; g.max_w = max_w;
    // enough workgroups along the band for a row tile whose lo climbs by one a row; a steeper tile loops
    const unsigned gy = (unsigned)cdiv(max_w + 31, 128);
    hipLaunchKernelGGL(align_cost_k, dim3((unsigned)cdiv(max_n, 32), gy, (unsigned)P), dim3(256), 0, (hipStream_t)stream, g);
    RV_LAUNCH_CHECK("rv_align_cost");
    return RV_OK;
}

int rv_align_dtw(const long* desc, int P, int max_nm, int max_w, const int* lo, long n_lo, const unsigned short* cost, long n_cost,
                 unsigned char* dirs, long n_dirs, int* out, long n_out, void* stream) {
    const int rc = align_check_common("rv_align_dtw", desc, P, max_w);
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(lo && cost && dirs && out, "rv_align_dtw: null pointer");
    RV_CHECK_ARG(max_nm >= 2 && n_lo >= 0 && n_cost >= 0 && n_dirs >= 0 && n_out >= 0, "rv_align_dtw: max_nm %d or a negative buffer length", max_nm);
    if (max_nm > ALIGN_MAX_NM) {
        rv_set_error("rv_align_dtw: N + M = %d; at most 2^18 (the sums of twelve-bit costs must stay below 2^30)", max_nm);
        return RV_EUNSUPPORTED;
    }
    DtwArgs g;
    g.desc = desc; g.lo = lo; g.n_lo = n_lo; g.cost = cost; g.n_cost = n_cost; g.dirs = dirs; g.n_dirs = n_dirs; g.out = out; g.n_out = n_out;
    g.max_w = max_w; g.max_nm = max_nm; g.L = max_w + 1;
    int bs = 64;
    while (bs < max_w && bs < 1024) bs *= 2;
    const int lds = 3 * g.L * (int)sizeof(unsigned);                 // at most 98 316 bytes
    static int granted = 0;
    if (lds > 64 * 1024 && !granted) {
        if (hipFuncSetAttribute((const void*)align_dtw_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                3 * (ALIGN_MAX_W + 1) * (int)sizeof(unsigned)) != hipSuccess) {
            (void)hipGetLastError();
            rv_set_error("rv_align_dtw: the device refused %d bytes of LDS per workgroup", lds);
            return RV_EUNSUPPORTED;
        }
        granted = 1;
    }
    hipLaunchKernelGGL(align_dtw_k, dim3((unsigned)P), dim3(bs), (size_t)lds, (hipStream_t)stream, g);
    RV_LAUNCH_CHECK("rv_align_dtw");
    return RV_OK;
}

}  // extern "C"
