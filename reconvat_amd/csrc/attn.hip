// Fused 31-frame local multi-head attention (reference MutliHeadAttention1D.forward,
// model/UNet_onset.py:56-91) for gfx950 -- no [B, L, F, 31] unfold is ever materialised.
//
//   energy[b,t,g,w] = sum_f q[b,t,g,f] * (k[b,t+w-15,g,f] + rel[g*dh+f, w])   (k = 0 outside [0,L): the
//                     reference zero-pads x and W_k has no bias, so padded slots score q.rel -- unmasked)
//   att = softmax_w(energy)          (no 1/sqrt(d) scaling)
//   out[b,t,g,f]    = sum_w att[b,t,g,w] * v[b,t+w-15,g,f]
//
// q, k, v (and dq, dk, dv): rows of G*dh floats with an explicit row stride `ld` (they may be column slices of one
// fused [B*L, 3F] projection buffer); out, dout: [B, L, F] contiguous; relT: [31, F] (the parameter [F, 31]
// transposed -- the host packs it once per optimiser step); att, de: [B, L, G, 31].
//
// Two forms of every kernel, chosen per head shape by attn_form() (RV_ATTN_TILE=16 / 32 forces one; read when the library is loaded):
//   the 32-frame form (attn_fwd32_k, attn_bwd_q32_k, attn_bwd_kv32_k; geometry and staging further down): one workgroup = (batch b,
//   32-frame tile, head g), a 62-row window padded to 64, rows staged through buffer resources (out-of-range rows and pad columns arrive
//   as zeros with no per-row test), each q/k/v row read 62/32 = 1.9 times;
//   the 16-frame form (attn_fwd_k, attn_bwd_q_k, attn_bwd_kv_k, described next): the A/B baseline, and the form for views beyond the
//   buffer-resource offset range.  Both produce the same bits (tests/test_attn_tiles_gpu.py).
//
// 16-frame form: one workgroup (5 waves) = (batch b, 16-frame tile, head g).  Both contractions run on v_mfma_f32_16x16x4_f32:
//   scores  S[16 x 80] = X[16 x dh] . Y^T, Y = [ 46-row key window (padded to 48) ; rel^T (31 rows padded to 32) ]:
//           one 16x16 tile per wave, operands read from LDS with ds_read_b128 (a lane's 4 floats feed 4 MFMAs);
//           energy[t][w] = S[t][t+w] + S[t][48+w]
//   apply   O[16 x dh] = A[16 x K] . Y[K x dh] with A the BANDED attention matrix A[t][t+w] = att[t][w] (K = 48),
//           for dq A = [ band(de) | de ] against [ key window ; rel^T ] (K = 80); output tiles round-robin over waves
// The head dimension is padded to a multiple of 16 in LDS (229 -> 240, zero filled).  ~0.5 GFLOP per forward, so the
// kernels are bound by staging the windows (each row is read 46/16 times, from L2).
#include "conv_shared.h"   // rv_make_rsrc / rv_buf_lds16 (the 32-frame form stages through buffer resources)
#include <stdlib.h>
#include <mutex>

// Timing ablations of attn_fwd_k (tools/attn_ablate.sh; wrong results by design; 0 in every product build):
//   1 no staging (q tile, key / value windows, rel^T) | 2 no score MFMAs | 4 no softmax | 8 no banded apply | 16 return at entry
#ifndef RV_ATTN_ABL
#define RV_ATTN_ABL 0
#endif
#define AT_W 31
#define AT_P 15
#define AT_TT 16
#define AT_WIN (AT_TT + 2 * AT_P)   // 46 rows
#define AT_WINP 48                  // ... padded to three MFMA tiles
#define AT_NW 5                     // waves per workgroup (5 score tiles)
#define AT_NTHR (AT_NW * 64)
#define AT_SLD 80                   // raw score row: 48 window columns + 32 rel columns
#define AT_A2LD 52                  // banded matrix row (48 + pad, 16-byte multiple)
#define AT_A3LD 84                  // [band | dense] row (80 + pad)
#define AT_MAXT 4                   // output tiles per wave (dh <= 256)

struct AttnArgs {
    const float* q; const float* k; const float* v; long ld;      // ld: row stride of q, k, v
    const float* rel;
    float* out; float* att;
    const float* dout; const float* de_in;
    float* dq; float* dk; float* dv; long dld;                    // dld: row stride of dq, dk, dv
    float* de;
    int B, L, G, dh, dhp;
    int v4, dv4;                     // 16-byte DMA legal for q/k/v rows / for dout and rel^T rows (stride F)
    int seq_kv;                      // attn_bwd_kv_k: one window buffer used twice (see the kernel)
    int rel_regs;                    // attn_fwd_k / attn_bwd_q_k (wide heads): rel^T fragments straight from global memory into registers
                                     // instead of a 32-row LDS block, so that two workgroups fit a CU
    // 32-frame form only: byte ranges of the buffer-resource views the windows are staged through (one (batch, head) column view each)
    unsigned qkv_bytes, do_bytes, rel_bytes, co_bytes;   // q/k/v rows | dout rows | rel^T rows | att / de rows
    int rel_first;                   // attn_bwd_q32_k: the rel^T terms of dq come before the window terms (the order the 16-frame form uses
                                     // for this head shape: it follows ITS rel_regs choice, so both forms round alike)
};

// dst[r][f] (r < ntotal, f < dhp) = src[(row0 + r) * ld + col0 + f] for r < nvalid, 0 <= row0 + r < L, f < dh; else 0.
// Rows travel by LDS-DMA (16 bytes per lane when `v4`: rows 16-byte aligned, else 4): all of a wave's rows are in
// flight at once and nothing passes through VGPRs; the caller waits (stage_wait) before the barrier.
// Rows outside [0, L) (the zero padding of the key / value windows) and the tail rows r >= nvalid are fetched from a buffer of zeros in
// global memory instead of being zero-filled by stores: per row the code is one scalar range test, one select of the source pointer and the
// DMA instructions -- no exec-mask branch around a store loop (the same scheme as the conv kernels' rv_zero_piece, round 4).
__device__ __attribute__((aligned(16))) const float rv_attn_zero[256] = {0.f};

__device__ __forceinline__ int stage_rows(float* dst, int ldk, const float* src, long ld, int col0, int dh, int dhp,
                                          int row0, int nvalid, int ntotal, int L, bool v4) {
    int issued = 0;                                                  // DMA instructions of this wave (wave-uniform)
    // Lean on purpose: the kernels are bound by the instructions spent here, not by bytes.  Everything per lane is
    // hoisted (byte offset inside a row, lane mask); per row there is a pointer bump, a range test and the DMA.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // v4: the whole quads of a row travel 16 bytes per lane -- the source needs 4-byte alignment only (tools/probes/glds16_unaligned.hip), so this
    // also serves dh = 229 (57 quads + one 4-byte tail instruction instead of four 4-byte instructions per row); else 4 bytes per lane
    const int per = v4 ? 256 : 64;                                   // floats one DMA instruction moves
    const int nfull = v4 ? (dh & ~3) : dh;                           // floats covered by the main instructions
    const int ninst = (nfull + per - 1) / per;
    const int rem = dh - nfull;                                      // v4: 0..3 floats left for one 4-byte instruction
    const int lf = v4 ? lane * 4 : lane;                             // this lane's first float inside an instruction
    const float* s = src + ((long)(row0 + wave) * ld + col0) + lf;   // only dereferenced for rows inside [0, L)
    const float* z = rv_attn_zero + lf;                              // (one instruction's worth of zeros: every k reads the same piece)
    float* drow = dst + wave * ldk;
    const long sstep = (long)AT_NW * ld;
    const int dstep = AT_NW * ldk;
    const int npad = dhp - dh;
    for (int r = wave; r < ntotal; r += AT_NW, s += sstep, drow += dstep) {
        const int t = row0 + r;
        const bool real = r < nvalid && t >= 0 && t < L;
        if (v4) {
            for (int k = 0; k < ninst; ++k)
                if (k * 256 + lf < nfull) glds16(real ? s + k * 256 : z, drow + k * 256);
            if (rem) {
                if (lane < rem) glds4(real ? s - lf + nfull + lane : rv_attn_zero + lane, drow + nfull);
                ++issued;
            }
        } else {
            for (int k = 0; k < ninst; ++k)
                if (k * 64 + lf < dh) glds4(real ? s + k * 64 : z, drow + k * 64);
        }
        issued += ninst;
        if (lane < npad) drow[dh + lane] = 0.f;                      // npad < 16
    }
    return issued;
}
__device__ __forceinline__ void stage_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// one 16x16 score tile: S[t][y] = sum_f X[t][f] * Y[y][f]; the lane ends up with S[4*g4 + r][i], r = 0..3
__device__ __forceinline__ f32x4 score_tile(const float* X, const float* Y, int ldk, int nchunk, int i, int g4) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* xp = X + i * ldk + 4 * g4;
    const float* yp = Y + i * ldk + 4 * g4;
    for (int c = 0; c < nchunk; ++c) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(xp + 16 * c);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(yp + 16 * c);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], b4[r], acc, 0, 0, 0);
    }
    return acc;
}

// the same with the Y operand in registers: yb[c] = Y[i][16 c + 4 g4 .. + 3]
__device__ __forceinline__ f32x4 score_tile_regs(const float* X, const f32x4 (&yb)[16], int ldk, int nchunk, int i, int g4) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* xp = X + i * ldk + 4 * g4;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < nchunk) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(xp + 16 * c);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], yb[c][r], acc, 0, 0, 0);
        }
    }
    return acc;
}

// O[t][f] = sum_k A[t][k] * Y[k][f] over NCH chunks of 16 k; wave `wave` owns the output tiles wave, wave+5, ...
// Rows t0 + t of dst (row stride dld, first column col0) receive the result for f < dh.
// rel^T rows as the B operand of apply_tiles, from global memory: yk[q][c][r] = relT[16 c + 4 g4 + r][col0 + 16 nt + i] (0 past row 30 / column dh)
template <int MAXT> struct RelFragT { f32x4 y[MAXT][2]; };
typedef RelFragT<AT_MAXT> RelFrag;
template <int NW, int MAXT>
__device__ __forceinline__ void rel_frag_load(RelFragT<MAXT>& rf, const float* relT, int F, int col0, int dh, int ntiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        const int f = 16 * (wave + NW * q) + i;
        const bool fok = wave + NW * q < ntiles && f < dh;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = 16 * c + 4 * g4 + r;
                rf.y[q][c][r] = (fok && w < AT_W) ? relT[(long)w * F + col0 + f] : 0.f;
            }
    }
}

// NCH chunks of 16 k from LDS; with `rf` two more chunks (k = 16 NCH .. 16 NCH + 31 of A) whose Y rows are rel^T fragments in registers
template <int NCH>
__device__ __forceinline__ void apply_tiles(const float* A, int lda, const float* Y, int ldk, int ntiles, float* dst,
                                            long dld, int col0, int dh, int nrows_valid, const RelFrag* rf = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    f32x4 acc[AT_MAXT];
#pragma unroll
    for (int q = 0; q < AT_MAXT; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (rf) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(A + i * lda + 16 * (NCH + c) + 4 * g4);
#pragma unroll
            for (int q = 0; q < AT_MAXT; ++q) {
                if (wave + AT_NW * q < ntiles) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], rf->y[q][c][r], acc[q], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(A + i * lda + 16 * c + 4 * g4);
        const float* yk = Y + (16 * c + 4 * g4) * ldk + i;
#pragma unroll
        for (int q = 0; q < AT_MAXT; ++q) {
            const int nt = wave + AT_NW * q;
            if (nt < ntiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], yk[r * ldk + 16 * nt], acc[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < AT_MAXT; ++q) {
        const int nt = wave + AT_NW * q;
        const int f = 16 * nt + i;
        if (nt >= ntiles || f >= dh) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 4 * g4 + r;
            if (t < nrows_valid) dst[(long)t * dld + col0 + f] = acc[q][r];
        }
    }
}

__device__ __forceinline__ float grp16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float grp16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(AT_NTHR) void attn_fwd_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    float* Qs = smem;                           // [16][ldk]
    float* Kx = Qs + AT_TT * ldk;               // [80][ldk]  key window | rel^T ; value window over rows 0..47 later  ([48][ldk] with rel_regs)
    float* Sr = Kx + (a.rel_regs ? AT_WINP : 80) * ldk;   // [16][80]
    float* A2 = Sr + AT_TT * AT_SLD;            // [16][52]
    const int ntile = (a.L + AT_TT - 1) / AT_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);     // an XCD (one L2) owns a run of neighbouring tiles: window overlap hits
    const int b = bx / ntile, t0 = (bx - b * ntile) * AT_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    const long boff = (long)b * a.L * a.ld;
    if (RV_ATTN_ABL & 16) return;
    if (!(RV_ATTN_ABL & 1)) {
    stage_rows(Qs, ldk, a.q + boff, a.ld, g * dh, dh, dhp, t0, AT_TT, AT_TT, a.L, a.v4);
    stage_rows(Kx, ldk, a.k + boff, a.ld, g * dh, dh, dhp, t0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
    }
    f32x4 yb[16];                               // rel_regs: waves 3, 4 hold their rel^T score operand (row 16 (wave - 3) + i) in registers
    if (a.rel_regs) {
        if (wave >= 3) {
            const int w = 16 * (wave - 3) + i;
            const float* rp = a.rel + (long)min(w, AT_W - 1) * F + g * dh + 4 * g4;
#pragma unroll
            for (int c = 0; c < 16; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) yb[c][r] = (c < nchunk && w < AT_W && 16 * c + 4 * g4 + r < dh) ? rp[16 * c + r] : 0.f;
        }
    } else if (!(RV_ATTN_ABL & 1)) {
        stage_rows(Kx + AT_WINP * ldk, ldk, a.rel, F, g * dh, dh, dhp, 0, AT_W, 32, AT_W, a.dv4);
    }
    for (int idx = tid; idx < AT_TT * AT_A2LD; idx += AT_NTHR) A2[idx] = 0.f;
    stage_wait();
    __syncthreads();
    if (!(RV_ATTN_ABL & 2)) {
        const f32x4 s = (a.rel_regs && wave >= 3) ? score_tile_regs(Qs, yb, ldk, nchunk, i, g4)
                                                  : score_tile(Qs, Kx + 16 * wave * ldk, ldk, nchunk, i, g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) Sr[(4 * g4 + r) * AT_SLD + 16 * wave + i] = s[r];
    }
    __syncthreads();                            // scores complete, key window dead
    if (!(RV_ATTN_ABL & 1)) stage_rows(Kx, ldk, a.v + boff, a.ld, g * dh, dh, dhp, t0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
    if (tid < 256 && !(RV_ATTN_ABL & 4)) {      // softmax: 16 lanes per frame, two window slots per lane
        const int t = tid >> 4, l = tid & 15;
        const float* sr = Sr + t * AT_SLD;
        const float e0 = sr[t + l] + sr[AT_WINP + l];
        const float e1 = l < 15 ? sr[t + l + 16] + sr[AT_WINP + l + 16] : -INFINITY;
        const float m = grp16_max(fmaxf(e0, e1));
        float p0 = expf(e0 - m), p1 = l < 15 ? expf(e1 - m) : 0.f;
        const float inv = 1.f / grp16_sum(p0 + p1);
        p0 *= inv; p1 *= inv;
        A2[t * AT_A2LD + t + l] = p0;
        if (l < 15) A2[t * AT_A2LD + t + l + 16] = p1;
        if (a.att && t0 + t < a.L) {
            float* ar = a.att + (((long)b * a.L + t0 + t) * a.G + g) * AT_W;
            ar[l] = p0;
            if (l < 15) ar[l + 16] = p1;
        }
    }
    stage_wait();
    __syncthreads();
    if (!(RV_ATTN_ABL & 8)) apply_tiles<3>(A2, AT_A2LD, Kx, ldk, nchunk, a.out + ((long)b * a.L + t0) * F, F, g * dh, dh, a.L - t0);
}

// backward, query side: de (softmax backward) and dq for a 16-frame tile
__global__ __launch_bounds__(AT_NTHR) void attn_bwd_q_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    float* Ds = smem;                           // [16][ldk]  dout tile
    float* Kx = Ds + AT_TT * ldk;               // [80][ldk]  value window, then key window | rel^T   ([48][ldk] with rel_regs)
    float* Sr = Kx + (a.rel_regs ? AT_WINP : 80) * ldk;   // [16][80]   dout . v^T (48 columns used)
    float* A3 = Sr + AT_TT * AT_SLD;            // [16][84]   [ band(de) | de ]
    const int ntile = (a.L + AT_TT - 1) / AT_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);     // an XCD (one L2) owns a run of neighbouring tiles: window overlap hits
    const int b = bx / ntile, t0 = (bx - b * ntile) * AT_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    const long boff = (long)b * a.L * a.ld;
    stage_rows(Ds, ldk, a.dout + (long)b * a.L * F, F, g * dh, dh, dhp, t0, AT_TT, AT_TT, a.L, a.dv4);
    stage_rows(Kx, ldk, a.v + boff, a.ld, g * dh, dh, dhp, t0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
    RelFrag rf;
    if (a.rel_regs) rel_frag_load<AT_NW>(rf, a.rel, F, g * dh, dh, nchunk);      // (consumed by the last phase: the loads fly under everything else)
    else stage_rows(Kx + AT_WINP * ldk, ldk, a.rel, F, g * dh, dh, dhp, 0, AT_W, 32, AT_W, a.dv4);
    for (int idx = tid; idx < AT_TT * AT_A3LD; idx += AT_NTHR) A3[idx] = 0.f;
    stage_wait();
    __syncthreads();
    if (wave < 3) {
        const f32x4 s = score_tile(Ds, Kx + 16 * wave * ldk, ldk, nchunk, i, g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) Sr[(4 * g4 + r) * AT_SLD + 16 * wave + i] = s[r];
    }
    __syncthreads();                            // value window dead
    stage_rows(Kx, ldk, a.k + boff, a.ld, g * dh, dh, dhp, t0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
    if (tid < 256) {
        const int t = tid >> 4, l = tid & 15;
        const bool rv = t0 + t < a.L;
        const long arow = (((long)b * a.L + t0 + t) * a.G + g) * AT_W;
        const float p0 = rv ? a.att[arow + l] : 0.f;
        const float p1 = (rv && l < 15) ? a.att[arow + l + 16] : 0.f;
        const float* sr = Sr + t * AT_SLD;
        const float d0 = sr[t + l], d1 = l < 15 ? sr[t + l + 16] : 0.f;
        const float dot = grp16_sum(p0 * d0 + p1 * d1);
        const float e0 = p0 * (d0 - dot), e1 = p1 * (d1 - dot);
        float* ar = A3 + t * AT_A3LD;
        ar[t + l] = e0;
        ar[AT_WINP + l] = e0;
        if (l < 15) { ar[t + l + 16] = e1; ar[AT_WINP + l + 16] = e1; }
        if (rv) {
            a.de[arow + l] = e0;
            if (l < 15) a.de[arow + l + 16] = e1;
        }
    }
    stage_wait();
    __syncthreads();
    if (a.rel_regs) apply_tiles<3>(A3, AT_A3LD, Kx, ldk, nchunk, a.dq + ((long)b * a.L + t0) * a.dld, a.dld, g * dh, dh, a.L - t0, &rf);
    else apply_tiles<5>(A3, AT_A3LD, Kx, ldk, nchunk, a.dq + ((long)b * a.L + t0) * a.dld, a.dld, g * dh, dh, a.L - t0);
}

// backward, key/value side for a 16-frame tile of window rows s:
//   dv[s] = sum_w att[s-w+15][w] * dout[s-w+15],   dk[s] = sum_w de[s-w+15][w] * q[s-w+15]
// i.e. the transposed band A4[s][u] = coef[s0-15+u][s - u + 30] (u = 0..45) against the 46-row window of dout / q.
__global__ __launch_bounds__(AT_NTHR) void attn_bwd_kv_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    // a.seq_kv (wide heads): ONE row-window buffer, used for the dout window (dv) and then for the q window (dk) -- 66 KB
    // instead of 113 KB of LDS at dh = 229, so that TWO workgroups fit a CU and one's DMA wait hides under the other's MFMAs
    // (a 5-wave workgroup alone leaves the CU idle through every staging phase: 82 -> 58 us).  Narrow heads (dh = 128) fit
    // twice either way and keep both windows in flight at once.
    float* Yd = smem;                           // [48][ldk]  dout window (then q window)
    float* Yq = a.seq_kv ? Yd : Yd + AT_WINP * ldk;   // [48][ldk]  q window
    float* Ca = Yq + AT_WINP * ldk;             // [48][32]   att window
    float* Ce = Ca + AT_WINP * 32;              // [48][32]   de window
    float* A4 = Ce + AT_WINP * 32;              // [16][52]   transposed band of att
    float* A5 = A4 + AT_TT * AT_A2LD;           // [16][52]   transposed band of de
    const int ntile = (a.L + AT_TT - 1) / AT_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bx / ntile, s0 = (bx - b * ntile) * AT_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x;
    // everything this tile needs is in flight at once: both row windows and both coefficient windows (a row of the
    // latter is 31 contiguous floats)
    stage_rows(Yd, ldk, a.dout + (long)b * a.L * F, F, g * dh, dh, dhp, s0 - AT_P, AT_WIN, AT_WINP, a.L, a.dv4);
    if (!a.seq_kv) stage_rows(Yq, ldk, a.q + (long)b * a.L * a.ld, a.ld, g * dh, dh, dhp, s0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
    const long cld = (long)a.G * AT_W;
    stage_rows(Ca, 32, a.att + (long)b * a.L * cld, cld, g * AT_W, AT_W, 32, s0 - AT_P, AT_WIN, AT_WINP, a.L, false);
    stage_rows(Ce, 32, a.de_in + (long)b * a.L * cld, cld, g * AT_W, AT_W, 32, s0 - AT_P, AT_WIN, AT_WINP, a.L, false);
    stage_wait();
    __syncthreads();
    for (int idx = tid; idx < AT_TT * AT_A2LD; idx += AT_NTHR) {
        const int sl = idx / AT_A2LD, u = idx - sl * AT_A2LD;
        const int w = sl - u + 2 * AT_P;        // t = s - w + 15  <=>  w = s - t + 15 = sl - u + 30
        const bool in = u < AT_WIN && w >= 0 && w < AT_W;
        A4[idx] = in ? Ca[u * 32 + w] : 0.f;
        A5[idx] = in ? Ce[u * 32 + w] : 0.f;
    }
    __syncthreads();
    const long orow = ((long)b * a.L + s0) * a.dld;
    apply_tiles<3>(A4, AT_A2LD, Yd, ldk, nchunk, a.dv + orow, a.dld, g * dh, dh, a.L - s0);
    if (a.seq_kv) {
        __syncthreads();                        // dout window dead
        stage_rows(Yq, ldk, a.q + (long)b * a.L * a.ld, a.ld, g * dh, dh, dhp, s0 - AT_P, AT_WIN, AT_WINP, a.L, a.v4);
        stage_wait();
        __syncthreads();
    }
    apply_tiles<3>(A5, AT_A2LD, Yq, ldk, nchunk, a.dk + orow, a.dld, g * dh, dh, a.L - s0);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The 32-frame form: one workgroup = (batch b, 32-frame tile, head g); the window is 32 + 30 = 62 rows padded to 64, so a q/k/v row is
// staged 62/32 = 1.9 times instead of 46/16 = 2.9 times and the per-workgroup fixed costs (rel^T, zeroing the banded matrix, barriers,
// launch tail) are paid half as often.  Every number it produces is bit-identical to the 16-frame form's:
//   scores  the two 16-row tiles need window column tiles {0,1,2} and {1,2,3} (the other two hold no band entry) plus two rel^T tiles
//           each: 10 tiles of 16x16, each contracted over the head dimension in the same chunk order as score_tile always did
//   apply   row tile rt multiplies window chunks rt .. rt+2 only -- the chunk in front of / behind its band holds exact zeros and is
//           skipped, not multiplied -- i.e. exactly the three chunks, in the same order, of the 16-frame workgroup at t0 + 16 rt; the
//           two row tiles share the B fragments of chunks 1 and 2
// NW waves (5: two score tiles per wave; 10: one), output column tiles round-robin over the waves as before.
#define AT2_TT 32
#define AT2_WIN (AT2_TT + 2 * AT_P)  // 62 rows
#define AT2_WINP 64                  // ... padded to four MFMA tiles
#define AT2_SLD 96                   // raw score row: 64 window columns + 32 rel columns
#define AT2_A2LD 68                  // banded matrix row (64 + pad)
#define AT2_A3LD 100                 // [band | dense] row (96 + pad)
#define AT2_NSCORE 10                // score tiles of the forward kernel: 6 window tiles, then 4 rel^T tiles

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void rv_buf_lds4(rv_rsrc_t rs, void* lds, unsigned voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 4, voff, 0, 0, 0);
}
#else
__device__ inline void rv_buf_lds4(rv_rsrc_t, void*, unsigned) {}
#endif

// stage_rows through a buffer resource over `bytes` bytes from `base` (the (batch, head) column view: row t at byte t * ld * 4, so
// bytes = ((L - 1) * ld + dh) * 4).  An offset outside [0, bytes) makes the DMA write ZEROS (tools/probes/buffer_lds_oob.hip): rows in
// front of / behind the sequence (negative offsets wrap to >= 0xC0000000), the tail rows r >= nvalid and the pad columns dh .. dhp
// all arrive as zeros with no range test, no source select and no store.  Per lane one offset per slot is hoisted; per row the code is
// one add and the DMA.  The host keeps (L + 64) * ld * 4 below 0x3f000000, so no sum below wraps into the view:
//   kColOut (a pad column) + row bytes stays in [0x41000000, 0xbf000400], kRowOut (a tail row) + column bytes in [0x40000000, 0xc0000000].
// v4: 16 bytes per lane (dhp <= 256: ONE instruction per row; the source needs 4-byte alignment only, tools/probes/glds16_unaligned.hip and
// buffer_lds16_unaligned.hip) plus one 4-byte instruction of four lanes for a row tail of dh % 4 floats and the zeros behind it.
template <int NW>
__device__ __forceinline__ void stage_rows_buf(float* dst, int ldk, const float* base, unsigned bytes, int ld, int dh, int dhp, int row0,
                                               int nvalid, int ntotal, bool v4) {
    const rv_rsrc_t rs = rv_make_rsrc(base, bytes);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned kColOut = 0x80000000u, kRowOut = 0x40000000u;
    float* drow = dst + wave * ldk;
    int rb = (row0 + wave) * ld * 4;                                 // byte offset of this wave's next row (negative in front of the sequence)
    const int rstep = NW * ld * 4, dstep = NW * ldk;
    if (v4) {
        const int nfull = dh & ~3, rem = dh - nfull, zlo = nfull + (rem ? 4 : 0), lf = 4 * lane;
        const bool act = lf < nfull || (lf >= zlo && lf < dhp);      // whole quads of the row | whole quads of padding
        const unsigned vo = lf < nfull ? lf * 4u : kColOut;
        const unsigned vt = lane < rem ? (nfull + lane) * 4u : kColOut;
        for (int r = wave; r < ntotal; r += NW, rb += rstep, drow += dstep) {
            const unsigned ro = r < nvalid ? (unsigned)rb : kRowOut;
            if (act) rv_buf_lds16(rs, drow, vo + ro);
            if (rem && lane < 4) rv_buf_lds4(rs, drow + nfull, vt + ro);
        }
    } else {
        for (int r = wave; r < ntotal; r += NW, rb += rstep, drow += dstep) {
            const unsigned ro = r < nvalid ? (unsigned)rb : kRowOut;
            for (int k = 0; k * 64 < dhp; ++k) {
                const int f = k * 64 + lane;
                if (f < dhp) rv_buf_lds4(rs, drow + k * 64, (f < dh ? f * 4u : kColOut) + ro);
            }
        }
    }
}

// window score tile `id` (0..5) of a 32-frame workgroup: row tile rt against window column tile ct
__device__ __forceinline__ void win_tile32(int id, int& rt, int& ct) { rt = id >= 3; ct = id - 2 * rt; }

// O[32 x dh] = A[32 x 64] . Y[64 x dh] with A banded (see above: row tile rt takes chunks rt .. rt+2); REL: A carries 32 dense columns
// behind the band (column 64 on) that multiply rel^T -- from LDS (Yrel) or, with `rf`, from register fragments -- in front of the window
// terms (rel_first) or behind them.  Wave `wave` owns the output column tiles wave, wave + NW, ...
template <int NW, bool REL>
__device__ __forceinline__ void apply32(const float* A, int lda, const float* Y, int ldk, int ntiles, float* dst, long dld, int col0, int dh,
                                        int nrows_valid, const float* Yrel = nullptr, const RelFragT<(16 + NW - 1) / NW>* rf = nullptr,
                                        bool rel_first = false) {
    constexpr int MAXT = (16 + NW - 1) / NW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    f32x4 acc[2][MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) acc[0][q] = acc[1][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto rel_part = [&]() {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(A + i * lda + AT2_WINP + 16 * c + 4 * g4);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(A + (16 + i) * lda + AT2_WINP + 16 * c + 4 * g4);
#pragma unroll
            for (int q = 0; q < MAXT; ++q) {
                const int nt = wave + NW * q;
                if (nt < ntiles) {
                    f32x4 y;
                    if (rf) y = rf->y[q][c];
                    else {
                        const float* yk = Yrel + (16 * c + 4 * g4) * ldk + 16 * nt + i;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = yk[r * ldk];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], y[r], acc[0][q], 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[1][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], y[r], acc[1][q], 0, 0, 0);
                }
            }
        }
    };
    if (REL && rel_first) rel_part();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f32x4 a0 = (f32x4){0.f, 0.f, 0.f, 0.f}, a1 = a0;
        if (c < 3) a0 = *reinterpret_cast<const f32x4*>(A + i * lda + 16 * c + 4 * g4);
        if (c > 0) a1 = *reinterpret_cast<const f32x4*>(A + (16 + i) * lda + 16 * c + 4 * g4);
        const float* yk = Y + (16 * c + 4 * g4) * ldk + i;
#pragma unroll
        for (int q = 0; q < MAXT; ++q) {
            const int nt = wave + NW * q;
            if (nt < ntiles) {
                f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = yk[r * ldk + 16 * nt];
                if (c < 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], y[r], acc[0][q], 0, 0, 0);
                }
                if (c > 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[1][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], y[r], acc[1][q], 0, 0, 0);
                }
            }
        }
    }
    if (REL && !rel_first) rel_part();
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
        const int nt = wave + NW * q;
        const int f = 16 * nt + i;
        if (nt >= ntiles || f >= dh) continue;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = 16 * rt + 4 * g4 + r;
                if (t < nrows_valid) dst[(long)t * dld + col0 + f] = acc[rt][q][r];
            }
    }
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_fwd32_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(AT2_NSCORE % NW == 0, "the score tiles divide over the waves");
    constexpr int NTHR = NW * 64, TPW = AT2_NSCORE / NW;
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    float* Qs = smem;                           // [32][ldk]
    float* Kx = Qs + AT2_TT * ldk;              // [64][ldk]  key window, value window later
    float* Rx = Kx + AT2_WINP * ldk;            // [32][ldk]  rel^T (absent with rel_regs)
    float* Sr = Rx + (a.rel_regs ? 0 : 32) * ldk;   // [32][96]
    float* A2 = Sr + AT2_TT * AT2_SLD;          // [32][68]
    const int ntile = (a.L + AT2_TT - 1) / AT2_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);     // an XCD (one L2) owns a run of neighbouring tiles: window overlap hits
    const int b = bx / ntile, t0 = (bx - b * ntile) * AT2_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g4 = lane >> 4;
    const long boff = (long)b * a.L * a.ld + g * dh;
    const int id0 = wave * TPW;                 // this wave's score tiles: id0 .. id0 + TPW - 1 (0..5 window tiles, 6..9 rel^T tile (id - 6) >> 1 of row tile (id - 6) & 1)
    if (RV_ATTN_ABL & 16) return;
    if (!(RV_ATTN_ABL & 1)) {
        stage_rows_buf<NW>(Qs, ldk, a.q + boff, a.qkv_bytes, (int)a.ld, dh, dhp, t0, AT2_TT, AT2_TT, a.v4);
        stage_rows_buf<NW>(Kx, ldk, a.k + boff, a.qkv_bytes, (int)a.ld, dh, dhp, t0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
    }
    f32x4 yb[16];                               // rel_regs: the waves of the rel^T tiles hold their score operand (row 16 c + i) in registers
    if (a.rel_regs) {
        if (id0 >= 6) {
            const int w = 16 * ((id0 - 6) >> 1) + i;
            const float* rp = a.rel + (long)min(w, AT_W - 1) * F + g * dh + 4 * g4;
#pragma unroll
            for (int c = 0; c < 16; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) yb[c][r] = (c < nchunk && w < AT_W && 16 * c + 4 * g4 + r < dh) ? rp[16 * c + r] : 0.f;
        }
    } else if (!(RV_ATTN_ABL & 1)) {
        stage_rows_buf<NW>(Rx, ldk, a.rel + g * dh, a.rel_bytes, F, dh, dhp, 0, AT_W, 32, a.dv4);
    }
    for (int idx = tid; idx < AT2_TT * AT2_A2LD; idx += NTHR) A2[idx] = 0.f;
    stage_wait();
    __syncthreads();
    if (!(RV_ATTN_ABL & 2)) {
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int id = id0 + j;
            int rt, col;
            f32x4 s;
            if (id < 6) {
                int ct;
                win_tile32(id, rt, ct);
                s = score_tile(Qs + 16 * rt * ldk, Kx + 16 * ct * ldk, ldk, nchunk, i, g4);
                col = 16 * ct;
            } else {
                rt = (id - 6) & 1;
                const int c = (id - 6) >> 1;
                s = a.rel_regs ? score_tile_regs(Qs + 16 * rt * ldk, yb, ldk, nchunk, i, g4)
                               : score_tile(Qs + 16 * rt * ldk, Rx + 16 * c * ldk, ldk, nchunk, i, g4);
                col = AT2_WINP + 16 * c;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Sr[(16 * rt + 4 * g4 + r) * AT2_SLD + col + i] = s[r];
        }
    }
    __syncthreads();                            // scores complete, key window dead
    if (!(RV_ATTN_ABL & 1)) stage_rows_buf<NW>(Kx, ldk, a.v + boff, a.qkv_bytes, (int)a.ld, dh, dhp, t0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
    if (!(RV_ATTN_ABL & 4)) {                   // softmax: 16 lanes per frame, two window slots per lane (the 16-frame form's arithmetic)
        for (int t = tid >> 4; t < AT2_TT; t += NTHR / 16) {
            const int l = tid & 15;
            const float* sr = Sr + t * AT2_SLD;
            const float e0 = sr[t + l] + sr[AT2_WINP + l];
            const float e1 = l < 15 ? sr[t + l + 16] + sr[AT2_WINP + l + 16] : -INFINITY;
            const float m = grp16_max(fmaxf(e0, e1));
            float p0 = expf(e0 - m), p1 = l < 15 ? expf(e1 - m) : 0.f;
            const float inv = 1.f / grp16_sum(p0 + p1);
            p0 *= inv; p1 *= inv;
            A2[t * AT2_A2LD + t + l] = p0;
            if (l < 15) A2[t * AT2_A2LD + t + l + 16] = p1;
            if (a.att && t0 + t < a.L) {
                float* ar = a.att + (((long)b * a.L + t0 + t) * a.G + g) * AT_W;
                ar[l] = p0;
                if (l < 15) ar[l + 16] = p1;
            }
        }
    }
    stage_wait();
    __syncthreads();
    if (!(RV_ATTN_ABL & 8)) apply32<NW, false>(A2, AT2_A2LD, Kx, ldk, nchunk, a.out + ((long)b * a.L + t0) * F, F, g * dh, dh, a.L - t0);
}

// backward, query side: de (softmax backward) and dq for a 32-frame tile
template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_bwd_q32_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTHR = NW * 64, TPW = AT2_NSCORE / NW, MAXT = (16 + NW - 1) / NW;
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    float* Ds = smem;                           // [32][ldk]  dout tile
    float* Kx = Ds + AT2_TT * ldk;              // [64][ldk]  value window, then key window
    float* Rx = Kx + AT2_WINP * ldk;            // [32][ldk]  rel^T (absent with rel_regs)
    float* Sr = Rx + (a.rel_regs ? 0 : 32) * ldk;   // [32][96]   dout . v^T (64 columns used)
    float* A3 = Sr + AT2_TT * AT2_SLD;          // [32][100]  [ band(de) | de ]
    const int ntile = (a.L + AT2_TT - 1) / AT2_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bx / ntile, t0 = (bx - b * ntile) * AT2_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g4 = lane >> 4;
    const long boff = (long)b * a.L * a.ld + g * dh;
    stage_rows_buf<NW>(Ds, ldk, a.dout + (long)b * a.L * F + g * dh, a.do_bytes, F, dh, dhp, t0, AT2_TT, AT2_TT, a.dv4);
    stage_rows_buf<NW>(Kx, ldk, a.v + boff, a.qkv_bytes, (int)a.ld, dh, dhp, t0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
    RelFragT<MAXT> rf;
    if (a.rel_regs) rel_frag_load<NW>(rf, a.rel, F, g * dh, dh, nchunk);      // (consumed by the last phase: the loads fly under everything else)
    else stage_rows_buf<NW>(Rx, ldk, a.rel + g * dh, a.rel_bytes, F, dh, dhp, 0, AT_W, 32, a.dv4);
    for (int idx = tid; idx < AT2_TT * AT2_A3LD; idx += NTHR) A3[idx] = 0.f;
    stage_wait();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int id = wave * TPW + j;
        if (id < 6) {
            int rt, ct;
            win_tile32(id, rt, ct);
            const f32x4 s = score_tile(Ds + 16 * rt * ldk, Kx + 16 * ct * ldk, ldk, nchunk, i, g4);
#pragma unroll
            for (int r = 0; r < 4; ++r) Sr[(16 * rt + 4 * g4 + r) * AT2_SLD + 16 * ct + i] = s[r];
        }
    }
    __syncthreads();                            // value window dead
    stage_rows_buf<NW>(Kx, ldk, a.k + boff, a.qkv_bytes, (int)a.ld, dh, dhp, t0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
    for (int t = tid >> 4; t < AT2_TT; t += NTHR / 16) {
        const int l = tid & 15;
        const bool rv = t0 + t < a.L;
        const long arow = (((long)b * a.L + t0 + t) * a.G + g) * AT_W;
        const float p0 = rv ? a.att[arow + l] : 0.f;
        const float p1 = (rv && l < 15) ? a.att[arow + l + 16] : 0.f;
        const float* sr = Sr + t * AT2_SLD;
        const float d0 = sr[t + l], d1 = l < 15 ? sr[t + l + 16] : 0.f;
        const float dot = grp16_sum(p0 * d0 + p1 * d1);
        const float e0 = p0 * (d0 - dot), e1 = p1 * (d1 - dot);
        float* ar = A3 + t * AT2_A3LD;
        ar[t + l] = e0;
        ar[AT2_WINP + l] = e0;
        if (l < 15) { ar[t + l + 16] = e1; ar[AT2_WINP + l + 16] = e1; }
        if (rv) {
            a.de[arow + l] = e0;
            if (l < 15) a.de[arow + l + 16] = e1;
        }
    }
    stage_wait();
    __syncthreads();
    float* dq = a.dq + ((long)b * a.L + t0) * a.dld;
    if (a.rel_regs) apply32<NW, true>(A3, AT2_A3LD, Kx, ldk, nchunk, dq, a.dld, g * dh, dh, a.L - t0, nullptr, &rf, a.rel_first != 0);
    else apply32<NW, true>(A3, AT2_A3LD, Kx, ldk, nchunk, dq, a.dld, g * dh, dh, a.L - t0, Rx, nullptr, a.rel_first != 0);
}

// backward, key/value side for a 32-frame tile of window rows s: the transposed band A4[s][u] = coef[s0-15+u][s - u + 30] (u = 0..61)
// against the 62-row window of dout / q -- the same band geometry as the forward apply (row tile rt holds entries in chunks rt .. rt+2)
template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_bwd_kv32_k(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTHR = NW * 64;
    const int dh = a.dh, dhp = a.dhp, ldk = dhp + 4, nchunk = dhp >> 4, F = a.G * dh;
    float* Yd = smem;                           // [64][ldk]  dout window (then q window with seq_kv)
    float* Yq = a.seq_kv ? Yd : Yd + AT2_WINP * ldk;  // [64][ldk]  q window
    float* Ca = Yq + AT2_WINP * ldk;            // [64][32]   att window
    float* Ce = Ca + AT2_WINP * 32;             // [64][32]   de window
    float* A4 = Ce + AT2_WINP * 32;             // [32][68]   transposed band of att
    float* A5 = A4 + AT2_TT * AT2_A2LD;         // [32][68]   transposed band of de
    const int ntile = (a.L + AT2_TT - 1) / AT2_TT;
    const int bx = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bx / ntile, s0 = (bx - b * ntile) * AT2_TT;
    const int g = blockIdx.y;
    const int tid = threadIdx.x;
    const float* qb = a.q + (long)b * a.L * a.ld + g * dh;
    stage_rows_buf<NW>(Yd, ldk, a.dout + (long)b * a.L * F + g * dh, a.do_bytes, F, dh, dhp, s0 - AT_P, AT2_WIN, AT2_WINP, a.dv4);
    if (!a.seq_kv) stage_rows_buf<NW>(Yq, ldk, qb, a.qkv_bytes, (int)a.ld, dh, dhp, s0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
    const int cld = a.G * AT_W;
    const long coff = (long)b * a.L * cld + g * AT_W;
    stage_rows_buf<NW>(Ca, 32, a.att + coff, a.co_bytes, cld, AT_W, 32, s0 - AT_P, AT2_WIN, AT2_WINP, false);
    stage_rows_buf<NW>(Ce, 32, a.de_in + coff, a.co_bytes, cld, AT_W, 32, s0 - AT_P, AT2_WIN, AT2_WINP, false);
    stage_wait();
    __syncthreads();
    for (int idx = tid; idx < AT2_TT * AT2_A2LD; idx += NTHR) {
        const int sl = idx / AT2_A2LD, u = idx - sl * AT2_A2LD;
        const int w = sl - u + 2 * AT_P;        // t = s - w + 15  <=>  w = s - t + 15 = sl - u + 30
        const bool in = u < AT2_WIN && w >= 0 && w < AT_W;
        A4[idx] = in ? Ca[u * 32 + w] : 0.f;
        A5[idx] = in ? Ce[u * 32 + w] : 0.f;
    }
    __syncthreads();
    const long orow = ((long)b * a.L + s0) * a.dld;
    apply32<NW, false>(A4, AT2_A2LD, Yd, ldk, nchunk, a.dv + orow, a.dld, g * dh, dh, a.L - s0);
    if (a.seq_kv) {
        __syncthreads();                        // dout window dead
        stage_rows_buf<NW>(Yq, ldk, qb, a.qkv_bytes, (int)a.ld, dh, dhp, s0 - AT_P, AT2_WIN, AT2_WINP, a.v4);
        stage_wait();
        __syncthreads();
    }
    apply32<NW, false>(A5, AT2_A2LD, Yq, ldk, nchunk, a.dk + orow, a.dld, g * dh, dh, a.L - s0);
}

static int attn_setup(AttnArgs& a, int dh, const char* who) {
    RV_CHECK_ARG(dh >= 1 && dh <= 256, "%s: head dim %d unsupported", who, dh);
    a.dh = dh;
    a.dhp = (dh + 15) & ~15;
    static std::once_flag attr_once;              // (forward and backward launches come from different threads)
    std::call_once(attr_once, [] {
        (void)hipFuncSetAttribute((const void*)attn_fwd_k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_q_k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_kv_k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_fwd32_k<5>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_q32_k<5>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_kv32_k<5>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_fwd32_k<10>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_q32_k<10>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipFuncSetAttribute((const void*)attn_bwd_kv32_k<10>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    });
    return RV_OK;
}

// Frames per workgroup (16 or 32) and waves of the 32-frame form (5 or 10), chosen per head shape by what won in the step
// (profiles/EXPERIMENTS.md, "attention tiles").  RV_ATTN_TILE=16 / 32 forces one form (16 is the A/B baseline and what
// tests/test_attn_tiles_gpu.py compares against), RV_ATTN_WAVES=5 / 10 the wave count; RV_ATTN_TILE_WIDE / RV_ATTN_WAVES_WIDE do the
// same for the wide heads only (dh > 128) and win over the former there.  All are read once, when the library is loaded.
// The 32-frame form addresses its views with 30-bit offsets (stage_rows_buf): longer views take the 16-frame form.
static int attn_env(const char* name) { return getenv(name) ? atoi(getenv(name)) : 0; }
static const int g_attn_tile_env = attn_env("RV_ATTN_TILE"), g_attn_tile_wide_env = attn_env("RV_ATTN_TILE_WIDE");
static const int g_attn_waves_env = attn_env("RV_ATTN_WAVES"), g_attn_waves_wide_env = attn_env("RV_ATTN_WAVES_WIDE");
struct AttnForm { int tile, waves; };
static AttnForm attn_form(int dh, int L, long max_ld) {
    const bool wide = dh > 128;
    const int tile = wide && g_attn_tile_wide_env ? g_attn_tile_wide_env : g_attn_tile_env;
    const int waves = wide && g_attn_waves_wide_env ? g_attn_waves_wide_env : g_attn_waves_env;
    AttnForm f;
    f.tile = tile == 16 || tile == 32 ? tile : 32;
    f.waves = waves == 5 || waves == 10 ? waves : 5;
    if (((long)L + 64) * max_ld * 4 >= 0x3f000000L) f.tile = 16;
    return f;
}
static unsigned attn_view_bytes(int L, long ld, int dh) { return (unsigned)((((long)L - 1) * ld + dh) * 4); }
// LDS of a workgroup above which only ONE fits a CU: beyond it the rel^T block moves to registers and the kv pass stages its two windows
// one after the other (two workgroups per CU again).  Far below the 128 KiB the kernels may be given (attn_setup), so nothing larger is launched.
static const size_t kAttnOccLds = 78 * 1024;

extern "C" {

int rv_local_attn_fwd(const float* q, const float* k, const float* v, long ld, const float* relT, float* out, float* att, int B,
                      int L, int G, int dh, void* stream) {
    AttnArgs a = {};
    const int rc = attn_setup(a, dh, "rv_local_attn_fwd");
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(ld >= (long)G * dh, "rv_local_attn_fwd: row stride %ld < G*dh", ld);
    a.q = q; a.k = k; a.v = v; a.ld = ld; a.rel = relT; a.out = out; a.att = att; a.B = B; a.L = L; a.G = G;
    a.v4 = a.dv4 = 1;      // 16-byte DMA lanes are legal for every fp32 row (the source needs 4-byte alignment only; a row tail of dh % 4 floats goes 4 bytes per lane)
    const int ntile = (L + AT_TT - 1) / AT_TT, ldk = a.dhp + 4;
    size_t lds = ((size_t)(AT_TT + 80) * ldk + AT_TT * AT_SLD + AT_TT * AT_A2LD) * sizeof(float);
    a.rel_regs = lds > kAttnOccLds;       // the rel^T block would leave room for only one workgroup per CU
    const AttnForm form = attn_form(dh, L, ld > (long)G * dh ? ld : (long)G * dh);
    if (form.tile == 32) {
        size_t lds32 = ((size_t)(AT2_TT + AT2_WINP + 32) * ldk + AT2_TT * AT2_SLD + AT2_TT * AT2_A2LD) * sizeof(float);
        a.rel_regs = lds32 > kAttnOccLds;
        if (a.rel_regs) lds32 -= (size_t)32 * ldk * sizeof(float);
        a.qkv_bytes = attn_view_bytes(L, ld, dh);
        a.rel_bytes = attn_view_bytes(AT_W, (long)G * dh, dh);
        const dim3 grid(B * ((L + AT2_TT - 1) / AT2_TT), G);
        if (form.waves == 10) hipLaunchKernelGGL((attn_fwd32_k<10>), grid, dim3(640), lds32, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((attn_fwd32_k<5>), grid, dim3(320), lds32, (hipStream_t)stream, a);
        RV_LAUNCH_CHECK("rv_local_attn_fwd");
        return RV_OK;
    }
    if (a.rel_regs) lds -= (size_t)32 * ldk * sizeof(float);
    hipLaunchKernelGGL(attn_fwd_k, dim3(B * ntile, G), dim3(AT_NTHR), lds, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK("rv_local_attn_fwd");
    return RV_OK;
}

// Inputs: dout and the forward's q, k, v, att.  Outputs: dq, dk, dv (row stride dld) and de [B,L,G,31] (the energy
// gradient; drel = sum_{b,t} de (x) q is a plain GEMM the host issues through rv_gemm).
int rv_local_attn_bwd(const float* dout, const float* q, const float* k, const float* v, long ld, const float* relT,
                      const float* att, float* dq, float* dk, float* dv, long dld, float* de, int B, int L, int G, int dh,
                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = {};
    const int rc = attn_setup(a, dh, "rv_local_attn_bwd");
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(ld >= (long)G * dh && dld >= (long)G * dh, "rv_local_attn_bwd: row stride < G*dh");
    a.q = q; a.k = k; a.v = v; a.ld = ld; a.rel = relT; a.att = (float*)att; a.dout = dout;
    a.dq = dq; a.dk = dk; a.dv = dv; a.dld = dld; a.de = de; a.de_in = de; a.B = B; a.L = L; a.G = G;
    a.v4 = a.dv4 = 1;      // (as in the forward)
    const int ntile = (L + AT_TT - 1) / AT_TT, ldk = a.dhp + 4;
    size_t lds1 = ((size_t)(AT_TT + 80) * ldk + AT_TT * AT_SLD + AT_TT * AT_A3LD) * sizeof(float);
    a.rel_regs = lds1 > kAttnOccLds;
    long max_ld = ld > (long)G * dh ? ld : (long)G * dh;
    if (max_ld < (long)G * AT_W) max_ld = (long)G * AT_W;
    const AttnForm form = attn_form(dh, L, max_ld);
    if (form.tile == 32) {
        a.rel_first = a.rel_regs;                      // dq accumulates in the order the 16-frame form uses for this head shape
        size_t q32 = ((size_t)(AT2_TT + AT2_WINP + 32) * ldk + AT2_TT * AT2_SLD + AT2_TT * AT2_A3LD) * sizeof(float);
        a.rel_regs = q32 > kAttnOccLds;
        if (a.rel_regs) q32 -= (size_t)32 * ldk * sizeof(float);
        a.qkv_bytes = attn_view_bytes(L, ld, dh);
        a.do_bytes = attn_view_bytes(L, (long)G * dh, dh);
        a.rel_bytes = attn_view_bytes(AT_W, (long)G * dh, dh);
        a.co_bytes = attn_view_bytes(L, (long)G * AT_W, AT_W);
        const dim3 grid(B * ((L + AT2_TT - 1) / AT2_TT), G), block(form.waves * 64);
        if (form.waves == 10) hipLaunchKernelGGL((attn_bwd_q32_k<10>), grid, block, q32, st, a);
        else hipLaunchKernelGGL((attn_bwd_q32_k<5>), grid, block, q32, st, a);
        RV_LAUNCH_CHECK("rv_local_attn_bwd(q)");
        const size_t two32 = ((size_t)2 * AT2_WINP * ldk + 2 * AT2_WINP * 32 + 2 * AT2_TT * AT2_A2LD) * sizeof(float);
        a.seq_kv = two32 > kAttnOccLds;
        const size_t kv32 = two32 - (a.seq_kv ? (size_t)AT2_WINP * ldk * sizeof(float) : 0);
        if (form.waves == 10) hipLaunchKernelGGL((attn_bwd_kv32_k<10>), grid, block, kv32, st, a);
        else hipLaunchKernelGGL((attn_bwd_kv32_k<5>), grid, block, kv32, st, a);
        RV_LAUNCH_CHECK("rv_local_attn_bwd(kv)");
        return RV_OK;
    }
    if (a.rel_regs) lds1 -= (size_t)32 * ldk * sizeof(float);
    hipLaunchKernelGGL(attn_bwd_q_k, dim3(B * ntile, G), dim3(AT_NTHR), lds1, st, a);
    RV_LAUNCH_CHECK("rv_local_attn_bwd(q)");
    const size_t lds_two = ((size_t)2 * AT_WINP * ldk + 2 * AT_WINP * 32 + 2 * AT_TT * AT_A2LD) * sizeof(float);
    a.seq_kv = lds_two > kAttnOccLds;            // two windows at once would leave room for only one workgroup per CU
    const size_t lds2 = lds_two - (a.seq_kv ? (size_t)AT_WINP * ldk * sizeof(float) : 0);
    hipLaunchKernelGGL(attn_bwd_kv_k, dim3(B * ntile, G), dim3(AT_NTHR), lds2, st, a);
    RV_LAUNCH_CHECK("rv_local_attn_bwd(kv)");
    return RV_OK;
}

}  // extern "C"
