// Viterbi note decoding on the device: per key a three-state onset / sustain / off hidden Markov model over the two
// posteriorgrams, for up to 16 parameter sets at once.  Rolls are [T, 88] row-major float32; states 0 = OFF, 1 = ONSET, 2 = SUSTAIN.
//
// Definition (reconvat_amd/hmm.py is the yardstick).  q(x) = 0 unless x >= 0, else min(255, floor(256 x)) in float32.  The emission
// cost of state s at frame t is E_t(s) = EO[s][q(onsets[t])] + EF[s][q(frames[t])] (uint16 tables); trans = init[3], A[3][3] with
// A[from][to], -1 = forbidden.  alpha_0(s) = init[s] + E_0(s), alpha_t(s) = min_s' (alpha_{t-1}(s') + A[s'][s]) + E_t(s) in exact
// integers, bp_t(s) the LOWEST s' that attains the minimum; the last state is the lowest s that attains min_s alpha_{T-1}(s) (that
// minimum is `cost`) and the path follows bp backwards from it.
//
// The recurrence is a product of 3 x 3 matrices in the (min, +) semiring over integers, which is exactly associative, so the time
// axis is cut into chunks of 64 frames and one lane owns one (set, chunk, key).  Six launches on one stream, no host synchronisation,
// no atomics, integer work in a fixed order -- the same bits on every run:
//   1. hmm_quantise_k   both rolls -> one uint16 per cell (q(onset) | q(frame) << 8) in the workspace; every set reads these.
//   2. hmm_matrices_k   grid (chunks, sets): the chunk's uint16 tile (one contiguous span) goes to LDS with 16-byte loads, the set's
//                       tables to LDS as one 8-byte entry per q and stream (the three states' costs: one ds_read_b64 per stream and
//                       frame); lane = key multiplies the chunk's frame matrices into one.  int32 with a saturating "forbidden"
//                       value of 2^29: an allowed entry is at most 64 * (65535 + 2 * 65535) < 2^24, and 2^29 + 2^29 + 2 * 65535 < 2^31.
//   3. hmm_carry_k      grid (sets): lane = key carries alpha across the chunk matrices in int64 (a path cost passes 2^31 on long
//                       rolls, and subtracting a running minimum would let the saturation erase a state that wins again later)
//                       and leaves the alpha entering every chunk, the cost and the last state.
//   4. hmm_forward_k    grid (chunks, sets): every chunk runs its frames again from its true incoming alpha, writes the three 2-bit
//                       back-pointers of every frame as one byte INTO `states` (the slot of that frame and key), and composes the
//                       chunk's map "state at its last frame -> state at the frame before its first".
//   5. hmm_ends_k       grid (sets): lane = key walks the chunk maps backwards from the last state: the state at every chunk's end.
//   6. hmm_backtrack_k  grid (chunks, sets): every chunk walks back through its back-pointer bytes and overwrites them with the states.
// The paths are defined through the values alpha, which no order of evaluation changes, plus the fixed tie rule; steps 4 and 6 apply
// the tie rule to the true alpha, so the chunking is invisible in the output.  Back-pointers of states no path reaches are arbitrary
// and never read: a path of finite cost passes through states of finite alpha only.
//
// Frame 0 has no predecessor: it is run as a transition from a virtual frame -1 in state OFF at alpha = (0, inf, inf) under the
// matrix whose row OFF is init and whose other rows are forbidden; its back-pointer is never followed.
#include "common.h"

#define RV_HMM_KEYS 88
#define RV_HMM_CHUNK 64                        // frames per chunk (reconvat_amd/hmm.py: DEVICE_CHUNK_FRAMES)
#define RV_HMM_MAX_FRAMES (1L << 20)
#define RV_HMM_MAX_SETS 16
#define RV_HMM_BLOCK 128                       // two waves; lanes 0..87 own a key
#define RV_HMM_CARRY_DEPTH 8                   // chunk matrices hmm_carry_k loads at once
#define RV_HMM_ENDS_DEPTH 32                   // chunk maps hmm_ends_k loads at once
#define RV_HMM_INF32 (1 << 29)
#define RV_HMM_INF64 (1LL << 60)
#define RV_HMM_TILE16 (RV_HMM_CHUNK * RV_HMM_KEYS * 2 / 16)      // 16-byte words of a whole uint16 tile: 704

typedef long long i64;

struct HmmTrans {                              // by value in the kernel arguments: checked on the host before any launch
    int v[RV_HMM_MAX_SETS][12];
};

struct HmmWs {                                 // carved out of the caller's workspace; nc = chunks
    i64* alpha;                                // [G][nc][3][88]  alpha entering the chunk (after the frame before its first)
    int* mats;                                 // [G][nc][9][88]  the chunk's matrix, [from][to]
    unsigned short* q;                         // [T][88]         q(onset) | q(frame) << 8
    unsigned char* maps;                       // [G][nc][88]     2 bits per state at the chunk's last frame: state before its first
    unsigned char* ends;                       // [G][nc][88]     state at the chunk's last frame on the best path
    unsigned char* fin;                        // [G][88]         state at frame T - 1 on the best path
};

static long hmm_pad16(long n) { return (n + 15) & ~15L; }

static long hmm_bytes(long T, int G) {
    const long nc = (T + RV_HMM_CHUNK - 1) / RV_HMM_CHUNK, cells = (long)G * nc * RV_HMM_KEYS;
    return hmm_pad16(cells * 3 * (long)sizeof(i64)) + hmm_pad16(cells * 9 * (long)sizeof(int)) + hmm_pad16(T * RV_HMM_KEYS * 2) +
           2 * hmm_pad16(cells) + hmm_pad16((long)G * RV_HMM_KEYS);
}

static HmmWs hmm_carve(void* workspace, long T, int G) {
    const long nc = (T + RV_HMM_CHUNK - 1) / RV_HMM_CHUNK, cells = (long)G * nc * RV_HMM_KEYS;
    char* at = reinterpret_cast<char*>(workspace);
    HmmWs w;
    w.alpha = reinterpret_cast<i64*>(at);
    at += hmm_pad16(cells * 3 * (long)sizeof(i64));
    w.mats = reinterpret_cast<int*>(at);
    at += hmm_pad16(cells * 9 * (long)sizeof(int));
    w.q = reinterpret_cast<unsigned short*>(at);
    at += hmm_pad16(T * RV_HMM_KEYS * 2);
    w.maps = reinterpret_cast<unsigned char*>(at);
    at += hmm_pad16(cells);
    w.ends = reinterpret_cast<unsigned char*>(at);
    at += hmm_pad16(cells);
    w.fin = reinterpret_cast<unsigned char*>(at);
    return w;
}

__device__ __forceinline__ unsigned hmm_q(float x) {
    const float y = x * 256.0f;                                         // exact: a power of two
    return !(x >= 0.0f) ? 0u : y >= 255.0f ? 255u : (unsigned)(int)y;   // NaN and negatives 0; +inf and x >= 1 are 255
}

// n4 = T * 88 / 4 groups of four cells; rolls 16-byte aligned, q 8-byte aligned.
__global__ __launch_bounds__(256) void hmm_quantise_k(const float* __restrict__ onsets, const float* __restrict__ frames, long n4,
                                                      unsigned short* __restrict__ q) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 a = *reinterpret_cast<const f32x4*>(onsets + 4 * i);
    const f32x4 b = *reinterpret_cast<const f32x4*>(frames + 4 * i);
    uint2 out;
    out.x = (hmm_q(a[0]) | (hmm_q(b[0]) << 8)) | ((hmm_q(a[1]) | (hmm_q(b[1]) << 8)) << 16);
    out.y = (hmm_q(a[2]) | (hmm_q(b[2]) << 8)) | ((hmm_q(a[3]) | (hmm_q(b[3]) << 8)) << 16);
    *reinterpret_cast<uint2*>(q + 4 * i) = out;
}

// The chunk's uint16 tile and the set's tables into LDS.  The tile of chunk c starts c * 64 * 176 bytes into q and holds rows * 176
// bytes, both multiples of 16.  tab[stream * 256 + q] = (cost of OFF | cost of ONSET << 16, cost of SUSTAIN).
__device__ __forceinline__ void hmm_stage(const unsigned short* __restrict__ q, long t0, int rows,
                                          const unsigned short* __restrict__ tables, uint4* tile, uint2* tab) {
    const uint4* src = reinterpret_cast<const uint4*>(q + t0 * RV_HMM_KEYS);
    const int n16 = rows * (RV_HMM_KEYS * 2 / 16);
    for (int i = threadIdx.x; i < n16; i += RV_HMM_BLOCK) tile[i] = src[i];
    for (int i = threadIdx.x; i < 512; i += RV_HMM_BLOCK) {
        const unsigned short* col = tables + (i >> 8) * 768 + (i & 255);
        tab[i] = make_uint2((unsigned)col[0] | ((unsigned)col[256] << 16), (unsigned)col[512]);
    }
    __syncthreads();
}

__device__ __forceinline__ void hmm_emission(const uint2* tab, unsigned qq, int E[3]) {
    const uint2 eo = tab[qq & 255u], ef = tab[256 + (qq >> 8)];
    E[0] = (int)((eo.x & 0xffffu) + (ef.x & 0xffffu));
    E[1] = (int)((eo.x >> 16) + (ef.x >> 16));
    E[2] = (int)(eo.y + ef.y);
}

// Transition costs of set g as [from][to]; `first` = the matrix of frame 0 (row OFF = init, the other rows forbidden).
template <class V>
__device__ __forceinline__ void hmm_transitions(const HmmTrans& tr, int g, bool first, V inf, V A[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int v = first ? (k == 0 ? tr.v[g][s] : -1) : tr.v[g][3 + 3 * k + s];
            A[k][s] = v < 0 ? inf : (V)v;
        }
}

// M <- M (x) F, F[k][s] = A[k][s] + E[s]; saturates at RV_HMM_INF32.
__device__ __forceinline__ void hmm_mat_step(int M[3][3], const int A[3][3], const int E[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int n[3];
#pragma unroll
        for (int s = 0; s < 3; ++s)
            n[s] = min(RV_HMM_INF32, min(min(M[i][0] + A[0][s], M[i][1] + A[1][s]), M[i][2] + A[2][s]) + E[s]);
#pragma unroll
        for (int s = 0; s < 3; ++s) M[i][s] = n[s];
    }
}

__global__ __launch_bounds__(RV_HMM_BLOCK) void hmm_matrices_k(long T, int nc, const unsigned short* __restrict__ tables, HmmTrans tr,
                                                               HmmWs w) {
    __shared__ uint4 tile[RV_HMM_TILE16];
    __shared__ uint2 tab[512];
    const int c = blockIdx.x, g = blockIdx.y, p = threadIdx.x;
    const long t0 = (long)c * RV_HMM_CHUNK;
    const int rows = (int)(T - t0 < RV_HMM_CHUNK ? T - t0 : RV_HMM_CHUNK);
    hmm_stage(w.q, t0, rows, tables + (long)g * 1536, tile, tab);
    if (p >= RV_HMM_KEYS) return;
    const unsigned short* col = reinterpret_cast<const unsigned short*>(tile) + p;
    int A[3][3], M[3][3], E[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < 3; ++s) M[k][s] = k == s ? 0 : RV_HMM_INF32;
    int i = 0;
    if (c == 0) {                                                       // frame 0 under the matrix of init
        hmm_transitions<int>(tr, g, true, RV_HMM_INF32, A);
        hmm_emission(tab, col[0], E);
        hmm_mat_step(M, A, E);
        i = 1;
    }
    hmm_transitions<int>(tr, g, false, RV_HMM_INF32, A);
#pragma unroll 4
    for (; i < rows; ++i) {
        hmm_emission(tab, col[i * RV_HMM_KEYS], E);
        hmm_mat_step(M, A, E);
    }
    int* out = w.mats + ((long)g * nc + c) * 9 * RV_HMM_KEYS + p;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < 3; ++s) out[(3 * k + s) * RV_HMM_KEYS] = M[k][s];
}

__global__ __launch_bounds__(RV_HMM_BLOCK) void hmm_carry_k(int nc, HmmWs w, long* __restrict__ cost) {
    const int g = blockIdx.x, p = threadIdx.x;
    if (p >= RV_HMM_KEYS) return;
    const int* __restrict__ mats = w.mats + (long)g * nc * 9 * RV_HMM_KEYS + p;
    i64* __restrict__ alpha = w.alpha + (long)g * nc * 3 * RV_HMM_KEYS + p;
    i64 a[3] = {0, RV_HMM_INF64, RV_HMM_INF64};
    // The chain over the chunks is short work per step behind a load: the matrices of RV_HMM_CARRY_DEPTH chunks are loaded at once,
    // and those of the next group are in flight while this group is applied (chunks past the end read the last one and are skipped).
    int M[RV_HMM_CARRY_DEPTH][9], N[RV_HMM_CARRY_DEPTH][9];
#pragma unroll
    for (int d = 0; d < RV_HMM_CARRY_DEPTH; ++d)
#pragma unroll
        for (int j = 0; j < 9; ++j) N[d][j] = mats[((long)min(d, nc - 1) * 9 + j) * RV_HMM_KEYS];
    for (int c0 = 0; c0 < nc; c0 += RV_HMM_CARRY_DEPTH) {
#pragma unroll
        for (int d = 0; d < RV_HMM_CARRY_DEPTH; ++d)
#pragma unroll
            for (int j = 0; j < 9; ++j) M[d][j] = N[d][j];
        if (c0 + RV_HMM_CARRY_DEPTH < nc) {
#pragma unroll
            for (int d = 0; d < RV_HMM_CARRY_DEPTH; ++d)
#pragma unroll
                for (int j = 0; j < 9; ++j) N[d][j] = mats[((long)min(c0 + RV_HMM_CARRY_DEPTH + d, nc - 1) * 9 + j) * RV_HMM_KEYS];
        }
#pragma unroll
        for (int d = 0; d < RV_HMM_CARRY_DEPTH; ++d) {
            const int c = c0 + d;
            if (c < nc) {                                               // the same in every lane
#pragma unroll
                for (int s = 0; s < 3; ++s) alpha[((long)c * 3 + s) * RV_HMM_KEYS] = a[s];
                i64 n[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    i64 best = RV_HMM_INF64;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const i64 v = M[d][3 * k + s] >= RV_HMM_INF32 ? RV_HMM_INF64 : a[k] + (i64)M[d][3 * k + s];
                        best = v < best ? v : best;
                    }
                    n[s] = best;                                        // <= 2^60: a[k] is at most 2^60 only where it IS 2^60, and then
                }                                                       // v >= 2^60 loses against the initial best
#pragma unroll
                for (int s = 0; s < 3; ++s) a[s] = n[s];
            }
        }
    }
    int last = 0;
    i64 best = a[0];
    if (a[1] < best) { best = a[1]; last = 1; }
    if (a[2] < best) { best = a[2]; last = 2; }
    cost[g * RV_HMM_KEYS + p] = (long)best;
    w.fin[g * RV_HMM_KEYS + p] = (unsigned char)last;
}

__global__ __launch_bounds__(RV_HMM_BLOCK) void hmm_forward_k(long T, int nc, const unsigned short* __restrict__ tables, HmmTrans tr,
                                                              HmmWs w, unsigned char* __restrict__ states) {
    __shared__ uint4 tile[RV_HMM_TILE16];
    __shared__ uint2 tab[512];
    const int c = blockIdx.x, g = blockIdx.y, p = threadIdx.x;
    const long t0 = (long)c * RV_HMM_CHUNK;
    const int rows = (int)(T - t0 < RV_HMM_CHUNK ? T - t0 : RV_HMM_CHUNK);
    hmm_stage(w.q, t0, rows, tables + (long)g * 1536, tile, tab);
    if (p >= RV_HMM_KEYS) return;
    const unsigned short* col = reinterpret_cast<const unsigned short*>(tile) + p;
    const i64* in = w.alpha + ((long)g * nc + c) * 3 * RV_HMM_KEYS + p;
    unsigned char* bp_out = states + ((long)g * T + t0) * RV_HMM_KEYS + p;
    i64 a[3] = {in[0], in[RV_HMM_KEYS], in[2 * RV_HMM_KEYS]}, A[3][3];
    unsigned m[3] = {0u, 1u, 2u};                                       // state at frame t0 - 1 as a function of the state at frame t
    int E[3];
    const auto step = [&](int i) {
        hmm_emission(tab, col[i * RV_HMM_KEYS], E);
        i64 n[3];
        unsigned b[3], nm[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            i64 best = a[0] + A[0][s];
            b[s] = 0u;
            const i64 c1 = a[1] + A[1][s], c2 = a[2] + A[2][s];
            if (c1 < best) { best = c1; b[s] = 1u; }                    // strict: ties stay with the lowest predecessor
            if (c2 < best) { best = c2; b[s] = 2u; }
            best += E[s];                                               // at most 2^61 + 2^17
            n[s] = best < RV_HMM_INF64 ? best : RV_HMM_INF64;
            nm[s] = b[s] == 0u ? m[0] : b[s] == 1u ? m[1] : m[2];
        }
        bp_out[(long)i * RV_HMM_KEYS] = (unsigned char)(b[0] | (b[1] << 2) | (b[2] << 4));
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            a[s] = n[s];
            m[s] = nm[s];
        }
    };
    int i = 0;
    if (c == 0) {
        hmm_transitions<i64>(tr, g, true, RV_HMM_INF64, A);
        step(0);
        m[0] = 0u, m[1] = 1u, m[2] = 2u;                                // nothing lies before frame 0: chunk 0's map is never followed
        i = 1;
    }
    hmm_transitions<i64>(tr, g, false, RV_HMM_INF64, A);
#pragma unroll 4
    for (; i < rows; ++i) step(i);
    w.maps[((long)g * nc + c) * RV_HMM_KEYS + p] = (unsigned char)(m[0] | (m[1] << 2) | (m[2] << 4));
}

__global__ __launch_bounds__(RV_HMM_BLOCK) void hmm_ends_k(int nc, HmmWs w) {
    const int g = blockIdx.x, p = threadIdx.x;
    if (p >= RV_HMM_KEYS) return;
    const unsigned char* __restrict__ maps = w.maps + (long)g * nc * RV_HMM_KEYS + p;
    unsigned char* __restrict__ ends = w.ends + (long)g * nc * RV_HMM_KEYS + p;
    unsigned s = w.fin[g * RV_HMM_KEYS + p];
    for (int c1 = nc; c1 > 0; c1 -= RV_HMM_ENDS_DEPTH) {                // chunks c1 - 1 down to c1 - DEPTH; those before chunk 0 are skipped
        unsigned m[RV_HMM_ENDS_DEPTH];
#pragma unroll
        for (int d = 0; d < RV_HMM_ENDS_DEPTH; ++d) m[d] = maps[(long)max(c1 - 1 - d, 0) * RV_HMM_KEYS];   // no load depends on s: all in flight
#pragma unroll
        for (int d = 0; d < RV_HMM_ENDS_DEPTH; ++d) {
            const int c = c1 - 1 - d;
            if (c >= 0) {
                ends[(long)c * RV_HMM_KEYS] = (unsigned char)s;
                s = (m[d] >> (2 * s)) & 3u;
            }
        }
    }
}

__global__ __launch_bounds__(RV_HMM_BLOCK) void hmm_backtrack_k(long T, int nc, HmmWs w, unsigned char* __restrict__ states) {
    __shared__ unsigned char bp[RV_HMM_CHUNK][RV_HMM_BLOCK];
    const int c = blockIdx.x, g = blockIdx.y, p = threadIdx.x;
    if (p >= RV_HMM_KEYS) return;
    const long t0 = (long)c * RV_HMM_CHUNK;
    const int rows = (int)(T - t0 < RV_HMM_CHUNK ? T - t0 : RV_HMM_CHUNK);
    unsigned char* io = states + ((long)g * T + t0) * RV_HMM_KEYS + p;
#pragma unroll 8
    for (int i = 0; i < rows; ++i) bp[i][p] = io[(long)i * RV_HMM_KEYS];   // this lane's own column: no barrier needed
    unsigned s = w.ends[((long)g * nc + c) * RV_HMM_KEYS + p];
    for (int i = rows - 1; i >= 0; --i) {
        const unsigned b = bp[i][p];
        io[(long)i * RV_HMM_KEYS] = (unsigned char)s;
        s = (b >> (2 * s)) & 3u;
    }
}

extern "C" {

// Bytes of device scratch rv_hmm_decode needs for T frames and G parameter sets (0 for arguments out of range).
long rv_hmm_workspace_bytes(long T, int G) {
    if (T < 1 || T > RV_HMM_MAX_FRAMES || G < 1 || G > RV_HMM_MAX_SETS) return 0;
    return hmm_bytes(T, G);
}

int rv_hmm_decode(const float* onsets, const float* frames, long T, const unsigned short* tables, const int* trans, int G,
                  unsigned char* states, long* cost, void* workspace, long workspace_bytes, void* stream) {
    RV_CHECK_ARG(onsets && frames && tables && trans && states && cost && workspace, "rv_hmm_decode: null pointer");
    RV_CHECK_ARG(T >= 1 && T <= RV_HMM_MAX_FRAMES, "rv_hmm_decode: T %ld not in 1..%ld", T, RV_HMM_MAX_FRAMES);
    RV_CHECK_ARG(G >= 1 && G <= RV_HMM_MAX_SETS, "rv_hmm_decode: G %d not in 1..%d", G, RV_HMM_MAX_SETS);
    HmmTrans tr;
    for (int g = 0; g < G; ++g) {
        for (int j = 0; j < 12; ++j) {
            const int v = trans[g * 12 + j];
            RV_CHECK_ARG(v >= -1 && v <= 65535, "rv_hmm_decode: trans[%d][%d] = %d not in -1..65535", g, j, v);
            tr.v[g][j] = v;
        }
        RV_CHECK_ARG(tr.v[g][0] >= 0 && tr.v[g][3] >= 0, "rv_hmm_decode: set %d forbids init[OFF] or A[OFF][OFF]: no path is left", g);
    }
    for (int g = G; g < RV_HMM_MAX_SETS; ++g)
        for (int j = 0; j < 12; ++j) tr.v[g][j] = 0;
    RV_CHECK_ARG(((((uintptr_t)onsets) | ((uintptr_t)frames) | ((uintptr_t)workspace)) & 15) == 0 && (((uintptr_t)tables) & 1) == 0 &&
                     (((uintptr_t)cost) & 7) == 0,
                 "rv_hmm_decode: misaligned roll, table, cost or workspace");
    RV_CHECK_ARG(workspace_bytes >= hmm_bytes(T, G), "rv_hmm_decode: workspace of %ld bytes, %ld needed", workspace_bytes,
                 hmm_bytes(T, G));
    const int nc = cdiv(T, RV_HMM_CHUNK);
    const HmmWs w = hmm_carve(workspace, T, G);
    const long n4 = T * RV_HMM_KEYS / 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hmm_quantise_k, dim3(cdiv(n4, 256)), dim3(256), 0, st, onsets, frames, n4, w.q);
    hipLaunchKernelGGL(hmm_matrices_k, dim3(nc, G), dim3(RV_HMM_BLOCK), 0, st, T, nc, tables, tr, w);
    hipLaunchKernelGGL(hmm_carry_k, dim3(G), dim3(RV_HMM_BLOCK), 0, st, nc, w, cost);
    hipLaunchKernelGGL(hmm_forward_k, dim3(nc, G), dim3(RV_HMM_BLOCK), 0, st, T, nc, tables, tr, w, states);
    hipLaunchKernelGGL(hmm_ends_k, dim3(G), dim3(RV_HMM_BLOCK), 0, st, nc, w);
    hipLaunchKernelGGL(hmm_backtrack_k, dim3(nc, G), dim3(RV_HMM_BLOCK), 0, st, T, nc, w, states);
    RV_LAUNCH_CHECK("rv_hmm_decode");
    return RV_OK;
}

}  // extern "C"
