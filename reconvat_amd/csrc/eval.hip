// Whole-song evaluation on the device: note decoding of the posteriorgrams, the painted piano roll of the decoded
// notes, and the integer counters behind the frame metrics.  Rolls are [T, 88] row-major (352 B per float row, 88 B per byte row).
//
// Decode.  Per pitch, with on = onset > thr_on, fr = frame > thr_fr (float32 compares), act = on | fr:
//   start[t]   = on[t] & ~on[t-1] (& fr[t] under rule1)                 -- a note begins          (needs the row before)
//   end(t)     = min { t' >= t : !act[t'] }, T if there is none         -- runs BACKWARDS in time
//   painted[t] = act[t] & (start[t] | painted[t-1])                     -- runs FORWARDS in time
// A start implies on[t], hence act[t], hence end > t: every start is a note, so the note count is the popcount of `start`.
// painted is what the host's notes_to_frames paints: [t, end) of every note = from the first start of an active run to its end.
//
// The time axis is cut into tiles of 64 frames; one tile of one pitch is three 64-bit masks (bit i = frame t0 + i; frames >= T
// are 0 = inactive, which makes "end = T" fall out of the last tile by itself).  Three launches on one stream, no host
// synchronisation between them, no atomics on global memory, no look-back -- the carries are a second pass:
//   1. eval_masks_k   one workgroup per tile: the tile of both rolls is ONE contiguous span (64 * 352 B), loaded with 16-byte
//                     loads, thresholded into LDS bytes; 88 work items then gather their column into masks.  Writes act / start
//                     masks and the tile's note count.
//   2. eval_carry_k   one workgroup: per pitch a forward sweep over the tiles (painted state entering each tile: a tile generates
//                     a carry if its last frame is painted from inside, and passes the incoming one iff all 64 frames are active
//                     -- so a run longer than a tile threads through whole tiles) and a backward sweep (next inactive frame after
//                     each tile); one wave turns the per-tile note counts into exclusive offsets and the total.
//   3. eval_emit_k    one workgroup per tile: painted masks by carry-propagating addition, the painted roll written as 4-byte
//                     words, and the notes of the tile written at offset[tile] + rank in (t, pitch) order = np.nonzero's order.
// Everything is integer work on fixed data in a fixed order: the output bits do not depend on scheduling.
//
// Frame counters.  One work item per frame reads its two 88-byte rows, counts n_ref, n_est, c = |ref & est| and the chroma
// c = sum over the 12 pitch classes of min(ref_k, est_k); workgroups write int64 partial sums of the fourteen counters and a
// one-workgroup launch adds the partials in index order.  Integer arithmetic only; the host forms the ratios in float64.
#include "common.h"

#define RV_EVAL_KEYS 88
#define RV_EVAL_TILE 64
#define RV_EVAL_MIN_MIDI 21
#define RV_EVAL_MAX_FRAMES (1L << 24)          // T * 88 and the note count stay far inside int32
#define RV_EVAL_NCOUNT 14

typedef unsigned long long u64;

// Frames of the active runs of `act` from their first `start` on (start must be a subset of act): adding start to act ripples a
// carry from each start to the end of its run, the xor shows the flipped frames (plus the one past the run, masked off again).
__device__ __forceinline__ u64 paint_runs(u64 start, u64 act) { return (((start + act) ^ act) | start) & act; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct EvalWs {                                // carved out of the caller's workspace; nt = tiles
    u64* act;                                  // [nt][88]
    u64* start;                                // [nt][88]
    int* cin;                                  // [nt][88]  painted state of the frame before the tile
    int* nxt;                                  // [nt][88]  first inactive frame at or after the END of the tile (T if none)
    int* cnt;                                  // [nt]      notes that start in the tile
    int* base;                                 // [nt + 1]  exclusive prefix of cnt; base[nt] = all notes
};

static long eval_decode_bytes(long nt) {
    return nt * RV_EVAL_KEYS * (2 * (long)sizeof(u64) + 2 * (long)sizeof(int)) + (2 * nt + 2) * (long)sizeof(int);
}

static EvalWs eval_carve(void* workspace, long nt) {
    EvalWs w;
    w.act = reinterpret_cast<u64*>(workspace);
    w.start = w.act + nt * RV_EVAL_KEYS;
    w.cin = reinterpret_cast<int*>(w.start + nt * RV_EVAL_KEYS);
    w.nxt = w.cin + nt * RV_EVAL_KEYS;
    w.cnt = w.nxt + nt * RV_EVAL_KEYS;
    w.base = w.cnt + nt;
    return w;
}

__global__ __launch_bounds__(256) void eval_masks_k(const float* __restrict__ onsets, const float* __restrict__ frames, long T,
                                                    float thr_on, float thr_fr, int rule1, EvalWs w) {
    __shared__ __attribute__((aligned(16))) unsigned char bits[RV_EVAL_TILE * RV_EVAL_KEYS];      // bit 0 on, bit 1 fr
    __shared__ int total;
    const long k = blockIdx.x, t0 = k * RV_EVAL_TILE;
    const int rows = (int)(T - t0 < RV_EVAL_TILE ? T - t0 : RV_EVAL_TILE);
    const int n = rows * RV_EVAL_KEYS;                                  // a multiple of 4: rows never split a 16-byte load
    const float* o = onsets + t0 * RV_EVAL_KEYS;
    const float* f = frames + t0 * RV_EVAL_KEYS;
    if (threadIdx.x == 0) total = 0;
    for (int i = threadIdx.x * 4; i < RV_EVAL_TILE * RV_EVAL_KEYS; i += 256 * 4) {
        unsigned word = 0;
        if (i < n) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(o + i);
            const f32x4 b = *reinterpret_cast<const f32x4*>(f + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= ((a[j] > thr_on ? 1u : 0u) | (b[j] > thr_fr ? 2u : 0u)) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(bits + i) = word;
    }
    __syncthreads();
    const int p = threadIdx.x;
    if (p < RV_EVAL_KEYS) {
        u64 on = 0, fr = 0;
#pragma unroll 8
        for (int t = 0; t < RV_EVAL_TILE; ++t) {
            const unsigned b = bits[t * RV_EVAL_KEYS + p];
            on |= (u64)(b & 1u) << t;
            fr |= (u64)(b >> 1) << t;
        }
        const u64 prev = (t0 > 0 && onsets[(t0 - 1) * RV_EVAL_KEYS + p] > thr_on) ? 1ull : 0ull;
        u64 start = on & ~((on << 1) | prev);
        if (rule1) start &= fr;
        w.act[k * RV_EVAL_KEYS + p] = on | fr;
        w.start[k * RV_EVAL_KEYS + p] = start;
        atomicAdd(&total, __popcll(start));                             // LDS, integer: order-independent
    }
    __syncthreads();
    if (threadIdx.x == 0) w.cnt[k] = total;
}

__global__ __launch_bounds__(256) void eval_carry_k(long T, int nt, EvalWs w, int* __restrict__ count) {
    const int p = threadIdx.x;
    if (p < RV_EVAL_KEYS) {
        int c = 0;
        for (int k = 0; k < nt; ++k) {
            const u64 a = w.act[(long)k * RV_EVAL_KEYS + p], s = w.start[(long)k * RV_EVAL_KEYS + p];
            w.cin[(long)k * RV_EVAL_KEYS + p] = c;
            const int gen = (int)(paint_runs(s, a) >> 63);
            c = gen | ((a == ~0ull) ? c : 0);
        }
        int no = (int)T;
        for (int k = nt - 1; k >= 0; --k) {
            const u64 a = w.act[(long)k * RV_EVAL_KEYS + p];
            w.nxt[(long)k * RV_EVAL_KEYS + p] = no;
            if (~a) no = k * RV_EVAL_TILE + __builtin_ctzll(~a);
        }
    } else if (threadIdx.x >= 128 && threadIdx.x < 192) {               // one whole wave: exclusive scan of the tile counts
        const int lane = threadIdx.x - 128;
        int run = 0;
        for (int k0 = 0; k0 < nt; k0 += 64) {
            const int k = k0 + lane;
            const int c = k < nt ? w.cnt[k] : 0;
            int v = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o, 64);
                if (lane >= o) v += u;
            }
            if (k < nt) w.base[k] = run + v - c;
            run += __shfl(v, 63, 64);
        }
        if (lane == 0) {
            w.base[nt] = run;
            *count = run;
        }
    }
}

__global__ __launch_bounds__(256) void eval_emit_k(long T, EvalWs w, int* __restrict__ notes, long max_notes,
                                                   unsigned char* __restrict__ painted) {
    __shared__ u64 s_paint[RV_EVAL_KEYS], s_start[RV_EVAL_KEYS], s_act[RV_EVAL_KEYS];
    __shared__ int s_nxt[RV_EVAL_KEYS];
    const long k = blockIdx.x, t0 = k * RV_EVAL_TILE;
    const int rows = (int)(T - t0 < RV_EVAL_TILE ? T - t0 : RV_EVAL_TILE);
    if (threadIdx.x < RV_EVAL_KEYS) {
        const int p = threadIdx.x;
        const u64 a = w.act[k * RV_EVAL_KEYS + p], s = w.start[k * RV_EVAL_KEYS + p];
        const u64 carry = (u64)(w.cin[k * RV_EVAL_KEYS + p] & 1) & a;  // the run of the frame before continues into frame 0
        s_paint[p] = paint_runs(s | carry, a);
        s_start[p] = s;
        s_act[p] = a;
        s_nxt[p] = w.nxt[k * RV_EVAL_KEYS + p];
    }
    __syncthreads();
    const int n = rows * RV_EVAL_KEYS;
    unsigned char* out = painted + t0 * RV_EVAL_KEYS;
    for (int i = threadIdx.x * 4; i < n; i += 256 * 4) {
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = (i + j) / RV_EVAL_KEYS, p = (i + j) - t * RV_EVAL_KEYS;
            word |= (unsigned)((s_paint[p] >> t) & 1ull) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(out + i) = word;
    }
    if (threadIdx.x < 64) {                                             // wave 0: lane = frame of the tile
        const int t = threadIdx.x;
        int c = 0;
        for (int p = 0; p < RV_EVAL_KEYS; ++p) c += (int)((s_start[p] >> t) & 1ull);
        int v = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (t >= o) v += u;
        }
        long off = (long)w.base[k] + (v - c);
        if (c) {
            for (int p = 0; p < RV_EVAL_KEYS; ++p) {
                if ((s_start[p] >> t) & 1ull) {
                    const u64 m = ~s_act[p] & (~0ull << t);
                    const int end = m ? (int)t0 + __builtin_ctzll(m) : s_nxt[p];
                    if (off < max_notes) {
                        notes[3 * off] = (int)t0 + t;
                        notes[3 * off + 1] = p;
                        notes[3 * off + 2] = end;
                    }
                    ++off;
                }
            }
        }
    }
}

// ---- frame counters ----------------------------------------------------------------------------------------------------------
// out order: plain (c, n_ref, n_est, sub, miss, fa, tot) then chroma (the same seven)
__global__ __launch_bounds__(256) void eval_frame_counts_k(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ est,
                                                           long T, long* __restrict__ partial) {
    __shared__ int red[4][RV_EVAL_NCOUNT];
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    int v[RV_EVAL_NCOUNT];
#pragma unroll
    for (int j = 0; j < RV_EVAL_NCOUNT; ++j) v[j] = 0;
    if (t < T) {
        const u64* r = reinterpret_cast<const u64*>(ref + t * RV_EVAL_KEYS);
        const u64* e = reinterpret_cast<const u64*>(est + t * RV_EVAL_KEYS);
        int rk[12], ek[12], c = 0;
#pragma unroll
        for (int q = 0; q < 12; ++q) rk[q] = ek[q] = 0;
#pragma unroll
        for (int g = 0; g < RV_EVAL_KEYS / 8; ++g) {
            const u64 rw = r[g], ew = e[g];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int rb = ((rw >> (8 * j)) & 0xffull) != 0, eb = ((ew >> (8 * j)) & 0xffull) != 0;
                const int q = (RV_EVAL_MIN_MIDI + g * 8 + j) % 12;      // compile-time after unrolling
                rk[q] += rb;
                ek[q] += eb;
                c += rb & eb;
            }
        }
        int nr = 0, ne = 0, cc = 0;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            nr += rk[q];
            ne += ek[q];
            cc += min(rk[q], ek[q]);
        }
        const int lo = min(nr, ne), hi = max(nr, ne);
        v[0] = c;  v[1] = nr; v[2] = ne; v[3] = lo - c;  v[4] = max(0, nr - ne); v[5] = max(0, ne - nr); v[6] = hi - c;
        v[7] = cc; v[8] = nr; v[9] = ne; v[10] = lo - cc; v[11] = v[4];          v[12] = v[5];           v[13] = hi - cc;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < RV_EVAL_NCOUNT; ++j) {
        const int s = wave_sum_i(v[j]);                                 // <= 64 * 88
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < RV_EVAL_NCOUNT)
        partial[(long)blockIdx.x * RV_EVAL_NCOUNT + threadIdx.x] =
            (long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void eval_frame_reduce_k(const long* __restrict__ partial, int nb, long* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < RV_EVAL_NCOUNT) {
        long s = 0;
        for (int b = 0; b < nb; ++b) s += partial[(long)b * RV_EVAL_NCOUNT + j];
        out[j] = s;
    }
}

extern "C" {

// Bytes of device scratch that rv_eval_decode and rv_eval_frame_counts need for rolls of T frames (either call; 0 for a bad T).
long rv_eval_workspace_bytes(long T) {
    if (T < 1 || T > RV_EVAL_MAX_FRAMES) return 0;
    const long nt = (T + RV_EVAL_TILE - 1) / RV_EVAL_TILE, nb = (T + 255) / 256;
    const long a = eval_decode_bytes(nt), b = nb * RV_EVAL_NCOUNT * (long)sizeof(long);
    return ((a > b ? a : b) + 15) & ~15L;
}

// onsets, frames: [T, 88] float32 (16-byte aligned, may alias).  rule: 1 = rule1, 2 = rule2.  notes: [max_notes, 3] int32 rows
// (t, pitch, end) in (t, pitch) order; *count (device) receives the number of notes the rolls hold -- rows past max_notes are not
// written, so count > max_notes tells the caller its buffer was too small (88 * ceil(T / 2) always suffices).  painted: [T, 88]
// uint8 (4-byte aligned) = the roll of the notes.
int rv_eval_decode(const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold, int rule, int* notes,
                   long max_notes, int* count, unsigned char* painted, void* workspace, long workspace_bytes, void* stream) {
    RV_CHECK_ARG(onsets && frames && notes && count && painted && workspace, "rv_eval_decode: null pointer");
    RV_CHECK_ARG(T >= 1 && T <= RV_EVAL_MAX_FRAMES, "rv_eval_decode: T %ld not in 1..%ld", T, RV_EVAL_MAX_FRAMES);
    RV_CHECK_ARG(rule == 1 || rule == 2, "rv_eval_decode: rule %d (1 = rule1, 2 = rule2)", rule);
    RV_CHECK_ARG(max_notes >= 1, "rv_eval_decode: empty note buffer");
    RV_CHECK_ARG(((((uintptr_t)onsets) | ((uintptr_t)frames)) & 15) == 0 && (((uintptr_t)painted) & 3) == 0 &&
                     (((uintptr_t)workspace) & 7) == 0,
                 "rv_eval_decode: misaligned roll or workspace");
    RV_CHECK_ARG(workspace_bytes >= rv_eval_workspace_bytes(T), "rv_eval_decode: workspace of %ld bytes, %ld needed", workspace_bytes,
                 rv_eval_workspace_bytes(T));
    const int nt = cdiv(T, RV_EVAL_TILE);
    const EvalWs w = eval_carve(workspace, nt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_masks_k, dim3(nt), dim3(256), 0, st, onsets, frames, T, onset_threshold, frame_threshold, rule == 1 ? 1 : 0, w);
    hipLaunchKernelGGL(eval_carry_k, dim3(1), dim3(256), 0, st, T, nt, w, count);
    hipLaunchKernelGGL(eval_emit_k, dim3(nt), dim3(256), 0, st, T, w, notes, max_notes, painted);
    RV_LAUNCH_CHECK("rv_eval_decode");
    return RV_OK;
}

// ref, est: [T, 88] uint8 rolls (8-byte aligned; a key is on where its byte is non-zero).  out: 14 int64 on the device -- for the
// plain and then the chroma set the sums over frames of c, n_ref, n_est, min(n_ref, n_est) - c, max(0, n_ref - n_est),
// max(0, n_est - n_ref), max(n_ref, n_est) - c.
int rv_eval_frame_counts(const unsigned char* ref, const unsigned char* est, long T, long* out, void* workspace, long workspace_bytes,
                         void* stream) {
    RV_CHECK_ARG(ref && est && out && workspace, "rv_eval_frame_counts: null pointer");
    RV_CHECK_ARG(T >= 1 && T <= RV_EVAL_MAX_FRAMES, "rv_eval_frame_counts: T %ld not in 1..%ld", T, RV_EVAL_MAX_FRAMES);
    RV_CHECK_ARG(((((uintptr_t)ref) | ((uintptr_t)est) | ((uintptr_t)out) | ((uintptr_t)workspace)) & 7) == 0,
                 "rv_eval_frame_counts: misaligned roll, output or workspace");
    RV_CHECK_ARG(workspace_bytes >= rv_eval_workspace_bytes(T), "rv_eval_frame_counts: workspace of %ld bytes, %ld needed", workspace_bytes,
                 rv_eval_workspace_bytes(T));
    const int nb = cdiv(T, 256);
    long* partial = reinterpret_cast<long*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_frame_counts_k, dim3(nb), dim3(256), 0, st, ref, est, T, partial);
    hipLaunchKernelGGL(eval_frame_reduce_k, dim3(1), dim3(64), 0, st, (const long*)partial, nb, out);
    RV_LAUNCH_CHECK("rv_eval_frame_counts");
    return RV_OK;
}

}  // extern "C"
