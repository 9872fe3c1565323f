// Whole-song evaluation on the device: note decoding of the posteriorgrams, the painted piano roll of the decoded
// notes, and the integer counters behind the frame metrics.  Rolls are [T, 88] row-major (352 B per float row, 88 B per byte row).
//
// Decode.  Per pitch, with on = onset > thr_on, fr = frame > thr_fr (float32 compares), act = on | fr:
//   start[t]   = on[t] & ~on[t-1] (& fr[t] under rule1)                 -- a note begins          (needs the row before)
//   end(t)     = min { t' >= t : !act[t'] }, T if there is none         -- runs BACKWARDS in time
//   painted[t] = act[t] & (start[t] | painted[t-1])                     -- runs FORWARDS in time
// A start implies on[t], hence act[t], hence end > t: every start is a note, so the note count is the popcount of `start`.
// painted is what the host's notes_to_frames paints: [t, end) of every note = from the first start of an active run to its end.
// Note clean-up (min_frames = m, bridge_gap = g; the lines above are m = 1, g = 0): act is bridged first -- an inactive
// run of at most g frames between two active frames counts as active; start stays as it is -- and a start is KEPT iff end - t >= m.
// Only kept starts are notes and only they paint.  All notes of one active run end with the run, so its first start is its longest
// note: a run is painted, from that first start, iff the first start is kept, and the recurrences hold with `kept` for `start`.
//
// The time axis is cut into tiles of 64 frames; one tile of one pitch is three 64-bit masks (bit i = frame t0 + i; frames >= T
// are 0 = inactive, which makes "end = T" fall out of the last tile by itself).  Three launches on one stream, no host
// synchronisation between them, no atomics on global memory, no look-back -- the carries are a second pass:
//   1. eval_masks_k   one workgroup per tile: the tile of both rolls is ONE contiguous span (64 * 352 B), loaded with 16-byte
//                     loads, thresholded into LDS bytes; 88 work items then gather their column into masks.  Writes the
//                     (unbridged) act and the start masks, and the number of starts in the tile.
//   2. eval_carry_k   one workgroup: per pitch a forward sweep over the tiles (painted state entering each tile: a tile generates
//                     a carry if its last frame is painted from inside, and passes the incoming one iff all 64 frames are active
//                     -- so a run longer than a tile threads through whole tiles) and a backward sweep (next inactive frame after
//                     each tile, in the bridged activity); one wave turns the per-tile note counts into exclusive offsets and the
//                     total.  With clean-up the forward sweep comes after the backward one, which tells it how far the run that
//                     leaves a tile goes on, hence which starts of the tile are kept (eval_emit_k works them out again the same
//                     way), and it counts the kept starts per tile itself (LDS) in place of the counts of eval_masks_k.
//   3. eval_emit_k    one workgroup per tile: painted masks by carry-propagating addition, the painted roll written as 4-byte
//                     words, and the notes of the tile written at offset[tile] + rank in (t, pitch) order = np.nonzero's order.
// Everything is integer work on fixed data in a fixed order: the output bits do not depend on scheduling.
//
// Frame counters.  One work item per frame reads its two 88-byte rows, counts n_ref, n_est, c = |ref & est| and the chroma
// c = sum over the 12 pitch classes of min(ref_k, est_k); workgroups write int64 partial sums of the fourteen counters and a
// one-workgroup launch adds the partials in index order.  Integer arithmetic only; the host forms the ratios in float64.
//
// Threshold sweep.  The counters behind note and frame precision / recall at every pair of a grid of onset and frame
// thresholds, two launches:
//   1. sweep_masks_k  one workgroup per tile: both float tiles and the reference roll's tile go to LDS once; one work item per
//                     (threshold, pitch) gathers its column into a 64-bit mask -- per onset threshold `on` and its rising edges
//                     `rise`, per frame threshold `fr`, and once the reference roll -- so the rolls are read once for the whole grid.
//   2. sweep_count_k  one workgroup per grid point, one work item per pitch.  A forward sweep over the tiles paints the estimate
//                     (paint_runs with the painted state of the last frame as carry) and counts notes, painted frames and frames
//                     painted on both sides -- with clean-up the kept notes: whether a start is kept shows in the next tile at
//                     the latest, so the sweep stays one pass with one tile of look-ahead.  Then the reference notes of the pitch
//                     (rows sorted by pitch, then time; the range of a pitch is found by bisection) are walked in time order: a
//                     reference note starting at t can only hit an estimate of the same pitch starting at t - 1, t or t + 1 (one
//                     hop <= 50 ms < two hops) and takes the earliest one that is still free (with clean-up: a KEPT one, its end
//                     in the bridged activity) -- on a candidate graph that is a union of time-monotone paths this is a maximum
//                     matching.  The offset test is integer: the host hands over, per reference note, how many frames the
//                     estimate may end early or late, evaluated once with its own float64 expressions.
// Integer work in a fixed order, no atomics: the counters are the same bits on every run.
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

// ---- note clean-up ---------------------------------------------------------------------------------------------
// Two tiles of one pitch side by side: lo holds the 64 frames before those of hi.  Shifts are by 1..31 frames and fill with 0.
struct Pair {
    u64 lo, hi;
};
__device__ __forceinline__ Pair later(Pair x, int n) { return {x.lo << n, (x.hi << n) | (x.lo >> (64 - n))}; }
__device__ __forceinline__ Pair earlier(Pair x, int n) { return {(x.lo >> n) | (x.hi << (64 - n)), x.hi >> n}; }

// hi word of: frame t is on iff one of the frames t - g .. t of x is (g = 0..31; spans doubled, then topped up to g + 1).
__device__ __forceinline__ u64 any_behind(Pair x, int g) {
    int n = 1;
    for (; 2 * n <= g + 1; n *= 2) {
        const Pair y = later(x, n);
        x.lo |= y.lo;
        x.hi |= y.hi;
    }
    if (n < g + 1) x.hi |= later(x, g + 1 - n).hi;
    return x.hi;
}

// lo word of: frame t is on iff all of the frames t .. t + g of x are (g = 0..31).
__device__ __forceinline__ u64 all_ahead(Pair x, int g) {
    int n = 1;
    for (; 2 * n <= g + 1; n *= 2) {
        const Pair y = earlier(x, n);
        x.lo &= y.lo;
        x.hi &= y.hi;
    }
    if (n < g + 1) x.lo &= earlier(x, g + 1 - n).lo;
    return x.lo;
}

// Activity of tile k of one pitch with every inactive run of at most g frames between two active frames switched on.  raw(k) is the
// unbridged activity of tile k.  g <= 31 < 64, so the tile before and the tile after hold all that decides: a frame stays off iff
// some g + 1 consecutive frames around it are all off, i.e. bridging is the closing "any_behind, then all_ahead" of the three tiles.
// The tile before tile 0 and the tile after the last one read as 0, and so do the frames >= T: 64 inactive frames are a run longer
// than g, so the runs at either end of the roll are never bridged.  g = 0 loads and computes nothing beyond raw(k).
template <class Raw>
__device__ __forceinline__ u64 bridged(Raw raw, long k, long nt, int g) {
    const u64 cur = raw(k);
    if (g == 0) return cur;
    const u64 prev = k > 0 ? raw(k - 1) : 0ull, next = k + 1 < nt ? raw(k + 1) : 0ull;
    return all_ahead({any_behind({prev, cur}, g), any_behind({cur, next}, g)}, g);
}

// The starts of a tile whose note lasts at least m frames: the m frames from the start on are all active.  act = the (bridged)
// activity of the tile, next = that of the tile after it -- only its frames up to the first inactive one matter.
__device__ __forceinline__ u64 kept_starts(u64 start, u64 act, u64 next, int m) { return start & all_ahead({act, next}, m - 1); }

// `next` for kept_starts from the first inactive frame at or after the end of the tile: the run that leaves the tile stays active up
// to there, and that many frames of the next tile are all kept_starts needs.
__device__ __forceinline__ u64 frames_ahead(int next_off, long tile_end) {
    const long ahead = next_off - tile_end;
    return ahead >= RV_EVAL_TILE ? ~0ull : ahead > 0 ? (1ull << ahead) - 1 : 0ull;
}

// Every kernel below that takes m = min_frames and g = bridge_gap is compiled twice: CLEAN = false is the (1, 0) case with both folded
// away -- the loops over the tiles keep their loads free of branches, as they were before the clean-up existed.

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct EvalWs {                                // carved out of the caller's workspace; nt = tiles
    u64* act;                                  // [nt][88]  unbridged activity
    u64* start;                                // [nt][88]  starts, kept or not
    int* cin;                                  // [nt][88]  painted state of the frame before the tile
    int* nxt;                                  // [nt][88]  first inactive frame at or after the END of the tile (T if none), bridged
    int* cnt;                                  // [nt]      starts in the tile, kept or not: the notes of the tile at (1, 0)
    int* base;                                 // [nt + 1]  exclusive prefix of the kept notes per tile; base[nt] = all notes
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

#define RV_EVAL_CARRY_CHUNK 256                // tiles whose kept-note counts eval_carry_k<true> holds in LDS at a time

// One wave: base[k] = run + the exclusive prefix of count(k) over k0 <= k < k1; returns run + their sum.
template <class Count>
__device__ __forceinline__ int scan_tile_counts(int lane, int k0, int k1, int run, Count count, int* __restrict__ base) {
    for (int kk = k0; kk < k1; kk += 64) {
        const int k = kk + lane;
        const int n = k < k1 ? count(k) : 0;
        int v = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (k < k1) base[k] = run + v - n;
        run += __shfl(v, 63, 64);
    }
    return run;
}

// One workgroup.  Work items 0..87 own a pitch each and sweep over the tiles, forwards (painted state entering each tile) and
// backwards (next inactive frame after each tile); wave 2 turns the note counts of the tiles into offsets.  The loops over the tiles
// are free of branches, 64-bit stores and atomics, so that the loads of consecutive tiles overlap.
//   (1, 0)    every start is a note: the counts are those eval_masks_k left, and wave 2 scans them while the sweeps run.
//   clean-up  the forward sweep needs the backward one (which starts of a tile are kept depends on how far the run that leaves the
//             tile goes on), so it comes second, chunk of tiles by chunk, and leaves the number of kept starts of its pitch in each
//             tile (at most 32: a byte) in LDS; wave 2 then adds the 88 bytes of every tile of the chunk and scans the sums.
template <bool CLEAN>
__global__ __launch_bounds__(256) void eval_carry_k(long T, int nt, int min_frames, int bridge_gap, EvalWs w, int* __restrict__ count) {
    __shared__ __attribute__((aligned(4))) unsigned char s_cnt[CLEAN ? RV_EVAL_CARRY_CHUNK : 1][RV_EVAL_KEYS];
    const int p = threadIdx.x, lane = threadIdx.x - 128, m = CLEAN ? min_frames : 1, g = CLEAN ? bridge_gap : 0;
    const bool sweeps = p < RV_EVAL_KEYS, scans = lane >= 0 && lane < 64;
    const auto raw = [&](long k) { return w.act[k * RV_EVAL_KEYS + p]; };
    int c = 0;                                                          // painted state of the frame before the tile
    const auto forward = [&](int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            const long at = (long)k * RV_EVAL_KEYS + p;
            const u64 a = bridged(raw, k, nt, g);
            const u64 next = CLEAN ? frames_ahead(w.nxt[at], (long)(k + 1) * RV_EVAL_TILE) : 0ull;
            const u64 s = kept_starts(w.start[at], a, next, m);
            w.cin[at] = c;
            // a tile generates a carry if its last frame is painted from inside -- from a KEPT start, the first of its run --
            // and passes the incoming one iff all 64 frames are active
            const int gen = (int)(paint_runs(s, a) >> 63);
            c = gen | ((a == ~0ull) ? c : 0);
            if (CLEAN) s_cnt[k - k0][p] = (unsigned char)__popcll(s);
        }
    };
    const auto backward = [&] {
        int no = (int)T;
        for (int k = nt - 1; k >= 0; --k) {
            const u64 a = bridged(raw, k, nt, g);
            w.nxt[(long)k * RV_EVAL_KEYS + p] = no;
            if (~a) no = k * RV_EVAL_TILE + __builtin_ctzll(~a);
        }
    };
    int run = 0;                                                        // notes before the tiles still to scan
    if (!CLEAN) {
        if (sweeps) {
            forward(0, nt);
            backward();
        } else if (scans) {
            run = scan_tile_counts(lane, 0, nt, 0, [&](int k) { return w.cnt[k]; }, w.base);
        }
    } else {
        if (sweeps) backward();
        for (int k0 = 0; k0 < nt; k0 += RV_EVAL_CARRY_CHUNK) {
            const int k1 = min(nt, k0 + RV_EVAL_CARRY_CHUNK);
            if (sweeps) forward(k0, k1);
            __syncthreads();
            if (scans) {
                const auto kept = [&](int k) {
                    const unsigned* row = reinterpret_cast<const unsigned*>(s_cnt[k - k0]);
                    int n = 0;
                    for (int q = 0; q < RV_EVAL_KEYS / 4; ++q) {
                        const unsigned pair = (row[q] & 0x00ff00ffu) + ((row[q] >> 8) & 0x00ff00ffu);
                        n += (int)((pair & 0xffffu) + (pair >> 16));
                    }
                    return n;
                };
                run = scan_tile_counts(lane, k0, k1, run, kept, w.base);
            }
            __syncthreads();
        }
    }
    if (lane == 0) {
        w.base[nt] = run;
        *count = run;
    }
}

template <bool CLEAN>
__global__ __launch_bounds__(256) void eval_emit_k(long T, int nt, int min_frames, int bridge_gap, EvalWs w, int* __restrict__ notes,
                                                   long max_notes, unsigned char* __restrict__ painted) {
    const int m = CLEAN ? min_frames : 1, g = CLEAN ? bridge_gap : 0;
    __shared__ u64 s_paint[RV_EVAL_KEYS], s_start[RV_EVAL_KEYS], s_act[RV_EVAL_KEYS];
    __shared__ int s_nxt[RV_EVAL_KEYS];
    const long k = blockIdx.x, t0 = k * RV_EVAL_TILE;
    const int rows = (int)(T - t0 < RV_EVAL_TILE ? T - t0 : RV_EVAL_TILE);
    if (threadIdx.x < RV_EVAL_KEYS) {
        const int p = threadIdx.x;
        const u64 a = bridged([&](long kk) { return w.act[kk * RV_EVAL_KEYS + p]; }, k, nt, g);
        const int nxt = w.nxt[k * RV_EVAL_KEYS + p];
        const u64 s = kept_starts(w.start[k * RV_EVAL_KEYS + p], a, CLEAN ? frames_ahead(nxt, t0 + RV_EVAL_TILE) : 0ull, m);
        const u64 carry = (u64)(w.cin[k * RV_EVAL_KEYS + p] & 1) & a;  // the run of the frame before continues into frame 0
        s_paint[p] = paint_runs(s | carry, a);
        s_start[p] = s;
        s_act[p] = a;
        s_nxt[p] = nxt;
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
                    const u64 idle = ~s_act[p] & (~0ull << t);
                    const int end = idle ? (int)t0 + __builtin_ctzll(idle) : s_nxt[p];
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

// ---- threshold sweep ---------------------------------------------------------------------------------------------------------
#define RV_SWEEP_MAX_THR 32
#define RV_SWEEP_NOUT 5                        // per grid point: notes, matched, matched with offsets, frames on both sides, frames
#define RV_SWEEP_REF_COLS 5                    // reference rows: t, pitch, end, frames the estimate may end early, ... or late

struct SweepWs {                               // carved out of the caller's workspace; nt = tiles; every array [.][nt][88]
    u64* on;                                   // [n_on]  onset roll > onset threshold
    u64* rise;                                 // [n_on]  ... and not so the frame before
    u64* fr;                                   // [n_fr]  frame roll > frame threshold
    u64* ref;                                  // [1]     reference roll != 0
};

static long sweep_bytes(long nt, int n_on, int n_fr) { return (2L * n_on + n_fr + 1) * nt * RV_EVAL_KEYS * (long)sizeof(u64); }

static SweepWs sweep_carve(void* workspace, long nt, int n_on, int n_fr) {
    SweepWs w;
    w.on = reinterpret_cast<u64*>(workspace);
    w.rise = w.on + (long)n_on * nt * RV_EVAL_KEYS;
    w.fr = w.rise + (long)n_on * nt * RV_EVAL_KEYS;
    w.ref = w.fr + (long)n_fr * nt * RV_EVAL_KEYS;
    return w;
}

__global__ __launch_bounds__(256) void sweep_masks_k(const float* __restrict__ onsets, const float* __restrict__ frames,
                                                     const unsigned char* __restrict__ ref_roll, long T, long nt,
                                                     const float* __restrict__ thr_on, int n_on, const float* __restrict__ thr_fr,
                                                     int n_fr, SweepWs w) {
    __shared__ __attribute__((aligned(16))) float s_on[RV_EVAL_TILE * RV_EVAL_KEYS];
    __shared__ __attribute__((aligned(16))) float s_fr[RV_EVAL_TILE * RV_EVAL_KEYS];
    __shared__ __attribute__((aligned(16))) unsigned char s_ref[RV_EVAL_TILE * RV_EVAL_KEYS];
    const long k = blockIdx.x, t0 = k * RV_EVAL_TILE;
    const int rows = (int)(T - t0 < RV_EVAL_TILE ? T - t0 : RV_EVAL_TILE);
    const int n = rows * RV_EVAL_KEYS;                                  // a multiple of 4: rows never split a 16-byte load
    const float* o = onsets + t0 * RV_EVAL_KEYS;
    const float* f = frames + t0 * RV_EVAL_KEYS;
    const unsigned char* r = ref_roll + t0 * RV_EVAL_KEYS;
    for (int i = threadIdx.x * 4; i < n; i += 256 * 4) {
        *reinterpret_cast<f32x4*>(s_on + i) = *reinterpret_cast<const f32x4*>(o + i);
        *reinterpret_cast<f32x4*>(s_fr + i) = *reinterpret_cast<const f32x4*>(f + i);
        *reinterpret_cast<unsigned*>(s_ref + i) = *reinterpret_cast<const unsigned*>(r + i);
    }
    __syncthreads();
    const int items = (n_on + n_fr + 1) * RV_EVAL_KEYS;
    for (int item = threadIdx.x; item < items; item += 256) {
        const int s = item / RV_EVAL_KEYS, p = item - s * RV_EVAL_KEYS;
        u64 m = 0;
        if (s < n_on + n_fr) {
            const bool is_on = s < n_on;
            const float thr = is_on ? thr_on[s] : thr_fr[s - n_on];
            const float* col = (is_on ? s_on : s_fr) + p;
            for (int t = 0; t < rows; ++t) m |= (u64)(col[t * RV_EVAL_KEYS] > thr ? 1u : 0u) << t;
            if (is_on) {
                const u64 prev = (t0 > 0 && onsets[(t0 - 1) * RV_EVAL_KEYS + p] > thr) ? 1ull : 0ull;
                w.on[((long)s * nt + k) * RV_EVAL_KEYS + p] = m;
                w.rise[((long)s * nt + k) * RV_EVAL_KEYS + p] = m & ~((m << 1) | prev);
            } else {
                w.fr[((long)(s - n_on) * nt + k) * RV_EVAL_KEYS + p] = m;
            }
        } else {
            for (int t = 0; t < rows; ++t) m |= (u64)(s_ref[t * RV_EVAL_KEYS + p] != 0 ? 1u : 0u) << t;
            w.ref[k * RV_EVAL_KEYS + p] = m;
        }
    }
}

// First index in [0, n) whose pitch column is >= pitch (n if none); rows sorted by pitch.  Terminates on any data.
__device__ __forceinline__ long sweep_lower_bound(const int* __restrict__ rows, long n, int pitch) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (rows[mid * RV_SWEEP_REF_COLS + 1] < pitch) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// min_frames, bridge_gap: of the estimate (the reference notes come decoded).
template <bool CLEAN>
__global__ __launch_bounds__(128) void sweep_count_k(long T, long nt, int n_fr, int rule1, int min_frames, int bridge_gap, SweepWs w,
                                                     const int* __restrict__ ref_notes, long n_ref, long* __restrict__ counts,
                                                     long* __restrict__ ref_totals) {
    const int m = CLEAN ? min_frames : 1, g = CLEAN ? bridge_gap : 0;
    __shared__ long red[RV_SWEEP_NOUT + 1][RV_EVAL_KEYS];
    const int i = blockIdx.x / n_fr, j = blockIdx.x - i * n_fr, p = threadIdx.x;
    if (p < RV_EVAL_KEYS) {
        const u64* on = w.on + (long)i * nt * RV_EVAL_KEYS + p;
        const u64* rise = w.rise + (long)i * nt * RV_EVAL_KEYS + p;
        const u64* fr = w.fr + (long)j * nt * RV_EVAL_KEYS + p;
        const u64* ref = w.ref + p;
        const u64 keep = rule1 ? 0ull : ~0ull;                          // rule1: a start needs the frame roll on
        const auto raw = [&](long k) { return on[k * RV_EVAL_KEYS] | fr[k * RV_EVAL_KEYS]; };
        long notes = 0, est_frames = 0, both = 0, ref_frames = 0;
        u64 carry = 0;                                                  // painted state of the frame before the tile
        // whether a start is kept shows at most m - 1 frames later: one tile of look-ahead, and only when m > 1; the tile looked
        // ahead at is handed on to the next turn, so every tile is bridged once
        const bool ahead = m > 1;
        u64 handed = ahead ? bridged(raw, 0, nt, g) : 0ull;
#pragma unroll 4
        for (long k = 0; k < nt; ++k) {
            const u64 a = ahead ? handed : bridged(raw, k, nt, g);
            const u64 next = (ahead && k + 1 < nt) ? bridged(raw, k + 1, nt, g) : 0ull;
            handed = next;
            const u64 s = kept_starts(rise[k * RV_EVAL_KEYS] & (fr[k * RV_EVAL_KEYS] | keep), a, next, m);
            const u64 r = ref[k * RV_EVAL_KEYS];
            const u64 painted = paint_runs(s | (carry & a), a);
            carry = painted >> 63;
            notes += __popcll(s);
            est_frames += __popcll(painted);
            both += __popcll(painted & r);
            ref_frames += __popcll(r);
        }
        long matched = 0, matched_off = 0;
        long used = -1, used_off = -1;                                  // start frame of the last estimate taken (they only move on)
        const long first = sweep_lower_bound(ref_notes, n_ref, p), last = sweep_lower_bound(ref_notes, n_ref, p + 1);
        for (long q = first; q < last; ++q) {
            const int* row = ref_notes + q * RV_SWEEP_REF_COLS;
            const long t = row[0], end = row[2], early = row[3], late = row[4];
            bool open = true, open_off = true;                          // this reference note is still unmatched
            for (long c = t - 1; c <= t + 1; ++c) {
                if (c < 0 || c >= T) continue;
                const long k = c >> 6;
                const int b = (int)(c & 63);
                if (!(((rise[k * RV_EVAL_KEYS] & (fr[k * RV_EVAL_KEYS] | keep)) >> b) & 1ull)) continue;
                const bool try_off = open_off && c > used_off;
                long e = T;
                if (m > 1 || try_off) {                                 // the estimate ends at the first inactive (bridged) frame
                    u64 off = ~bridged(raw, k, nt, g) & (~0ull << b);
                    long kk = k;
                    while (!off && ++kk < nt) off = ~bridged(raw, kk, nt, g);
                    if (off) e = kk * RV_EVAL_TILE + __builtin_ctzll(off);
                    if (e > T) e = T;
                }
                if (e - c < m) continue;                                // a candidate is a KEPT start (m = 1 keeps every start)
                if (open && c > used) {
                    used = c;
                    ++matched;
                    open = false;
                }
                if (try_off) {
                    const long d = e - end;
                    if (d >= -early && d <= late) {
                        used_off = c;
                        ++matched_off;
                        open_off = false;
                    }
                }
            }
        }
        red[0][p] = notes;
        red[1][p] = matched;
        red[2][p] = matched_off;
        red[3][p] = both;
        red[4][p] = est_frames;
        red[5][p] = ref_frames;
    }
    __syncthreads();
    if (threadIdx.x <= RV_SWEEP_NOUT) {
        long s = 0;
        for (int q = 0; q < RV_EVAL_KEYS; ++q) s += red[threadIdx.x][q];
        if (threadIdx.x < RV_SWEEP_NOUT) counts[(long)blockIdx.x * RV_SWEEP_NOUT + threadIdx.x] = s;
        else if (blockIdx.x == 0) ref_totals[1] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 127) ref_totals[0] = n_ref;
}

#define RV_EVAL_MAX_MIN_FRAMES 32              // the look-ahead of kept_starts and the reach of bridged stay inside one tile
#define RV_EVAL_MAX_BRIDGE_GAP 31

static long eval_workspace_bytes(long T) {
    if (T < 1 || T > RV_EVAL_MAX_FRAMES) return 0;
    const long nt = (T + RV_EVAL_TILE - 1) / RV_EVAL_TILE, nb = (T + 255) / 256;
    const long a = eval_decode_bytes(nt), b = nb * RV_EVAL_NCOUNT * (long)sizeof(long);
    return ((a > b ? a : b) + 15) & ~15L;
}

static long eval_sweep_workspace_bytes(long T, int n_on, int n_fr) {
    if (T < 1 || T > RV_EVAL_MAX_FRAMES || n_on < 1 || n_on > RV_SWEEP_MAX_THR || n_fr < 1 || n_fr > RV_SWEEP_MAX_THR) return 0;
    return (sweep_bytes((T + RV_EVAL_TILE - 1) / RV_EVAL_TILE, n_on, n_fr) + 15) & ~15L;
}

// rv_eval_decode and rv_eval_decode_clean; fn names the entry point in the error text
static int eval_decode(const char* fn, const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold,
                       int rule, int min_frames, int bridge_gap, int* notes, long max_notes, int* count, unsigned char* painted,
                       void* workspace, long workspace_bytes, void* stream) {
    RV_CHECK_ARG(onsets && frames && notes && count && painted && workspace, "%s: null pointer", fn);
    RV_CHECK_ARG(T >= 1 && T <= RV_EVAL_MAX_FRAMES, "%s: T %ld not in 1..%ld", fn, T, RV_EVAL_MAX_FRAMES);
    RV_CHECK_ARG(rule == 1 || rule == 2, "%s: rule %d (1 = rule1, 2 = rule2)", fn, rule);
    RV_CHECK_ARG(min_frames >= 1 && min_frames <= RV_EVAL_MAX_MIN_FRAMES, "%s: min_frames %d not in 1..%d", fn, min_frames,
                 RV_EVAL_MAX_MIN_FRAMES);
    RV_CHECK_ARG(bridge_gap >= 0 && bridge_gap <= RV_EVAL_MAX_BRIDGE_GAP, "%s: bridge_gap %d not in 0..%d", fn, bridge_gap,
                 RV_EVAL_MAX_BRIDGE_GAP);
    RV_CHECK_ARG(max_notes >= 1, "%s: empty note buffer", fn);
    RV_CHECK_ARG(((((uintptr_t)onsets) | ((uintptr_t)frames)) & 15) == 0 && (((uintptr_t)painted) & 3) == 0 &&
                     (((uintptr_t)workspace) & 7) == 0,
                 "%s: misaligned roll or workspace", fn);
    RV_CHECK_ARG(workspace_bytes >= eval_workspace_bytes(T), "%s: workspace of %ld bytes, %ld needed", fn, workspace_bytes,
                 eval_workspace_bytes(T));
    const int nt = cdiv(T, RV_EVAL_TILE);
    const EvalWs w = eval_carve(workspace, nt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_masks_k, dim3(nt), dim3(256), 0, st, onsets, frames, T, onset_threshold, frame_threshold, rule == 1 ? 1 : 0, w);
    if (min_frames == 1 && bridge_gap == 0) {
        hipLaunchKernelGGL(eval_carry_k<false>, dim3(1), dim3(256), 0, st, T, nt, 1, 0, w, count);
        hipLaunchKernelGGL(eval_emit_k<false>, dim3(nt), dim3(256), 0, st, T, nt, 1, 0, w, notes, max_notes, painted);
    } else {
        hipLaunchKernelGGL(eval_carry_k<true>, dim3(1), dim3(256), 0, st, T, nt, min_frames, bridge_gap, w, count);
        hipLaunchKernelGGL(eval_emit_k<true>, dim3(nt), dim3(256), 0, st, T, nt, min_frames, bridge_gap, w, notes, max_notes, painted);
    }
    RV_LAUNCH_CHECK(fn);
    return RV_OK;
}

// rv_eval_sweep and rv_eval_sweep_clean; fn names the entry point in the error text
static int eval_sweep(const char* fn, const float* onsets, const float* frames, long T, const float* onset_thresholds, int n_on,
                      const float* frame_thresholds, int n_fr, int rule, int min_frames, int bridge_gap, const int* ref_notes, long n_ref,
                      const unsigned char* ref_roll, long* counts, long* ref_totals, void* workspace, long workspace_bytes, void* stream) {
    RV_CHECK_ARG(onsets && frames && onset_thresholds && frame_thresholds && ref_roll && counts && ref_totals && workspace,
                 "%s: null pointer", fn);
    RV_CHECK_ARG(T >= 1 && T <= RV_EVAL_MAX_FRAMES, "%s: T %ld not in 1..%ld", fn, T, RV_EVAL_MAX_FRAMES);
    RV_CHECK_ARG(n_on >= 1 && n_on <= RV_SWEEP_MAX_THR && n_fr >= 1 && n_fr <= RV_SWEEP_MAX_THR,
                 "%s: grid of %d x %d thresholds, 1..%d each", fn, n_on, n_fr, RV_SWEEP_MAX_THR);
    RV_CHECK_ARG(rule == 1 || rule == 2, "%s: rule %d (1 = rule1, 2 = rule2)", fn, rule);
    RV_CHECK_ARG(min_frames >= 1 && min_frames <= RV_EVAL_MAX_MIN_FRAMES, "%s: min_frames %d not in 1..%d", fn, min_frames,
                 RV_EVAL_MAX_MIN_FRAMES);
    RV_CHECK_ARG(bridge_gap >= 0 && bridge_gap <= RV_EVAL_MAX_BRIDGE_GAP, "%s: bridge_gap %d not in 0..%d", fn, bridge_gap,
                 RV_EVAL_MAX_BRIDGE_GAP);
    RV_CHECK_ARG(n_ref >= 0 && n_ref <= RV_EVAL_KEYS * ((T + 1) / 2) && (n_ref == 0 || ref_notes),
                 "%s: %ld reference notes (at most 88 * ceil(T / 2), and a buffer for them)", fn, n_ref);
    RV_CHECK_ARG(((((uintptr_t)onsets) | ((uintptr_t)frames)) & 15) == 0 && (((uintptr_t)ref_roll) & 3) == 0 &&
                     ((((uintptr_t)workspace) | ((uintptr_t)counts) | ((uintptr_t)ref_totals)) & 7) == 0 &&
                     ((((uintptr_t)onset_thresholds) | ((uintptr_t)frame_thresholds) | ((uintptr_t)ref_notes)) & 3) == 0,
                 "%s: misaligned roll, list, output or workspace", fn);
    RV_CHECK_ARG(workspace_bytes >= eval_sweep_workspace_bytes(T, n_on, n_fr), "%s: workspace of %ld bytes, %ld needed", fn,
                 workspace_bytes, eval_sweep_workspace_bytes(T, n_on, n_fr));
    const long nt = (T + RV_EVAL_TILE - 1) / RV_EVAL_TILE;
    const SweepWs w = sweep_carve(workspace, nt, n_on, n_fr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sweep_masks_k, dim3((unsigned)nt), dim3(256), 0, st, onsets, frames, ref_roll, T, nt, onset_thresholds, n_on,
                       frame_thresholds, n_fr, w);
    if (min_frames == 1 && bridge_gap == 0)
        hipLaunchKernelGGL(sweep_count_k<false>, dim3(n_on * n_fr), dim3(128), 0, st, T, nt, n_fr, rule == 1 ? 1 : 0, 1, 0, w, ref_notes,
                           n_ref, counts, ref_totals);
    else
        hipLaunchKernelGGL(sweep_count_k<true>, dim3(n_on * n_fr), dim3(128), 0, st, T, nt, n_fr, rule == 1 ? 1 : 0, min_frames,
                           bridge_gap, w, ref_notes, n_ref, counts, ref_totals);
    RV_LAUNCH_CHECK(fn);
    return RV_OK;
}

extern "C" {

// Bytes of device scratch that rv_eval_decode and rv_eval_frame_counts need for rolls of T frames (either call; 0 for a bad T).
long rv_eval_workspace_bytes(long T) { return eval_workspace_bytes(T); }

// onsets, frames: [T, 88] float32 (16-byte aligned, may alias).  rule: 1 = rule1, 2 = rule2.  notes: [max_notes, 3] int32 rows
// (t, pitch, end) in (t, pitch) order; *count (device) receives the number of notes the rolls hold -- rows past max_notes are not
// written, so count > max_notes tells the caller its buffer was too small (88 * ceil(T / 2) always suffices).  painted: [T, 88]
// uint8 (4-byte aligned) = the roll of the notes.
// min_frames, bridge_gap: the note clean-up, as include/reconvat_hip.h states it; (1, 0) is rv_eval_decode.
int rv_eval_decode_clean(const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold, int rule,
                         int min_frames, int bridge_gap, int* notes, long max_notes, int* count, unsigned char* painted, void* workspace,
                         long workspace_bytes, void* stream) {
    return eval_decode("rv_eval_decode_clean", onsets, frames, T, onset_threshold, frame_threshold, rule, min_frames, bridge_gap, notes,
                       max_notes, count, painted, workspace, workspace_bytes, stream);
}

// rv_eval_decode_clean without clean-up: min_frames = 1, bridge_gap = 0.
int rv_eval_decode(const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold, int rule, int* notes,
                   long max_notes, int* count, unsigned char* painted, void* workspace, long workspace_bytes, void* stream) {
    return eval_decode("rv_eval_decode", onsets, frames, T, onset_threshold, frame_threshold, rule, 1, 0, notes, max_notes, count, painted,
                       workspace, workspace_bytes, stream);
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

// Bytes of device scratch that rv_eval_sweep needs for rolls of T frames and an n_on x n_fr grid (0 for arguments out of range).
long rv_eval_sweep_workspace_bytes(long T, int n_on, int n_fr) { return eval_sweep_workspace_bytes(T, n_on, n_fr); }

// onsets, frames: [T, 88] float32 (16-byte aligned, may alias).  onset_thresholds [n_on], frame_thresholds [n_fr]: float32 on the
// device, any order, duplicates allowed.  ref_notes: [n_ref, 5] int32 rows (t, pitch, end, early, late) sorted by (pitch, t) -- the
// notes rv_eval_decode finds in the labels, and how many frames an estimate may end before / after `end` and still pass the offset
// test; n_ref may be 0.  ref_roll: [T, 88] uint8 (4-byte aligned), the painted roll of those notes.  counts: [n_on][n_fr][5] int64
// (notes, matched on onset and pitch, matched on onset, pitch and offset, frames painted on both sides, frames painted by the
// estimate); ref_totals: 2 int64 (n_ref, frames painted by the reference).
// min_frames, bridge_gap: the note clean-up of the ESTIMATE, as include/reconvat_hip.h states it; (1, 0) is rv_eval_sweep.
int rv_eval_sweep_clean(const float* onsets, const float* frames, long T, const float* onset_thresholds, int n_on,
                        const float* frame_thresholds, int n_fr, int rule, int min_frames, int bridge_gap, const int* ref_notes, long n_ref,
                        const unsigned char* ref_roll, long* counts, long* ref_totals, void* workspace, long workspace_bytes,
                        void* stream) {
    return eval_sweep("rv_eval_sweep_clean", onsets, frames, T, onset_thresholds, n_on, frame_thresholds, n_fr, rule, min_frames,
                      bridge_gap, ref_notes, n_ref, ref_roll, counts, ref_totals, workspace, workspace_bytes, stream);
}

// rv_eval_sweep_clean without clean-up: min_frames = 1, bridge_gap = 0.
int rv_eval_sweep(const float* onsets, const float* frames, long T, const float* onset_thresholds, int n_on,
                  const float* frame_thresholds, int n_fr, int rule, const int* ref_notes, long n_ref, const unsigned char* ref_roll,
                  long* counts, long* ref_totals, void* workspace, long workspace_bytes, void* stream) {
    return eval_sweep("rv_eval_sweep", onsets, frames, T, onset_thresholds, n_on, frame_thresholds, n_fr, rule, 1, 0, ref_notes, n_ref,
                      ref_roll, counts, ref_totals, workspace, workspace_bytes, stream);
}

}  // extern "C"
