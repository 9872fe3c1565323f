// Note velocities: a head that shares its weights across the 88 keys, on the spectrogram bins nearest to the first eight
// harmonics of a key over four frames.  reconvat_amd/velocity.py has the definition; in short, for the cell (b, t, p)
//     x[8 j + k] = spec[b][clamp(t - 1 + j, 0, T - 1)][tab[p][k]]  (0 where tab[p][k] = -1), j = 0..3, k = 0..7;    x[32] = p / 88
//     v          = sigmoid(b2 + sum_h w2[h] sigmoid(b1[h] + sum_i w1[h][i] x[i]))
// with the 1121 parameters packed as w1 [32][33], b1 [32], w2 [32], b2.
//
// The table comes from the HOST: the entry points check every entry against n_bins and hand it to the kernels by value (704 int16 in
// the kernel arguments), so no kernel indexes the spectrogram with a number it read from device memory.
//
// vel_roll_k       one workgroup = VEL_TILE = 32 frames of one clip, 256 work items.  It stages the parameters (w1 rows padded to 36
//                  floats: 16-byte broadcast reads), the table and its 35 spectrogram rows in LDS once; the rows have an ODD stride
//                  (n_bins | 1).  A half wave is the 32 frames of one key, so the 32 lanes of a ds_read_b32 group gather the same
//                  bin of 32 consecutive rows: 32 different banks for any bin.  Weights are the same address in every lane.  The
//                  88 x 32 results go through an LDS tile (stride 89) and leave as one contiguous run.  LDS: 51 KB at 229 bins, three
//                  workgroups per CU; the ten-minute spectrogram is 586 workgroups, a training batch of 8 x 640 frames 160.
// vel_loss_k       the same tile.  The mask of the tile is read first and the cells with m != 0 are compacted into an LDS list by
//                  ballot, in cell order; a tile without any writes zeros and is done -- onset cells are one in a thousand.
//                  Otherwise the tile is staged as above and the list is worked off in chunks of 64 cells: one work item per
//                  cell runs the head forward and leaves x [33], dz1 [32] = d2 w2 sigmoid'(z1), d2 a [32], d2 = 2 m (v - target)
//                  sigmoid'(z2), m (v - target)^2 and m in LDS (cell stride 33: conflict-free); then every work item owns up to
//                  five of the 1123 outputs -- the [32 x cells] . [cells x 33] product, the three vectors and the two sums -- and adds
//                  its cells in list order.  sigmoid'(z) = e / (1 + e)^2 with e = exp(-|z|): no 1 - v cancellation when saturated.
// vel_fold_k       adds the per-workgroup partials in float64 in workgroup order and divides by sum m (0 and zero gradient if 0).
// vel_note_k       one work item per note row: the float64 mean, in ascending frames, of the velocity roll over the note's
//                  onset-active frames, rounded to float32 once.
// Plain and vector stores only, no atomics: the same bits on every run.
#include "common.h"

#define VEL_KEYS 88
#define VEL_HARM 8
#define VEL_CTX 4
#define VEL_IN 33
#define VEL_HID 32
#define VEL_W1 (VEL_HID * VEL_IN)
#define VEL_PARAMS (VEL_W1 + 2 * VEL_HID + 1)
#define VEL_TILE 32
#define VEL_ROWS (VEL_TILE + VEL_CTX - 1)
#define VEL_W1LD 36
#define VEL_PARAM_LDS (VEL_HID * VEL_W1LD + 2 * VEL_HID + 4)
#define VEL_OUT_LD 89
#define VEL_MAX_BINS 384
#define VEL_THREADS 256
#define VEL_CELLS (VEL_TILE * VEL_KEYS)                      // 2816 = 11 * 256
#define VEL_ROUNDS (VEL_CELLS / VEL_THREADS)
#define VEL_CHUNK 64
#define VEL_CELL_LD 33
#define VEL_OUTPUTS (VEL_PARAMS + 2)                         // gradient, sum m (v - target)^2, sum m
#define VEL_PART_LD 1124
#define VEL_OWN ((VEL_OUTPUTS + VEL_THREADS - 1) / VEL_THREADS)

struct VelTable {
    short bin[VEL_KEYS * VEL_HARM];
};

struct VelArgs {
    const float* spec;
    const float* params;
    const float* target;
    const float* mask;
    float* out;              // the roll, or the per-workgroup partials
    int T, n_bins;
    VelTable tab;
};

__device__ __forceinline__ float vel_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float vel_dsigmoid(float z) {
    const float e = expf(-fabsf(z));
    const float d = 1.0f + e;
    return e / (d * d);
}

// LDS image shared by both kernels: parameters, table, spectrogram rows
struct VelLds {
    float* w1;               // [32][36]
    float* b1;
    float* w2;
    float* b2;
    int* tab;                // [88][8]
    float* rows;             // [35][stride]
    int stride;
};

__device__ __forceinline__ VelLds vel_carve(float* base, int n_bins) {
    VelLds l;
    l.w1 = base;
    l.b1 = base + VEL_HID * VEL_W1LD;
    l.w2 = l.b1 + VEL_HID;
    l.b2 = l.w2 + VEL_HID;
    l.tab = (int*)(base + VEL_PARAM_LDS);
    l.rows = base + VEL_PARAM_LDS + VEL_KEYS * VEL_HARM;
    l.stride = n_bins | 1;
    return l;
}

__device__ __forceinline__ void vel_stage(const VelLds& l, const VelArgs& g, int b, int t0) {
    const int tid = threadIdx.x;
    for (int i = tid; i < VEL_HID * VEL_W1LD; i += VEL_THREADS) {
        const int h = i / VEL_W1LD, c = i - h * VEL_W1LD;
        l.w1[i] = c < VEL_IN ? g.params[h * VEL_IN + c] : 0.0f;
    }
    if (tid < 2 * VEL_HID + 1) l.b1[tid] = g.params[VEL_W1 + tid];               // b1, w2, b2 are contiguous in both images
    for (int i = tid; i < VEL_KEYS * VEL_HARM; i += VEL_THREADS) l.tab[i] = g.tab.bin[i];
    const int lane = tid & 63, wave = tid >> 6;
    const float* clip = g.spec + (long)b * g.T * g.n_bins;
    for (int r = wave; r < VEL_ROWS; r += VEL_THREADS / 64) {
        const int t = min(max(t0 - 1 + r, 0), g.T - 1);
        const float* src = clip + (long)t * g.n_bins;
        for (int c = lane; c < g.n_bins; c += 64) l.rows[r * l.stride + c] = src[c];
    }
}

// the features of the cell (tile frame f, key p)
__device__ __forceinline__ void vel_gather(const VelLds& l, int f, int p, float* x) {
#pragma unroll
    for (int k = 0; k < VEL_HARM; ++k) {
        const int bin = l.tab[p * VEL_HARM + k];
#pragma unroll
        for (int j = 0; j < VEL_CTX; ++j) x[VEL_HARM * j + k] = bin >= 0 ? l.rows[(f + j) * l.stride + bin] : 0.0f;
    }
    x[VEL_IN - 1] = (float)p / (float)VEL_KEYS;
}

__device__ __forceinline__ float vel_hidden(const VelLds& l, int h, const float* x) {
    const f32x4* w = (const f32x4*)(l.w1 + h * VEL_W1LD);
    float acc = l.b1[h];
#pragma unroll
    for (int q = 0; q < (VEL_IN - 1) / 4; ++q) {
        const f32x4 v = w[q];
        acc = fmaf(v.x, x[4 * q], acc);
        acc = fmaf(v.y, x[4 * q + 1], acc);
        acc = fmaf(v.z, x[4 * q + 2], acc);
        acc = fmaf(v.w, x[4 * q + 3], acc);
    }
    return fmaf(l.w1[h * VEL_W1LD + VEL_IN - 1], x[VEL_IN - 1], acc);
}

__global__ __launch_bounds__(VEL_THREADS) void vel_roll_k(VelArgs g) {
    extern __shared__ __attribute__((aligned(16))) float vel_lds[];
    const VelLds l = vel_carve(vel_lds, g.n_bins);
    float* tile = l.rows + VEL_ROWS * l.stride;                                  // [32][89]
    const int b = blockIdx.y, t0 = (int)blockIdx.x * VEL_TILE;
    vel_stage(l, g, b, t0);
    __syncthreads();
    const int tid = threadIdx.x, f = tid & 31, sub = tid >> 5;                    // 8 half waves: 8 keys a round
    const float b2 = l.b2[0];
    for (int p = sub; p < VEL_KEYS; p += VEL_THREADS / 32) {
        float x[VEL_IN];
        vel_gather(l, f, p, x);
        float z2 = b2;
        for (int h = 0; h < VEL_HID; ++h) z2 = fmaf(l.w2[h], vel_sigmoid(vel_hidden(l, h, x)), z2);
        tile[f * VEL_OUT_LD + p] = vel_sigmoid(z2);
    }
    __syncthreads();
    const int n = min(VEL_TILE, g.T - t0) * VEL_KEYS;
    float* dst = g.out + ((long)b * g.T + t0) * VEL_KEYS;
    for (int i = tid; i < n; i += VEL_THREADS) {
        const int fr = i / VEL_KEYS;
        dst[i] = tile[fr * VEL_OUT_LD + (i - fr * VEL_KEYS)];
    }
}

__global__ __launch_bounds__(VEL_THREADS) void vel_loss_k(VelArgs g) {
    extern __shared__ __attribute__((aligned(16))) float vel_lds[];
    const VelLds l = vel_carve(vel_lds, g.n_bins);
    float* xs = l.rows + VEL_ROWS * l.stride;                                    // [64][33] features
    float* ds = xs + VEL_CHUNK * VEL_CELL_LD;                                    // [64][33] dz1
    float* es = ds + VEL_CHUNK * VEL_CELL_LD;                                    // [64][33] d2 a
    float* tail = es + VEL_CHUNK * VEL_CELL_LD;                                  // [3][64]  d2, m r^2, m
    int* wcount = (int*)(tail + 3 * VEL_CHUNK);                                  // [4] + total
    unsigned short* list = (unsigned short*)(wcount + 8);                        // [2816]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = (int)blockIdx.x * VEL_TILE;
    const int wg = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const int n_valid = min(VEL_TILE, g.T - t0) * VEL_KEYS;
    const long cell0 = ((long)b * g.T + t0) * VEL_KEYS;
    float* part = g.out + (long)wg * VEL_PART_LD;

    // the masked cells of the tile, in cell order
    float mv[VEL_ROUNDS];
#pragma unroll
    for (int r = 0; r < VEL_ROUNDS; ++r) {
        const int i = r * VEL_THREADS + tid;
        mv[r] = i < n_valid ? g.mask[cell0 + i] : 0.0f;
    }
    int n_list = 0;
#pragma unroll
    for (int r = 0; r < VEL_ROUNDS; ++r) {
        const bool on = mv[r] != 0.0f;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int before = n_list;
        for (int w = 0; w < wave; ++w) before += wcount[w];
        if (on) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)(r * VEL_THREADS + tid);
        n_list += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    float acc[VEL_OWN];
#pragma unroll
    for (int q = 0; q < VEL_OWN; ++q) acc[q] = 0.0f;
    if (n_list > 0) {                                                            // (the same for the whole workgroup)
        vel_stage(l, g, b, t0);
        __syncthreads();
        for (int c0 = 0; c0 < n_list; c0 += VEL_CHUNK) {
            const int nc = min(VEL_CHUNK, n_list - c0);
            if (tid < nc) {
                const int i = list[c0 + tid];
                const int f = i / VEL_KEYS, p = i - f * VEL_KEYS;
                float x[VEL_IN];
                vel_gather(l, f, p, x);
                float* xc = xs + tid * VEL_CELL_LD;
                float* dc = ds + tid * VEL_CELL_LD;
                float* ec = es + tid * VEL_CELL_LD;
#pragma unroll
                for (int k = 0; k < VEL_IN; ++k) xc[k] = x[k];
                float z2 = l.b2[0];
                for (int h = 0; h < VEL_HID; ++h) {
                    const float z1 = vel_hidden(l, h, x);
                    const float a = vel_sigmoid(z1);
                    const float w2 = l.w2[h];
                    z2 = fmaf(w2, a, z2);
                    ec[h] = a;
                    dc[h] = w2 * vel_dsigmoid(z1);
                }
                const float m = g.mask[cell0 + i];
                const float r = vel_sigmoid(z2) - g.target[cell0 + i];
                const float d2 = 2.0f * m * r * vel_dsigmoid(z2);
                for (int h = 0; h < VEL_HID; ++h) {
                    ec[h] *= d2;
                    dc[h] *= d2;
                }
                tail[tid] = d2;
                tail[VEL_CHUNK + tid] = m * r * r;
                tail[2 * VEL_CHUNK + tid] = m;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < VEL_OWN; ++q) {
                const int o = q * VEL_THREADS + tid;
                float s = acc[q];
                if (o < VEL_W1) {
                    const int h = o / VEL_IN, i = o - h * VEL_IN;
                    for (int c = 0; c < nc; ++c) s = fmaf(ds[c * VEL_CELL_LD + h], xs[c * VEL_CELL_LD + i], s);
                } else if (o < VEL_OUTPUTS) {
                    const float* src;
                    int ld = VEL_CELL_LD;
                    if (o < VEL_W1 + VEL_HID) src = ds + (o - VEL_W1);
                    else if (o < VEL_W1 + 2 * VEL_HID) src = es + (o - VEL_W1 - VEL_HID);
                    else { src = tail + (o - (VEL_PARAMS - 1)) * VEL_CHUNK; ld = 1; }
                    for (int c = 0; c < nc; ++c) s += src[c * ld];
                }
                acc[q] = s;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < VEL_OWN; ++q) {
        const int o = q * VEL_THREADS + tid;
        if (o < VEL_OUTPUTS) part[o] = acc[q];
    }
}

__global__ __launch_bounds__(VEL_THREADS) void vel_fold_k(const float* part, int n_wg, float* loss, float* grad) {
    const int o = (int)(blockIdx.x * VEL_THREADS + threadIdx.x);
    if (o > VEL_PARAMS) return;                                                  // 0..1120 the gradient, 1121 the loss
    double s = 0.0, m = 0.0;
    for (int w = 0; w < n_wg; ++w) {
        s += (double)part[(long)w * VEL_PART_LD + o];
        m += (double)part[(long)w * VEL_PART_LD + VEL_PARAMS + 1];
    }
    const float v = m == 0.0 ? 0.0f : (float)(s / m);
    if (o < VEL_PARAMS) grad[o] = v;
    else loss[0] = v;
}

__global__ __launch_bounds__(VEL_THREADS) void vel_note_k(const float* onsets, const float* velocity, int T, float threshold,
                                                           const int* notes, int n, float* out) {
    const int i = (int)(blockIdx.x * VEL_THREADS + threadIdx.x);
    if (i >= n) return;
    const int t = notes[3 * i], p = notes[3 * i + 1], e = min(notes[3 * i + 2], T);
    double s = 0.0;
    int c = 0;
    if (p >= 0 && p < VEL_KEYS && t >= 0)
        for (int f = t; f < e; ++f)
            if (onsets[(long)f * VEL_KEYS + p] > threshold) {
                s += (double)velocity[(long)f * VEL_KEYS + p];
                ++c;
            }
    out[i] = c ? (float)(s / (double)c) : 0.0f;
}

static inline bool vel_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

static int vel_check(const char* name, const float* spec, long n_spec, int B, int T, int n_bins, const int* table, const float* params,
                     long n_params, VelTable* tab) {
    RV_CHECK_ARG(spec && table && params, "%s: null pointer", name);
    RV_CHECK_ARG(vel_aligned(spec) && vel_aligned(params), "%s: spec and params must be 4-byte aligned", name);
    RV_CHECK_ARG(B >= 1 && B <= 65535, "%s: batch %d outside [1, 65535]", name, B);
    RV_CHECK_ARG(T >= 1 && T <= (1 << 24), "%s: %d frames outside [1, 2^24]", name, T);
    RV_CHECK_ARG(n_bins >= 1 && n_bins <= VEL_MAX_BINS, "%s: %d bins outside [1, %d]", name, n_bins, VEL_MAX_BINS);
    RV_CHECK_ARG(n_spec >= (long)B * T * n_bins, "%s: spec holds %ld floats, %ld needed", name, n_spec, (long)B * T * n_bins);
    RV_CHECK_ARG(n_params >= VEL_PARAMS, "%s: params holds %ld floats, %d needed", name, n_params, VEL_PARAMS);
    for (int i = 0; i < VEL_KEYS * VEL_HARM; ++i) {
        RV_CHECK_ARG(table[i] >= -1 && table[i] < n_bins, "%s: table entry %d is %d, outside [-1, %d)", name, i, table[i], n_bins);
        tab->bin[i] = (short)table[i];
    }
    return RV_OK;
}

// more than 64 KB of LDS needs the kernel's consent; the attribute belongs to the device the launch goes to, so it is set on every
// such call (a host-side setting, no launch) and nothing is remembered between calls, devices or threads
static int vel_grant(const char* name, const void* fn, int lds, int lds_max) {
    if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
        (void)hipGetLastError();
        rv_set_error("%s: the device refused %d bytes of LDS per workgroup", name, lds);
        return RV_EUNSUPPORTED;
    }
    return RV_OK;
}

static inline int vel_common_floats(int n_bins) { return VEL_PARAM_LDS + VEL_KEYS * VEL_HARM + VEL_ROWS * (n_bins | 1); }
static inline int vel_roll_lds(int n_bins) { return (vel_common_floats(n_bins) + VEL_TILE * VEL_OUT_LD) * 4; }
static inline int vel_loss_lds(int n_bins) {
    return (vel_common_floats(n_bins) + 3 * VEL_CHUNK * VEL_CELL_LD + 3 * VEL_CHUNK + 8) * 4 + VEL_CELLS * 2;
}

extern "C" {

int rv_velocity_roll(const float* spec, long n_spec, int B, int T, int n_bins, const int* table, const float* params, long n_params,
                     float* out, long n_out, void* stream) {
    VelArgs g;
    const int rc = vel_check("rv_velocity_roll", spec, n_spec, B, T, n_bins, table, params, n_params, &g.tab);
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(out && vel_aligned(out), "rv_velocity_roll: out is null or not 4-byte aligned");
    RV_CHECK_ARG(n_out >= (long)B * T * VEL_KEYS, "rv_velocity_roll: out holds %ld floats, %ld needed", n_out, (long)B * T * VEL_KEYS);
    g.spec = spec; g.params = params; g.target = nullptr; g.mask = nullptr; g.out = out; g.T = T; g.n_bins = n_bins;
    const int lds = vel_roll_lds(n_bins);
    const int rg = vel_grant("rv_velocity_roll", (const void*)vel_roll_k, lds, vel_roll_lds(VEL_MAX_BINS));
    if (rg != RV_OK) return rg;
    hipLaunchKernelGGL(vel_roll_k, dim3((unsigned)cdiv(T, VEL_TILE), (unsigned)B), dim3(VEL_THREADS), (size_t)lds, (hipStream_t)stream, g);
    RV_LAUNCH_CHECK("rv_velocity_roll");
    return RV_OK;
}

long rv_velocity_workspace_bytes(int B, int T) {
    if (B < 1 || B > 65535 || T < 1 || T > (1 << 24)) return 0;
    return (long)B * cdiv(T, VEL_TILE) * VEL_PART_LD * (long)sizeof(float);
}

int rv_velocity_loss_grad(const float* spec, long n_spec, int B, int T, int n_bins, const int* table, const float* params, long n_params,
                          const float* target, const float* mask, long n_cells, float* loss, float* grad, long n_grad, void* workspace,
                          long workspace_bytes, void* stream) {
    VelArgs g;
    const int rc = vel_check("rv_velocity_loss_grad", spec, n_spec, B, T, n_bins, table, params, n_params, &g.tab);
    if (rc != RV_OK) return rc;
    RV_CHECK_ARG(target && mask && loss && grad && workspace, "rv_velocity_loss_grad: null pointer");
    RV_CHECK_ARG(vel_aligned(target) && vel_aligned(mask) && vel_aligned(loss) && vel_aligned(grad) && vel_aligned(workspace),
                 "rv_velocity_loss_grad: every buffer must be 4-byte aligned");
    RV_CHECK_ARG(n_cells >= (long)B * T * VEL_KEYS, "rv_velocity_loss_grad: target and mask hold %ld floats, %ld needed", n_cells,
                 (long)B * T * VEL_KEYS);
    RV_CHECK_ARG(n_grad >= VEL_PARAMS, "rv_velocity_loss_grad: grad holds %ld floats, %d needed", n_grad, VEL_PARAMS);
    RV_CHECK_ARG(workspace_bytes >= rv_velocity_workspace_bytes(B, T), "rv_velocity_loss_grad: workspace of %ld bytes, %ld needed",
                 workspace_bytes, rv_velocity_workspace_bytes(B, T));
    const long n_wg = (long)B * cdiv(T, VEL_TILE);
    RV_CHECK_ARG(n_wg < (1L << 31), "rv_velocity_loss_grad: %ld tiles", n_wg);
    g.spec = spec; g.params = params; g.target = target; g.mask = mask; g.out = (float*)workspace; g.T = T; g.n_bins = n_bins;
    const int lds = vel_loss_lds(n_bins);
    const int rg = vel_grant("rv_velocity_loss_grad", (const void*)vel_loss_k, lds, vel_loss_lds(VEL_MAX_BINS));
    if (rg != RV_OK) return rg;
    hipLaunchKernelGGL(vel_loss_k, dim3((unsigned)cdiv(T, VEL_TILE), (unsigned)B), dim3(VEL_THREADS), (size_t)lds, (hipStream_t)stream, g);
    RV_LAUNCH_CHECK("rv_velocity_loss_grad");
    hipLaunchKernelGGL(vel_fold_k, dim3((unsigned)cdiv(VEL_PARAMS + 1, VEL_THREADS)), dim3(VEL_THREADS), 0, (hipStream_t)stream,
                       (const float*)workspace, (int)n_wg, loss, grad);
    RV_LAUNCH_CHECK("rv_velocity_loss_grad");
    return RV_OK;
}

int rv_eval_note_velocity(const float* onsets, const float* velocity, long T, float onset_threshold, const int* notes, long n, float* out,
                          long n_out, void* stream) {
    RV_CHECK_ARG(n >= 0 && n < (1L << 30), "rv_eval_note_velocity: %ld notes", n);
    RV_CHECK_ARG(T >= 1 && T <= (1 << 24), "rv_eval_note_velocity: %ld frames outside [1, 2^24]", T);
    RV_CHECK_ARG(n_out >= n, "rv_eval_note_velocity: out holds %ld floats, %ld needed", n_out, n);
    if (n == 0) return RV_OK;
    RV_CHECK_ARG(onsets && velocity && notes && out, "rv_eval_note_velocity: null pointer");
    RV_CHECK_ARG(vel_aligned(onsets) && vel_aligned(velocity) && vel_aligned(notes) && vel_aligned(out),
                 "rv_eval_note_velocity: every buffer must be 4-byte aligned");
    hipLaunchKernelGGL(vel_note_k, dim3((unsigned)cdiv(n, VEL_THREADS)), dim3(VEL_THREADS), 0, (hipStream_t)stream, onsets, velocity, (int)T,
                       onset_threshold, notes, (int)n, out);
    RV_LAUNCH_CHECK("rv_eval_note_velocity");
    return RV_OK;
}

}  // extern "C"
