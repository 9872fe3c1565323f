// VAT perturbation primitives, losses, optimiser and small reductions for gfx950.
// All HBM-bound: one pass per tensor, wavefront (64-lane) reductions over the 229-/88-wide rows.
//
// Reference anchors:
//   _l2_normalize / r = XI*d/||d|| / clamp(0,1) ......... model/UNet_onset.py:130-131,145-151,165-171
//   F.binary_cross_entropy (soft targets, log clamp -100) .. model/UNet_onset.py:136-137,157-158,473-476
//   F.mse_loss ............................................ model/UNet_onset.py:472
//   Adam + StepLR ......................................... train_UNet_Onset_VAT.py:113,124
#include "common.h"

// ---------------------------------------------------------------------------------------------
// VAT: x_adv = clamp(x + scale * (prescale*d) / ||prescale*d||_row, 0, 1)
// ---------------------------------------------------------------------------------------------
struct PerturbArgs {
    const float* x; const float* d; const float* g;   // g: grad wrt x_adv (bwd only)
    float* x_adv; float* r_out; float* dn_out; float* gd;
    long rows; int n;
    float prescale, scale;
    int* nan_flag;
};

template <bool BWD>
__global__ __launch_bounds__(256) void vat_perturb_k(PerturbArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const float* d = a.d + row * a.n;
    const float* x = a.x + row * a.n;
    float ss = 0.f;
    for (int i = lane; i < a.n; i += 64) { float v = d[i] * a.prescale; ss = fmaf(v, v, ss); }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float inv = 1.0f / nrm;        // 0/0 -> NaN exactly like the reference (no epsilon)
    if (!BWD) {
        bool bad = false;
        for (int i = lane; i < a.n; i += 64) {
            float dn = (d[i] * a.prescale) / nrm;
            float r = a.scale * dn;
            bad |= (r != r);
            float xa = x[i] + r;
            xa = fminf(fmaxf(xa, 0.f), 1.f);
            a.x_adv[row * a.n + i] = xa;
            if (a.r_out) a.r_out[row * a.n + i] = r;
            if (a.dn_out) a.dn_out[row * a.n + i] = dn;
        }
        if (a.nan_flag && __any(bad) && lane == 0) atomicOr(a.nan_flag, 1);
    } else {
        const float* g = a.g + row * a.n;
        float dot = 0.f;
        for (int i = lane; i < a.n; i += 64) {
            float dn = (d[i] * a.prescale) / nrm;
            float xa = x[i] + a.scale * dn;
            float gr = (xa >= 0.f && xa <= 1.f) ? g[i] * a.scale : 0.f;
            dot = fmaf(dn, gr, dot);
        }
        dot = wave_sum(dot);
        for (int i = lane; i < a.n; i += 64) {
            float dn = (d[i] * a.prescale) / nrm;
            float xa = x[i] + a.scale * dn;
            float gr = (xa >= 0.f && xa <= 1.f) ? g[i] * a.scale : 0.f;
            a.gd[row * a.n + i] = (gr - dn * dot) * inv * a.prescale;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// mean-reduced losses: two-stage deterministic reduction (per-block partials, fp64 fold)
// ---------------------------------------------------------------------------------------------
enum { RED_BCE = 0, RED_MSE = 1, RED_ABS = 2, RED_SUMSQ = 3 };

template <int KIND>
__device__ __forceinline__ float red_term(float p, float t) {
    if (KIND == RED_BCE) {
        float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);   // torch clamps log at -100
        return -(t * lp + (1.f - t) * lq);
    } else if (KIND == RED_MSE) {
        float e = p - t;
        return e * e;
    } else if (KIND == RED_ABS) {
        return fabsf(p);
    } else {
        return p * p;
    }
}

// ticket (nullable): a zeroed device word.  With it the LAST workgroup to finish also does the final fold (fixed order, so
// the result does not depend on which workgroup that is) and re-zeroes the ticket: one launch per loss instead of two.
template <int KIND>
__global__ __launch_bounds__(256) void reduce_partial_k(const float* p, const float* t, long n, float* part, unsigned* ticket,
                                                        double denom, float* out, int sqrt_out) {
    __shared__ float sh[4];
    __shared__ double shd[4];
    __shared__ bool last;
    float s = 0.f;
    const long base = (long)blockIdx.x * 2048;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        long i = base + k * 256 + threadIdx.x;
        if (i < n) s += red_term<KIND>(p[i], (KIND == RED_BCE || KIND == RED_MSE) ? t[i] : 0.f);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if (!ticket) return;
    if (threadIdx.x == 0) {
        __threadfence();                                      // the partial is visible before the ticket is taken
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double d = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) d += (double)__hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    d = wave_sum_d(d);
    if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double v = ((shd[0] + shd[1]) + (shd[2] + shd[3])) / denom;
        *out = (float)(sqrt_out ? sqrt(v) : v);
        *ticket = 0u;
    }
}

__global__ __launch_bounds__(256) void reduce_final_k(const float* part, int nparts, double denom, float* out, int sqrt_out) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += (double)part[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = ((sh[0] + sh[1]) + (sh[2] + sh[3])) / denom;
        *out = (float)(sqrt_out ? sqrt(v) : v);
    }
}

// grad of the mean-reduced loss wrt its first argument, times the upstream scalar *gout
template <int KIND>
__global__ __launch_bounds__(256) void loss_bwd_k(const float* p, const float* t, long n, const float* gout, float* gp) {
    const float go = *gout / (float)n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float g;
        if (KIND == RED_BCE) g = (p[i] - t[i]) / fmaxf((1.f - p[i]) * p[i], 1e-12f);   // torch's BCE backward
        else g = 2.f * (p[i] - t[i]);
        gp[i] = g * go;
    }
}

// ---------------------------------------------------------------------------------------------
// sigmoid backward with up to two upstream gradients (strided): dz = (g1 + g2) * y * (1 - y)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sigmoid_bwd_k(const float* g1, int ld1, const float* g2, int ld2, const float* y,
                                                     int ldy, float* dz, int ldz, long M, int N) {
    const long total = M * N;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long m = i / N; int n = (int)(i - m * N);
        float g = 0.f;
        if (g1) g += g1[m * ld1 + n];
        if (g2) g += g2[m * ld2 + n];
        float yy = y[m * ldy + n];
        dz[m * ldz + n] = g * yy * (1.f - yy);
    }
}

// column sums of a [M, N] matrix (bias gradients): out[n] (+)= sum_m x[m*ld + n]
// generic version: 64 columns x 4 row lanes per workgroup
__global__ __launch_bounds__(256) void colsum_k(const float* x, int ld, long M, int N, float* out, int rows_per_block) {
    __shared__ float sh[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(r0 + rows_per_block, M);
    float s = 0.f;
    if (col < N)
        for (long r = r0 + rl; r < r1; r += 4) s += x[r * ld + col];
    sh[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && col < N) atomicAdd(&out[col], (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]));
}

// narrow matrices (N % 4 == 0, N <= 256; the up-conv bias gradients over millions of pixels): 16-byte loads,
// thread -> (column quad, row lane), 32 rows per thread, LDS fold, one atomic per column per workgroup
__global__ __launch_bounds__(256) void colsum_vec_k(const float* x, int ld, long M, int N, float* out, int rpt) {
    __shared__ float sh[256 * 4];
    const int C4 = N >> 2, PL = 256 / C4;
    const int t = threadIdx.x;
    const int c = (t % C4) * 4, pl = t / C4;
    f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        const long p0 = (long)blockIdx.x * PL * rpt;
#pragma unroll 4
        for (int k = 0; k < rpt; ++k) {
            const long p = p0 + pl + (long)k * PL;
            if (p >= M) break;
            s += *reinterpret_cast<const f32x4*>(x + p * ld + c);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[pl * N + c + q] = s[q];
    }
    __syncthreads();
    if (t < N) {
        float d = 0.f;
        for (int l = 0; l < PL; ++l) d += sh[l * N + t];
        atomicAdd(&out[t], d);
    }
}

// ---------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults) + StepLR on one flat parameter buffer
// ---------------------------------------------------------------------------------------------
struct AdamArgs {
    float* p; const float* g; float* m; float* v; long n;
    const long* step;      // number of optimiser steps already taken (device scalar)
    float lr0, decay_rate; long decay_steps;
    float b1, b2, eps, grad_scale;
    const int* skip;       // nullable: a non-zero word means "this step's gradients are invalid" -> leave p, m, v untouched
};

__global__ __launch_bounds__(256) void adam_k(AdamArgs a) {
    if (a.skip && *a.skip != 0) return;
    const long step = *a.step;
    const double t = (double)(step + 1);
    const float lr = a.lr0 * (float)pow((double)a.decay_rate, (double)(step / a.decay_steps));
    const float bc1 = (float)(1.0 - pow((double)a.b1, t));
    const float bc2s = (float)sqrt(1.0 - pow((double)a.b2, t));
    const float step_size = lr / bc1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        float g = a.g[i] * a.grad_scale;
        float m = a.m[i] * a.b1 + (1.f - a.b1) * g;
        float v = a.v[i] * a.b2 + (1.f - a.b2) * g * g;
        a.m[i] = m; a.v[i] = v;
        float denom = sqrtf(v) / bc2s + a.eps;
        a.p[i] -= step_size * (m / denom);
    }
}

__global__ void counter_add_k(long* c, long inc, const int* skip) { if (!skip || *skip == 0) *c += inc; }

__global__ __launch_bounds__(256) void scale_by_clip_k(float* g, long n, const float* total_norm, float max_norm) {
    // torch.nn.utils.clip_grad_norm_: coef = clamp(max_norm / (total_norm + 1e-6), max=1)
    float coef = fminf(max_norm / (*total_norm + 1e-6f), 1.0f);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] *= coef;
}

// (restated in tests/stream_cases.py: grid_for)
static int grid_for(long n) { long b = (n + 255) / 256; return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096); }

// ---------------------------------------------------------------------------------------------
// AdamW + StepLR with the optimiser options: clip_grad_norm_ BEFORE the update, decoupled weight decay, an exponential
// moving average of the weights -- all in the one pass over the flat bucket.  adam_k above is the default path and stays as it is.
// ---------------------------------------------------------------------------------------------
struct AdamWArgs {
    AdamArgs a;
    float weight_decay, max_grad_norm;
    const float* total_norm;   // nullable: L2 norm of the bucket as stored (before grad_scale)
    float* ema;                // nullable
    float ema_decay;
    long i0;                   // scalar kernel: first element
};

struct AdamWCoef { float gmul, step_size, bc2s, keep; };

// lr / bc1 / bc2s / step_size: adam_k's expressions, character for character
__device__ __forceinline__ AdamWCoef adamw_coef(const AdamWArgs& w) {
#pragma clang fp contract(off)
    const AdamArgs& a = w.a;
    const long step = *a.step;
    const double t = (double)(step + 1);
    const float lr = a.lr0 * (float)pow((double)a.decay_rate, (double)(step / a.decay_steps));
    const float bc1 = (float)(1.0 - pow((double)a.b1, t));
    const float bc2s = (float)sqrt(1.0 - pow((double)a.b2, t));
    AdamWCoef c;
    c.step_size = lr / bc1;
    c.bc2s = bc2s;
    // torch.nn.utils.clip_grad_norm_ on the SCALED gradient: coef = clamp(max_norm / (total_norm + 1e-6), max=1)
    c.gmul = 1.f;
    if (w.max_grad_norm > 0.f && w.total_norm) c.gmul = fminf(w.max_grad_norm / (*w.total_norm * a.grad_scale + 1e-6f), 1.f);
    c.keep = 1.f - lr * w.weight_decay;
    return c;
}

// One element.  Contraction is OFF and the two fused multiply-adds are the ones the compiler forms in adam_k (v, and the update of
// p): with weight_decay = 0, max_grad_norm = 0 the only extra operations are g * 1.f and p * 1.f, so p, m, v equal adam_k's bit for
// bit (tests/test_optim_options_gpu.py holds the two kernels against each other).
// Element rule: g == 0 with zero moments keeps p (no decay) -- torch skips tensors whose .grad is None, and the pad elements and
// never-touched tensors of the flat bucket are exactly these elements.  It deviates from torch.optim.AdamW only for an element of a
// TOUCHED tensor whose gradient has been exactly zero since step 1: torch decays it, this kernel does not.
__device__ __forceinline__ void adamw_elem(const AdamWArgs& w, const AdamWCoef& c, float graw, float& p, float& m, float& v, float& e) {
#pragma clang fp contract(off)
    const AdamArgs& a = w.a;
    const float g = graw * a.grad_scale * c.gmul;
    const bool idle = g == 0.f && m == 0.f && v == 0.f;
    m = m * a.b1 + (1.f - a.b1) * g;
    v = __builtin_fmaf((1.f - a.b2) * g, g, v * a.b2);
    if (!idle) {
        const float denom = sqrtf(v) / c.bc2s + a.eps;
        p = __builtin_fmaf(-c.step_size, m / denom, p * c.keep);
    }
    if (w.ema) e = w.ema_decay * e + (1.f - w.ema_decay) * p;
}

// n % 4 == 0 and 16-byte bases (what FlatAdam always has): dwordx4 loads and stores, up to six streams, grid-stride
__global__ __launch_bounds__(256) void adamw_vec_k(AdamWArgs w) {
    const AdamArgs& a = w.a;
    if (a.skip && *a.skip != 0) return;
    const AdamWCoef c = adamw_coef(w);
    const long n4 = a.n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(a.g);
    f32x4* p4 = reinterpret_cast<f32x4*>(a.p);
    f32x4* m4 = reinterpret_cast<f32x4*>(a.m);
    f32x4* v4 = reinterpret_cast<f32x4*>(a.v);
    f32x4* e4 = reinterpret_cast<f32x4*>(w.ema);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 g = g4[i];
        f32x4 p = p4[i], m = m4[i], v = v4[i];
        f32x4 e = e4 ? e4[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float pq = p[q], mq = m[q], vq = v[q], eq = e[q];
            adamw_elem(w, c, g[q], pq, mq, vq, eq);
            p[q] = pq; m[q] = mq; v[q] = vq; e[q] = eq;
        }
        m4[i] = m; v4[i] = v; p4[i] = p;
        if (e4) e4[i] = e;
    }
}

// any n / alignment (C-ABI callers), and the n % 4 tail of the vector kernel: elements [i0, n)
__global__ __launch_bounds__(256) void adamw_k(AdamWArgs w) {
    const AdamArgs& a = w.a;
    if (a.skip && *a.skip != 0) return;
    const AdamWCoef c = adamw_coef(w);
    for (long i = w.i0 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        float p = a.p[i], m = a.m[i], v = a.v[i], e = w.ema ? w.ema[i] : 0.f;
        adamw_elem(w, c, a.g[i], p, m, v, e);
        a.m[i] = m; a.v[i] = v; a.p[i] = p;
        if (w.ema) w.ema[i] = e;
    }
}

__global__ __launch_bounds__(256) void swap_vec_k(f32x4* a, f32x4* b, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

__global__ __launch_bounds__(256) void swap_k(float* a, float* b, long i0, long n) {
    for (long i = i0 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// vector kernels: one 16-byte quad per thread and pass, at most 8 workgroups of 256 per CU
static int grid_for_quads(long n4) { long b = (n4 + 255) / 256; return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048); }

extern "C" {

// x_adv = clamp(x + scale*normalise_rows(prescale*d), 0, 1); optional r (=scale*dn) and dn outputs;
// nan_flag (device int, may be null) is OR-ed with 1 when any r is NaN (the reference's assert).
int rv_vat_perturb_fwd(const float* x, const float* d, long rows, int n, float prescale, float scale, float* x_adv,
                       float* r_out, float* dn_out, int* nan_flag, void* stream) {
    PerturbArgs a = {};
    a.x = x; a.d = d; a.x_adv = x_adv; a.r_out = r_out; a.dn_out = dn_out; a.rows = rows; a.n = n;
    a.prescale = prescale; a.scale = scale; a.nan_flag = nan_flag;
    hipLaunchKernelGGL(vat_perturb_k<false>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK("rv_vat_perturb_fwd");
    return RV_OK;
}

// gd = d(loss)/d(d) given g = d(loss)/d(x_adv): through clamp, the scale and the row L2-normalisation.
int rv_vat_perturb_bwd(const float* g, const float* x, const float* d, long rows, int n, float prescale, float scale,
                       float* gd, void* stream) {
    PerturbArgs a = {};
    a.x = x; a.d = d; a.g = g; a.gd = gd; a.rows = rows; a.n = n; a.prescale = prescale; a.scale = scale;
    hipLaunchKernelGGL(vat_perturb_k<true>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK("rv_vat_perturb_bwd");
    return RV_OK;
}

// one partial per 2 048 elements (restated in tests/stream_cases.py: reduce_parts)
long rv_reduce_workspace_bytes(long n) { return ((n + 2047) / 2048) * 4; }

// kind: 0 = BCE mean (p vs soft/hard target t), 1 = MSE mean, 2 = mean |p|, 3 = sqrt(sum p^2) (L2 norm)
// ticket (nullable): a ZEROED device word (left zero again): single-launch form, see reduce_partial_k
int rv_reduce_mean(int kind, const float* p, const float* t, long n, float* out, void* workspace, unsigned* ticket, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int nparts = cdiv(n, 2048);
    float* part = (float*)workspace;
    const double denom = kind == RED_SUMSQ ? 1.0 : (double)n;
    const int sq = kind == RED_SUMSQ ? 1 : 0;
    switch (kind) {
        case RED_BCE: hipLaunchKernelGGL(reduce_partial_k<RED_BCE>, dim3(nparts), dim3(256), 0, st, p, t, n, part, ticket, denom, out, sq); break;
        case RED_MSE: hipLaunchKernelGGL(reduce_partial_k<RED_MSE>, dim3(nparts), dim3(256), 0, st, p, t, n, part, ticket, denom, out, sq); break;
        case RED_ABS: hipLaunchKernelGGL(reduce_partial_k<RED_ABS>, dim3(nparts), dim3(256), 0, st, p, t, n, part, ticket, denom, out, sq); break;
        case RED_SUMSQ: hipLaunchKernelGGL(reduce_partial_k<RED_SUMSQ>, dim3(nparts), dim3(256), 0, st, p, t, n, part, ticket, denom, out, sq); break;
        default: rv_set_error("rv_reduce_mean: bad kind %d", kind); return RV_EINVAL;
    }
    RV_LAUNCH_CHECK("rv_reduce_mean(partial)");
    if (ticket) return RV_OK;
    hipLaunchKernelGGL(reduce_final_k, dim3(1), dim3(256), 0, st, part, nparts, denom, out, sq);
    RV_LAUNCH_CHECK("rv_reduce_mean(final)");
    return RV_OK;
}

// gp = *gout * d(mean loss)/dp ; kind 0 = BCE, 1 = MSE
int rv_loss_bwd(int kind, const float* p, const float* t, long n, const float* gout, float* gp, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (kind == RED_BCE) hipLaunchKernelGGL(loss_bwd_k<RED_BCE>, dim3(grid_for(n)), dim3(256), 0, st, p, t, n, gout, gp);
    else if (kind == RED_MSE) hipLaunchKernelGGL(loss_bwd_k<RED_MSE>, dim3(grid_for(n)), dim3(256), 0, st, p, t, n, gout, gp);
    else { rv_set_error("rv_loss_bwd: bad kind %d", kind); return RV_EINVAL; }
    RV_LAUNCH_CHECK("rv_loss_bwd");
    return RV_OK;
}

int rv_sigmoid_bwd(const float* g1, int ld1, const float* g2, int ld2, const float* y, int ldy, float* dz, int ldz, long M,
                   int N, void* stream) {
    hipLaunchKernelGGL(sigmoid_bwd_k, dim3(grid_for(M * N)), dim3(256), 0, (hipStream_t)stream, g1, ld1, g2, ld2, y, ldy, dz,
                       ldz, M, N);
    RV_LAUNCH_CHECK("rv_sigmoid_bwd");
    return RV_OK;
}

__global__ void zero_floats_k(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// out[n] = sum_m x[m*ld + n]   (out is overwritten unless accumulate)
// (rv_colsum below; its path choice and rows per thread are restated in tests/stream_cases.py: colsum_path)
// out[i] (+)= sum over the RV_BN_NREP replicas of sums[rep][c0 + i], i < n, where `sums` is a BatchNorm statistics workspace of C channels
// ([rep][2][C] fp64) that a conv's fused epilogue filled (rv_conv_fwd bn_sums): the per-channel sums of what the conv stored ARE the
// column sums of its output -- the bias gradient of the layer that consumes that output as dY, without another pass over it.
__global__ void sums_fold_k(const double* sums, int C, int c0, int n, float* out, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < RV_BN_NREP; ++r) s += sums[(long)r * 2 * C + c0 + i];
    out[i] = accumulate ? out[i] + (float)s : (float)s;
}

int rv_sums_fold(const double* sums, int C, int c0, int n, float* out, int accumulate, void* stream) {
    RV_CHECK_ARG(sums && out && n > 0 && c0 >= 0 && c0 + n <= C, "rv_sums_fold: bad channel range");
    hipLaunchKernelGGL(sums_fold_k, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, sums, C, c0, n, out, accumulate);
    RV_LAUNCH_CHECK("rv_sums_fold");
    return RV_OK;
}

int rv_colsum(const float* x, int ld, long M, int N, float* out, int accumulate, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) hipLaunchKernelGGL(zero_floats_k, dim3(cdiv(N, 256)), dim3(256), 0, st, out, N);   // (a kernel: memset nodes proved unreliable across hipGraph replays)
    if ((N & 3) == 0 && N <= 256 && (ld & 3) == 0 && ((((uintptr_t)x) & 15) == 0) && M >= 1024) {
        // rows per thread: ~512 workgroups -- enough to fill the chip on the 5 120-row linear layers (32 rows per thread
        // left 15 workgroups there), few enough that the per-column atomics (serialised, ~23 ns each) stay a short tail
        const int PL = 256 / (N / 4);
        long rpt = M / ((long)PL * 512);
        if (rpt < 4) rpt = 4;
        if (rpt > 64) rpt = 64;
        hipLaunchKernelGGL(colsum_vec_k, dim3(cdiv(M, (long)PL * rpt)), dim3(256), 0, st, x, ld, M, N, out, (int)rpt);
    } else {
        int rpb = 256;
        dim3 grid(cdiv(N, 64), cdiv(M, rpb));
        hipLaunchKernelGGL(colsum_k, grid, dim3(256), 0, st, x, ld, M, N, out, rpb);
    }
    RV_LAUNCH_CHECK("rv_colsum");
    return RV_OK;
}

// Deterministic form of rv_colsum (RV_DETERMINISTIC=1 of the host side): no atomics.  Pass 1: row block b leaves its per-column sums in
// ws[b][N] (plain stores, a fixed row order inside the block); pass 2: one thread per column folds the blocks in index order and
// writes / accumulates.  ws: rv_colsum_ordered_workspace_bytes(M, N), uninitialised.
__global__ __launch_bounds__(256) void colsum_part_k(const float* x, int ld, long M, int N, float* ws, long rows_per_block) {
    __shared__ float sh[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(r0 + rows_per_block, M);
    float s = 0.f;
    if (col < N)
        for (long r = r0 + rl; r < r1; r += 4) s += x[r * ld + col];
    sh[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && col < N) ws[(long)blockIdx.y * N + col] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void colsum_fold_k(const float* ws, int nblk, int N, float* out, int accumulate) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += ws[(long)b * N + col];
    out[col] = accumulate ? out[col] + s : s;
}
// (restated in tests/stream_cases.py: colsum_ordered_blocks, colsum_ordered_launch)
static long colsum_ordered_blocks(long M) {
    long nblk = (M + 255) / 256;
    return nblk > 1024 ? 1024 : (nblk < 1 ? 1 : nblk);
}
long rv_colsum_ordered_workspace_bytes(long M, int N) { return colsum_ordered_blocks(M) * (long)N * 4; }
int rv_colsum_ordered(const float* x, int ld, long M, int N, float* out, int accumulate, void* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RV_CHECK_ARG(ws, "rv_colsum_ordered: null workspace");
    const long nblk = colsum_ordered_blocks(M);
    const long rpb = (M + nblk - 1) / nblk;
    hipLaunchKernelGGL(colsum_part_k, dim3(cdiv(N, 64), (unsigned)nblk), dim3(256), 0, st, x, ld, M, N, (float*)ws, rpb);
    hipLaunchKernelGGL(colsum_fold_k, dim3(cdiv(N, 256)), dim3(256), 0, st, (const float*)ws, (int)nblk, N, out, accumulate);
    RV_LAUNCH_CHECK("rv_colsum_ordered");
    return RV_OK;
}

// One Adam step on flat buffers; lr = lr0 * decay_rate^(step // decay_steps) (StepLR); *step is NOT modified
// (call rv_counter_add afterwards, with the same skip word).  grad_scale multiplies g on the fly (1/world_size after an all-reduce sum).
int rv_adam_step(float* p, const float* g, float* m, float* v, long n, const long* step, float lr0, long decay_steps,
                 float decay_rate, float beta1, float beta2, float eps, float grad_scale, const int* skip, void* stream) {
    AdamArgs a;
    a.skip = skip;
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.step = step; a.lr0 = lr0; a.decay_steps = decay_steps;
    a.decay_rate = decay_rate; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.grad_scale = grad_scale;
    hipLaunchKernelGGL(adam_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a);
    RV_LAUNCH_CHECK("rv_adam_step");
    return RV_OK;
}

// skip (nullable): the per-device "this step is invalid" word -- while it is set the counter does not move either, so a step
// whose update rv_adam_step skipped advances neither StepLR nor the bias correction.
int rv_counter_add(long* counter, long inc, const int* skip, void* stream) {
    hipLaunchKernelGGL(counter_add_k, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, inc, skip);
    RV_LAUNCH_CHECK("rv_counter_add");
    return RV_OK;
}

// g *= min(1, max_norm / (*total_norm + 1e-6))  -- the reference's post-step clip_grad_norm_
int rv_clip_scale(float* g, long n, const float* total_norm, float max_norm, void* stream) {
    hipLaunchKernelGGL(scale_by_clip_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, n, total_norm, max_norm);
    RV_LAUNCH_CHECK("rv_clip_scale");
    return RV_OK;
}

// rv_adam_step with the optimiser options (see adamw_elem for the per-element semantics): g is scaled by grad_scale and by the
// clip coefficient min(1, max_grad_norm / (*total_norm * grad_scale + 1e-6)) (1 when max_grad_norm <= 0 or total_norm is null;
// *total_norm = L2 norm of g as stored, rv_reduce_mean kind 3), p is decayed by 1 - lr * weight_decay before the Adam update, and
// ema (nullable) becomes ema_decay * ema + (1 - ema_decay) * p.  While *skip != 0 nothing is written, ema included.  With
// weight_decay = 0, max_grad_norm = 0 and ema null the result equals rv_adam_step's bit for bit.  n % 4 == 0 with 16-byte aligned
// buffers takes 16-byte loads and stores; anything else a scalar kernel.
int rv_adamw_step(float* p, const float* g, float* m, float* v, long n, const long* step, float lr0, long decay_steps,
                  float decay_rate, float beta1, float beta2, float eps, float grad_scale, const int* skip, float weight_decay,
                  float max_grad_norm, const float* total_norm, float* ema, float ema_decay, void* stream) {
    RV_CHECK_ARG(p && g && m && v && step && n >= 0 && decay_steps > 0, "rv_adamw_step: null buffer, negative n or decay_steps <= 0");
    RV_CHECK_ARG(weight_decay >= 0.f && ema_decay >= 0.f && ema_decay < 1.f, "rv_adamw_step: weight_decay < 0 or ema_decay outside [0, 1)");
    if (n == 0) return RV_OK;
    AdamWArgs w;
    AdamArgs& a = w.a;
    a.skip = skip;
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.step = step; a.lr0 = lr0; a.decay_steps = decay_steps;
    a.decay_rate = decay_rate; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.grad_scale = grad_scale;
    w.weight_decay = weight_decay; w.max_grad_norm = max_grad_norm; w.total_norm = total_norm; w.ema = ema; w.ema_decay = ema_decay;
    w.i0 = 0;
    const bool vec = n >= 4 && aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema);
    if (vec) {
        hipLaunchKernelGGL(adamw_vec_k, dim3(grid_for_quads(n >> 2)), dim3(256), 0, (hipStream_t)stream, w);
        w.i0 = n & ~3L;
    }
    if (w.i0 < n) hipLaunchKernelGGL(adamw_k, dim3(grid_for(n - w.i0)), dim3(256), 0, (hipStream_t)stream, w);
    RV_LAUNCH_CHECK("rv_adamw_step");
    return RV_OK;
}

// a <-> b in place (FlatAdam.ema_weights: the averaged weights take the place of the raw ones and back)
int rv_swap_floats(float* a, float* b, long n, void* stream) {
    RV_CHECK_ARG(a && b && n >= 0, "rv_swap_floats: null buffer or negative n");
    if (n == 0 || a == b) return RV_OK;
    long i0 = 0;
    if (n >= 4 && aligned16(a) && aligned16(b)) {
        hipLaunchKernelGGL(swap_vec_k, dim3(grid_for_quads(n >> 2)), dim3(256), 0, (hipStream_t)stream, (f32x4*)a, (f32x4*)b, n >> 2);
        i0 = n & ~3L;
    }
    if (i0 < n) hipLaunchKernelGGL(swap_k, dim3(grid_for(n - i0)), dim3(256), 0, (hipStream_t)stream, a, b, i0, n);
    RV_LAUNCH_CHECK("rv_swap_floats");
    return RV_OK;
}

}  // extern "C"
