// Device-side segment cropper for the data feed: the reference's item rule
// PianoRollAudioDataset.__getitem__ (model/dataset.py:35-69) applied to a whole batch on the GPU.
//
// The corpus lives in HBM as the reference keeps it on the host: int16 audio and uint8 label / velocity rolls of all
// tracks, concatenated.  The host only draws the crop positions (the reference's RandomState rule) and hands over
// two small index arrays; one launch per tensor family then produces the float batch the training step consumes:
//   audio[b][i]      = float(corpus_audio[audio_begin[b] + i]) / 32768                       (:62, exact in fp32)
//   onset/offset/frame[b][s][k] = label == 3 / == 1 / > 1                                    (:63-65)
//   velocity[b][s][k] = float(vel) / 128                                                     (:66)
// Pure byte/integer streaming (HBM-bound, 2 B -> 4 B and 2 B -> 16 B expansion), bit-exact by construction;
// 16-byte loads and stores whenever the crop start is 16-byte aligned (track starts are padded by the host).
#include "common.h"

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));

struct CropArgs {
    const short* audio; const unsigned char* label; const unsigned char* velocity;
    const long* audio_begin; const long* label_begin;      // [B] element offsets into the corpus buffers
    long seq_len, nlab;                                     // samples per item, label bytes per item (n_steps * n_keys)
    float* out_audio; float* onset; float* offset; float* frame; float* out_velocity;
};

__global__ __launch_bounds__(256) void crop_audio_k(CropArgs a) {
    const int b = blockIdx.y;
    const short* src = a.audio + a.audio_begin[b];
    float* dst = a.out_audio + (long)b * a.seq_len;
    const float k = 1.0f / 32768.0f;                        // power of two: x * k == x / 32768 exactly
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    const long stride = (long)gridDim.x * blockDim.x;
    if (vec) {
        const long n8 = a.seq_len >> 3;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
            const i16x8 v = *reinterpret_cast<const i16x8*>(src + i * 8);
            f32x4 lo = (f32x4){(float)v[0] * k, (float)v[1] * k, (float)v[2] * k, (float)v[3] * k};
            f32x4 hi = (f32x4){(float)v[4] * k, (float)v[5] * k, (float)v[6] * k, (float)v[7] * k};
            *reinterpret_cast<f32x4*>(dst + i * 8) = lo;
            *reinterpret_cast<f32x4*>(dst + i * 8 + 4) = hi;
        }
        for (long i = (n8 << 3) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.seq_len; i += stride) dst[i] = (float)src[i] * k;
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.seq_len; i += stride) dst[i] = (float)src[i] * k;
    }
}

__global__ __launch_bounds__(256) void crop_label_k(CropArgs a) {
    const int b = blockIdx.y;
    const unsigned char* lab = a.label + a.label_begin[b];
    const unsigned char* vel = a.velocity ? a.velocity + a.label_begin[b] : nullptr;
    const long o = (long)b * a.nlab;
    const float kv = 1.0f / 128.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    // four labels per thread when everything is 4-byte (inputs) / 16-byte (outputs) aligned: one dword load, float4 stores
    const bool vec = ((((uintptr_t)lab) | (vel ? (uintptr_t)vel : 0)) & 3) == 0 && ((o | a.nlab) & 3) == 0 &&
                     (((uintptr_t)a.onset | (uintptr_t)a.frame | (uintptr_t)a.offset | (uintptr_t)a.out_velocity) & 15) == 0;
    long done = 0;
    if (vec) {
        const long n4 = a.nlab >> 2;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const unsigned l4 = *reinterpret_cast<const unsigned*>(lab + i * 4);
            f32x4 on, of, fr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned l = (l4 >> (8 * q)) & 255u;
                on[q] = l == 3 ? 1.f : 0.f;
                of[q] = l == 1 ? 1.f : 0.f;
                fr[q] = l > 1 ? 1.f : 0.f;
            }
            *reinterpret_cast<f32x4*>(a.onset + o + i * 4) = on;
            if (a.offset) *reinterpret_cast<f32x4*>(a.offset + o + i * 4) = of;
            *reinterpret_cast<f32x4*>(a.frame + o + i * 4) = fr;
            if (vel && a.out_velocity) {
                const unsigned v4 = *reinterpret_cast<const unsigned*>(vel + i * 4);
                *reinterpret_cast<f32x4*>(a.out_velocity + o + i * 4) =
                    (f32x4){(float)(v4 & 255u) * kv, (float)((v4 >> 8) & 255u) * kv, (float)((v4 >> 16) & 255u) * kv,
                            (float)(v4 >> 24) * kv};
            }
        }
        done = n4 << 2;
    }
    for (long i = done + (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.nlab; i += stride) {
        const unsigned char l = lab[i];
        a.onset[o + i] = l == 3 ? 1.f : 0.f;
        if (a.offset) a.offset[o + i] = l == 1 ? 1.f : 0.f;
        a.frame[o + i] = l > 1 ? 1.f : 0.f;
        if (vel && a.out_velocity) a.out_velocity[o + i] = (float)vel[i] * kv;
    }
}

// ---- pitch-shift augmentation (reconvat_amd/augment.py): the crop of item b transposed by k_b semitones ------------------
// Per item a row of RV_SHIFT_FIELDS longs in device memory:
//   0 a0        corpus index of the crop's first source sample          6 Kp        taps per phase of its bank (multiple of 4)
//   1 t_begin   corpus index of the track's first sample                7 bank_off  float offset of its bank [L, Kp] in `banks` (multiple of 4)
//   2 t_end     ... and one past its last sample                        8 lab       byte offset of source row j0 in the label corpora
//   3 L, 4 M    output sample m sits at source position m M / L         9 rows      source rows that exist from j0 on
//   5 F         bank[p][u] = h[p + (F - u) L]                          10 k         output key c reads source key c - k
// Audio follows resample_k (csrc/resample.hip): a workgroup owns Lr * 4 consecutive outputs of ONE item, Lr = the multiple of the
// item's L next to 256, stages their source span once in LDS (int16 -> float and the zero extension at the TRACK's ends on that load:
// every global read is predicated on [t_begin, t_end), so a neighbouring track of the corpus is never read), and work item w sums
// outputs w, w + Lr, .. -- which share their phase, hence one 16-byte coefficient load feeds all four -- each in ONE accumulator over
// u = 0 .. Kp-1 ascending with fmaf: the bits do not depend on the tile, on B or on the item's place in the batch.  L, M, Kp differ
// between the items of a launch; they are uniform within a workgroup, and LDS is sized for the largest legal item.
// A row outside the limits below cannot be reported from the device: its outputs are NaN, never an out-of-bounds access.
#define RV_SHIFT_FIELDS 12
#define RV_SHIFT_MAX_TERM 128                  // L, M; and M <= 2 L, L <= 2 M (half an octave either way is 1.415)
#define RV_SHIFT_MAX_KP 256
#define RV_SHIFT_R 4
// floats of LDS: Lr < 256 + 128, so ((L-1) + (Lr-1) M) / L < 1 + 382 * 2, 3 * (Lr / L * M) <= 3 * 766, plus Kp <= 256: < 3319
#define RV_SHIFT_LDS 3328

struct ShiftArgs {
    const short* audio; const unsigned char* label; const unsigned char* velocity; const float* banks; const long* items;
    long n_audio, n_label, n_bank, seq_len;
    int n_steps, n_keys;
    float* out_audio; float* onset; float* offset; float* frame; float* out_velocity;
};

__device__ __forceinline__ bool shift_ratio_ok(long L, long M) {
    return L >= 1 && M >= 1 && L <= RV_SHIFT_MAX_TERM && M <= RV_SHIFT_MAX_TERM && M <= 2 * L && L <= 2 * M;
}

__global__ __launch_bounds__(256) void shift_audio_k(ShiftArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[RV_SHIFT_LDS];
    const int b = blockIdx.y;
    const long* it = a.items + (long)b * RV_SHIFT_FIELDS;
    const long a0 = it[0], bank_off = it[7];
    const long t_begin = it[1] > 0 ? it[1] : 0, t_end = it[2] < a.n_audio ? it[2] : a.n_audio;
    const long Ll = it[3], Ml = it[4], Fl = it[5], Kl = it[6];
    float* dst = a.out_audio + (long)b * a.seq_len;
    const bool ok = shift_ratio_ok(Ll, Ml) && Kl >= 4 && Kl <= RV_SHIFT_MAX_KP && (Kl & 3) == 0 && Fl >= 0 && Fl < Kl && bank_off >= 0 &&
                    (bank_off & 3) == 0 && bank_off + Ll * Kl <= a.n_bank;
    if (!ok) {                                                 // (the grid has a workgroup per 1024 outputs: this covers the item)
        for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < a.seq_len && i < ((long)blockIdx.x + 1) * 1024; i += 256)
            dst[i] = __builtin_nanf("");
        return;
    }
    const int L = (int)Ll, M = (int)Ml, F = (int)Fl, Kp = (int)Kl;
    const int Lr = (256 + L - 1) / L * L, stepx = Lr / L * M;
    const long t0 = (long)blockIdx.x * (Lr * RV_SHIFT_R);      // first output of the tile
    if (t0 >= a.seq_len) return;                               // Lr >= 256: items with a larger tile need fewer workgroups
    const int span = (int)(((long)(L - 1) + (long)(Lr - 1) * M) / L) + (RV_SHIFT_R - 1) * stepx + Kp;      // <= RV_SHIFT_LDS
    const long q0 = t0 * M;
    const long n_base = a0 + q0 / L - F;                       // corpus index of xs[0]
    const int p0 = (int)(q0 % L);
    for (int s = threadIdx.x; s < span; s += 256) {
        const long n = n_base + s;
        xs[s] = (n >= t_begin && n < t_end) ? (float)a.audio[n] * (1.0f / 32768.0f) : 0.f;
    }
    __syncthreads();
    const float* bank = a.banks + bank_off;
    const long left = a.seq_len - t0;
    for (int w = threadIdx.x; w < Lr && w < left; w += 256) {
        const long t = (long)p0 + (long)w * M;
        const int off = (int)(t / L), p = (int)(t % L);
        const f32x4* row = reinterpret_cast<const f32x4*>(bank + (long)p * Kp);
        const float* xr = xs + off;
        float acc[RV_SHIFT_R];
#pragma unroll
        for (int r = 0; r < RV_SHIFT_R; ++r) acc[r] = 0.f;
        for (int u = 0; u < Kp; u += 4) {
            const f32x4 c = row[u >> 2];
#pragma unroll
            for (int r = 0; r < RV_SHIFT_R; ++r) {
                const float* xv = xr + r * stepx + u;
                acc[r] = fmaf(c[0], xv[0], acc[r]);
                acc[r] = fmaf(c[1], xv[1], acc[r]);
                acc[r] = fmaf(c[2], xv[2], acc[r]);
                acc[r] = fmaf(c[3], xv[3], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RV_SHIFT_R; ++r) {
            const long i = t0 + w + (long)r * Lr;
            if (i < a.seq_len) dst[i] = acc[r];
        }
    }
}

// Labels: one work item per output frame and four keys, integer arithmetic only.  near(s) = (2 s M + L) / (2 L); the source rows u with
// tgt(u) = (2 u L + M) / (2 M) == s are those with 2 M s - M <= 2 u L < 2 M s + M: at most M / L + 1 of them.  Rows >= `rows` are empty.
__global__ __launch_bounds__(256) void shift_label_k(ShiftArgs a) {
    const int b = blockIdx.y;
    const long* it = a.items + (long)b * RV_SHIFT_FIELDS;
    const long L = it[3], M = it[4], lab = it[8], k = it[10];
    const int nk = a.n_keys, kq = nk >> 2;
    const long n4 = (long)a.n_steps * kq, o = (long)b * a.n_steps * nk;
    const long stride = (long)gridDim.x * blockDim.x;
    const bool ok = shift_ratio_ok(L, M) && lab >= 0 && lab <= a.n_label && k > -nk && k < nk;
    long rows = ok ? it[9] : 0;
    if (ok && rows > (a.n_label - lab) / nk) rows = (a.n_label - lab) / nk;
    const float kv = 1.0f / 128.0f, fill = ok ? 0.f : __builtin_nanf("");
    const unsigned char* roll = a.label + lab;
    const unsigned char* vroll = a.velocity + lab;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const long s = i / kq;
        const int c0 = (int)(i - s * kq) * 4;
        f32x4 on = (f32x4){fill, fill, fill, fill}, of = on, fr = on, ve = on;
        if (ok) {
            const long near = (2 * s * M + L) / (2 * L);
            const long lo2 = 2 * s * M - M;
            const long u_lo = lo2 <= 0 ? 0 : (lo2 + 2 * L - 1) / (2 * L);
            long u_end = (2 * s * M + M + 2 * L - 1) / (2 * L);
            if (u_end > rows) u_end = rows;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long src = c0 + q - k;
                if (src < 0 || src >= nk) continue;
                bool ev3 = false, ev1 = false;
                for (long u = u_lo; u < u_end; ++u) {
                    const unsigned char l = roll[u * nk + src];
                    ev3 |= l == 3;
                    ev1 |= l == 1;
                }
                const bool have = near < rows;
                const bool sounding = have && roll[near * nk + src] > 1;
                const int code = ev3 ? 3 : sounding ? 2 : ev1 ? 1 : 0;
                on[q] = code == 3 ? 1.f : 0.f;
                of[q] = code == 1 ? 1.f : 0.f;
                fr[q] = code > 1 ? 1.f : 0.f;
                ve[q] = have ? (float)vroll[near * nk + src] * kv : 0.f;
            }
        }
        *reinterpret_cast<f32x4*>(a.onset + o + i * 4) = on;
        *reinterpret_cast<f32x4*>(a.offset + o + i * 4) = of;
        *reinterpret_cast<f32x4*>(a.frame + o + i * 4) = fr;
        *reinterpret_cast<f32x4*>(a.out_velocity + o + i * 4) = ve;
    }
}

extern "C" {

// audio: int16 corpus, label / velocity: uint8 corpora (velocity, offset, out_velocity nullable); audio_begin /
// label_begin: DEVICE arrays of B element offsets (label_begin in bytes = step_begin * n_keys + track offset).
// out_audio [B, seq_len]; onset / offset / frame / out_velocity [B, n_steps, n_keys] float32.
int rv_crop_segments(const short* audio, const unsigned char* label, const unsigned char* velocity, const long* audio_begin,
                     const long* label_begin, int B, long seq_len, int n_steps, int n_keys, float* out_audio, float* onset,
                     float* offset, float* frame, float* out_velocity, void* stream) {
    RV_CHECK_ARG(B >= 1 && seq_len >= 1 && n_steps >= 1 && n_keys >= 1, "rv_crop_segments: empty batch");
    RV_CHECK_ARG(audio && label && audio_begin && label_begin && out_audio && onset && frame, "rv_crop_segments: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CropArgs a;
    a.audio = audio; a.label = label; a.velocity = velocity; a.audio_begin = audio_begin; a.label_begin = label_begin;
    a.seq_len = seq_len; a.nlab = (long)n_steps * n_keys;
    a.out_audio = out_audio; a.onset = onset; a.offset = offset; a.frame = frame; a.out_velocity = out_velocity;
    long bx = cdiv(seq_len / 8 + 1, 256);
    if (bx > 64) bx = 64;                                   // 64 x B workgroups stream a 327 680-sample batch
    hipLaunchKernelGGL(crop_audio_k, dim3((unsigned)bx, B), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_crop_segments(audio)");
    long lx = cdiv(a.nlab, 256);
    if (lx > 64) lx = 64;
    hipLaunchKernelGGL(crop_label_k, dim3((unsigned)lx, B), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_crop_segments(labels)");
    return RV_OK;
}

// The crop of rv_crop_segments with item b transposed by items[b].k semitones (layout of `items` and the definition: above and
// reconvat_amd/augment.py).  audio [n_audio] int16, label / velocity [n_label] uint8, banks [n_bank] float32 (16-byte aligned):
// the polyphase banks of every shift, concatenated; items: DEVICE array [B, 12] of longs.  Outputs as rv_crop_segments (none nullable,
// 16-byte aligned, n_keys a multiple of 4).  One launch for the audio, one for the labels; no atomics, allocation or synchronisation.
int rv_crop_segments_shift(const short* audio, long n_audio, const unsigned char* label, const unsigned char* velocity, long n_label,
                           const float* banks, long n_bank, const long* items, int B, long seq_len, int n_steps, int n_keys,
                           float* out_audio, float* onset, float* offset, float* frame, float* out_velocity, void* stream) {
    RV_CHECK_ARG(B >= 1 && B <= 65535 && seq_len >= 1 && seq_len <= (1L << 31) && n_steps >= 1, "rv_crop_segments_shift: empty or oversized batch");
    RV_CHECK_ARG(n_keys >= 4 && (n_keys & 3) == 0 && n_keys <= 1024, "rv_crop_segments_shift: n_keys %d must be a multiple of 4 in 4..1024", n_keys);
    RV_CHECK_ARG(audio && label && velocity && banks && items && out_audio && onset && offset && frame && out_velocity,
                 "rv_crop_segments_shift: null pointer");
    RV_CHECK_ARG(n_audio >= 1 && n_label >= 1 && n_bank >= 4, "rv_crop_segments_shift: empty corpus or bank");
    RV_CHECK_ARG(((((uintptr_t)banks) | (uintptr_t)onset | (uintptr_t)offset | (uintptr_t)frame | (uintptr_t)out_velocity) & 15) == 0 &&
                 (((uintptr_t)items) & 7) == 0, "rv_crop_segments_shift: banks and label outputs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ShiftArgs a;
    a.audio = audio; a.label = label; a.velocity = velocity; a.banks = banks; a.items = items;
    a.n_audio = n_audio; a.n_label = n_label; a.n_bank = n_bank; a.seq_len = seq_len; a.n_steps = n_steps; a.n_keys = n_keys;
    a.out_audio = out_audio; a.onset = onset; a.offset = offset; a.frame = frame; a.out_velocity = out_velocity;
    hipLaunchKernelGGL(shift_audio_k, dim3((unsigned)cdiv(seq_len, 256 * RV_SHIFT_R), B), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_crop_segments_shift(audio)");
    long lx = cdiv((long)n_steps * (n_keys / 4), 256);
    if (lx > 64) lx = 64;
    hipLaunchKernelGGL(shift_label_k, dim3((unsigned)lx, B), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_crop_segments_shift(labels)");
    return RV_OK;
}

}  // extern "C"
