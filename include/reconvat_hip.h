/*
 * reconvat_hip.h -- C ABI of libreconvat_hip.so (gfx950 / MI355X only).
 *
 * The reference (KinWaiCheuk/ReconVAT) has no native layer: its hot path is a chain of generic
 * PyTorch ops.  Each entry point below replaces the PyTorch call sites cited next to it (paths are
 * relative to the reference root).  Conventions, for every function:
 *   - plain `extern "C"`, raw DEVICE pointers, explicit sizes/strides, fp32 data;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); the call only ENQUEUES work:
 *     it never allocates, never synchronises, never owns memory (the host framework's allocator owns
 *     every buffer; scratch is passed in as `workspace`, sized by the *_workspace_bytes queries);
 *   - returns 0 on success, <0 on error (-1 bad argument, -2 launch failure, -3 unsupported shape);
 *     `rv_last_error()` returns the text of the last error on the calling thread;
 *   - re-entrant per stream.  Process-global state, all of it: (1) the weight-gradient plan table written by
 *     rv_conv_wgrad_set_plan (configure it once per shape before the first launch of that shape: the shipped plan table does
 *     exactly that; it is not synchronised against concurrent launches of the same shape); (2) the block-tile policy of rv_gemm,
 *     an atomic that only the test hook rv_debug_set_gemm_big writes (default: 64 x 64 tiles everywhere); (3) the form of the
 *     local-attention kernels, fixed when the library is LOADED from RV_ATTN_TILE, RV_ATTN_TILE_WIDE, RV_ATTN_WAVES and
 *     RV_ATTN_WAVES_WIDE (unset: the shipped choice per head shape) and constant afterwards.  Nothing else is read from the
 *     environment, and nothing at all on a launch path (the experiment knobs of tools/ exist in the lab / ablation builds only:
 *     reconvat_amd/build.py).
 *
 * Activations are NHWC with an explicit pixel stride `*_ld` (floats between consecutive pixels), so a
 * tensor may be a channel slice of a wider buffer (the decoder's concat buffers).
 */
#ifndef RECONVAT_HIP_H
#define RECONVAT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

int rv_abi_version(void);
const char* rv_last_error(void);
/* first 16 hex digits of the sha256 over the sources (reconvat_amd/csrc: *.hip, *.h, *.cpp) this library was built from */
const char* rv_source_digest(void);

/* ---- log-Mel front-end ------------------------------------------------------------------------
 * replaces nnAudio MelSpectrogram.forward / STFT.forward (model/Spectrogram.py:187-231, :443-461),
 * torch.log(spec + 1e-5) and Normalization('imagewise').transform (model/UNet_onset.py:419-423,
 * :432-442; model/utils.py:94-100).  audio [B, nsamp] -> out [B, T, n_mels], T = 1 + nsamp/hop.
 * twiddle: [1024][2] = (cos, -sin)(2*pi*k/2048); window: [2048]; sparse mel rows: start/len/w[n_mels][mel_ld].
 * workspace: 2*B uint32. */
int rv_melspec_lognorm_fwd(const float* audio, long audio_stride, int B, int nsamp, const float* window,
                           const float* twiddle, const int* mel_start, const int* mel_len, const float* mel_w, int mel_ld,
                           int n_mels, int hop, int do_log, int normalise, float* out, int T, void* workspace, void* stream);

/* ---- constant-Q front end (nnAudio CQT1992v2 as the reference configures it, model/UNet_onset.py:346-349) ----------
 * audio [B, nsamp] -> out [B, T, n_bins] time-major, T = 1 + nsamp/hop, reflect pad kernel_width/2 (nsamp must exceed it):
 * |cqt| (do_log: log(|cqt| + 1e-5); normalise: per-clip min-max).  w / items / groups / scale are the packed tables of
 * reconvat_amd.frontend.CQT1992v2.tables(): per 16-bin group the [32][K_g] taps of its window, split-K work items
 * (group, first tap, taps, weight offset, K_g, 0, 0, 0), per group (first item, item count), sqrt(lengths).
 * workspace: rv_cqt_workspace_bytes(B, nsamp, n_items, hop, kernel_width) bytes, 16-byte aligned. */
long rv_cqt_workspace_bytes(int B, int nsamp, int n_items, int hop, int kernel_width);
int rv_cqt_lognorm_fwd(const float* audio, long audio_stride, int B, int nsamp, const float* w, long w_floats, const int* items,
                       int n_items, const int* groups, int n_groups, const float* scale, int n_bins, int kernel_width, int hop,
                       int do_log, int normalise, float* out, int T, void* workspace, long workspace_bytes, void* stream);

/* ---- convolutions (nn.Conv2d / nn.ConvTranspose2d call sites, model/UNet_onset.py:173-224) ------
 * rv_pack_weights: PyTorch-layout weight -> MFMA fragment order for a logical Wm[tap][k][n]
 *   value(tap,k,n) = w[k*s_k + n*s_n + (flip ? taps-1-tap : tap)];  scatter_cmid>0: 2x2/s2 scatter GEMM.
 *   3x3 weights with kdim % 16 == 0 also carry their Winograd F(2x2,3x3) transform U = G g G^T (16 fragments per chunk and
 *   n-tile) behind the nine tap fragments; rv_packed_weight_floats counts both.
 * rv_conv_fwd mode: 0 = 3x3 s1 p1, 1 = 1x1, 2 = 2x2/s2 gather (down fwd, up dgrad), 3 = 2x2/s2 scatter
 *   (ConvTranspose2d(k=2,s=2)(x, output_size=...) fwd, down dgrad).  Forward AND input-gradient of
 *   every layer are instances of it (the packing decides which).  algo: 0 default, 1 LDS-free direct kernel,
 *   2 LDS/DMA-pipelined kernel (3x3 only); forced tiles for the host autotuner (ops._conv_call), RV_EUNSUPPORTED when the tile
 *   does not fit the shape: 0x100|NT<<4|MT direct kernel, 0x200 / 0x300 / 0x400 / 0x700 |NT<<4|MTW LDS kernel with 4 / 8 / 16 /
 *   12 waves per workgroup (MTW in {3,5,6} for 12 waves: 9/15/18 tiles per SIMD and band), optionally TH<<12 = rows per band
 *   (<= what the tile slots hold); 0x600 |NT<<4|MTW: Winograd F(2x2,3x3) form of the persistent 3x3 kernel with 8 waves per
 *   workgroup (Cin % 16 == 0; NT = MTW = 1; TH<<12 = even rows per band), same epilogue fusions; 0xA00 / 0xC00: the same with the
 *   patch read half a chunk at a time, 8 waves (NT in {1,2}, MTW = 1) / 12 waves (NT = MTW = 1); 0x800 / 0x900 / 0xB00 / 0xD00 |NT<<4|MTW (round 5,
 *   conv_wino2.hip): the software-pipelined Winograd kernel -- 8 waves with the full-chunk patch (NT = MTW = 1), 8 waves with the
 *   half-chunk patch ((NT, MTW) in {(1,1), (2,1), (1,2)}), 4 waves with 512 registers ((1,2), (2,1)), 12 waves with the half-chunk patch (NT = MTW = 1); same results as 0x600 up to the
 *   fp32 summation order, same epilogue fusions (the 8-wave NT = 2 tile refuses bn_z).  bn_sums (nullable,
 *   rv_bn_workspace_bytes(Cout) bytes of fp64 = 8 replicas of [2*Cout] that the consumer adds up, += ): per-channel sum / sum of squares of the written output, i.e. the batch statistics of the
 *   BatchNorm2d that consumes it (conv -> bn call sites, model/UNet_onset.py:196-198,221-223), produced in the conv
 *   epilogue; pass the same buffer to rv_bn_lrelu_fwd as `workspace` with sums_ready = 1.  bn_z (nullable; with
 *   bn_z_ld, bn_coef = that layer's saved [5C] coefficients, bn_slope): the call is an INPUT-GRADIENT whose result is
 *   d(loss)/d(output of a BatchNorm+leaky_relu with pre-normalisation input bn_z); bn_sums then receives that layer's
 *   backward reduction (sum dd, sum dd*xhat) and rv_bn_lrelu_bwd(..., sums_ready = 1) skips its own pass over dy, z.
 * rv_conv_wgrad: G[tap][a][b] = sum_p U[f(p,tap)][a]*V[p][b] (+ column sums of V for the bias), written
 *   to dw[a*s_a + b*s_b + tap'] / dbias[b]; mode 0 = 3x3, 1 = 1x1, 2 = 2x2/s2.  U is [B, Hu, Wu] pixels of u_ld >= Ca floats, V
 *   [B, Hv, Wv] pixels of v_ld >= Cb floats; modes 0 and 1 want Hu == Hv and Wu == Wv, mode 2 wants 2 Hv <= Hu <= 2 Hv + 1 and
 *   2 Wv <= Wu <= 2 Wv + 1.  Outside the small-channel kernels (Ca * Cb * taps <= 144 with Ca < 8 or Cb < 8, and the sliced
 *   1 -> 32 / 48 3x3 layer, which take any stride and alignment) the rows are staged by 16-byte LDS-DMA, one channel quad per lane:
 *   Ca, Cb, u_ld and v_ld must be multiples of 4 and U and V (every segment of rv_conv_wgrad_seg) 16-byte aligned.  Anything else
 *   is refused with -1 before a kernel is launched. */
long rv_packed_weight_floats(int taps, int kdim, int ndim);
int rv_pack_weights(const float* w, float* out, int taps, int kdim, int ndim, long s_k, long s_n, int flip,
                    int scatter_cmid, int force_plain, void* stream);
/* batched packing (all weights of the model, one launch per optimiser step): fill a HOST table entry by entry
 * (i = 0, 1, ... in order; returns the running workgroup total, <0 on error), copy it to the device, run it. */
long rv_pack_table_entry_bytes(void);
long rv_pack_table_fill(void* table_host, int i, const float* w, float* out, int taps, int kdim, int ndim, long s_k, long s_n,
                        int flip, int scatter_cmid, int force_plain);
int rv_pack_table_run(const void* table_dev, int count, long total_blocks, void* stream);
int rv_conv_fwd(int mode, const float* in, int in_ld, int B, int H, int W, int Cin, float* out, int out_ld, int Ho,
                int Wo, int Cout, const float* wpack, const float* bias, int accumulate, int algo, double* bn_sums,
                const float* bn_z, int bn_z_ld, const float* bn_coef, float bn_slope, void* stream);
long rv_conv_wgrad_workspace_bytes(int taps, int B, int Hv, int Ca, int Cb);
/* Host autotuner hook (reconvat_amd/ops.py conv_wgrad): the launch partition of the MFMA weight-gradient kernel for this shape
 * from now on -- nw = waves per workgroup (4 / 8, 0 = default; 24 = eight waves, Winograd F(3x3, 2x2) form of the 3x3 kernel,
 * wgrad_wino_k: even Hv, falls back to the direct form where its six-row ring does not fit LDS), wgs = workgroups on the chip
 * (0 = default 256).  Changes the result of rv_conv_wgrad_workspace_bytes for the shape; not thread-safe against concurrent
 * weight-gradient calls. */
int rv_conv_wgrad_set_plan(int taps, int B, int Hv, int Ca, int Cb, int nw, int wgs);
int rv_conv_wgrad(int mode, const float* U, int u_ld, int Hu, int Wu, int Ca, const float* V, int v_ld, int Hv, int Wv,
                  int Cb, int B, float* dw, long s_a, long s_b, int flip, float* dbias, int accumulate, void* workspace,
                  long workspace_bytes, void* stream);
/* Deferred weight-gradient reductions: rv_conv_wgrad_deferred launches only the partial-sum kernel of rv_conv_wgrad and
 * writes the pending reduction (which ADDS into dw / dbias, fp32 atomics) to *entry_host (rv_wgrad_table_entry_bytes() bytes
 * of HOST memory); it returns the number of workgroups that reduction needs (> 0) or a negative status.  After the last
 * entry, rv_wgrad_table_finalize(table_host, count) turns the counts into block offsets and returns the total; a DEVICE copy
 * of the table then runs every reduction of a backward pass in ONE launch (rv_wgrad_reduce_table).  Workspaces must stay
 * untouched until then.  (One reduction launch per layer is launch-latency bound: 161 launches of ~5 us per step.) */
long rv_conv_wgrad_deferred(int mode, const float* U, int u_ld, int Hu, int Wu, int Ca, const float* V, int v_ld, int Hv, int Wv,
                            int Cb, int B, float* dw, long s_a, long s_b, int flip, float* dbias, void* workspace,
                            long workspace_bytes, void* entry_host, void* stream);
/* Segmented forms: the pixel reduction runs over nseg (1..4) runs of Bseg images, run s at U[s] / V[s] (identical geometry and strides):
 * the (input, dY) pairs of ONE layer from several backward passes of a training step (model/UNet_onset.py:383,117-146: the transcriber
 * is back-propagated three times per step on one stream) folded by ONE launch instead of one per pass -- the fixed cost of a
 * weight-gradient launch (prologue, accumulator fold, partial sums, reduction entry) is paid once.  Plan and workspace: those of
 * B = nseg * Bseg images.  RV_EUNSUPPORTED for the small-channel layers (launch those per pass). */
int rv_conv_wgrad_seg(int mode, int nseg, const float* const* U, const float* const* V, int u_ld, int Hu, int Wu, int Ca, int v_ld, int Hv,
                      int Wv, int Cb, int Bseg, float* dw, long s_a, long s_b, int flip, float* dbias, int accumulate, void* workspace,
                      long workspace_bytes, void* stream);
long rv_conv_wgrad_deferred_seg(int mode, int nseg, const float* const* U, const float* const* V, int u_ld, int Hu, int Wu, int Ca, int v_ld,
                                int Hv, int Wv, int Cb, int Bseg, float* dw, long s_a, long s_b, int flip, float* dbias, void* workspace,
                                long workspace_bytes, void* entry_host, void* stream);
long rv_wgrad_table_entry_bytes(void);
long rv_wgrad_table_finalize(void* table_host, int count);
int rv_wgrad_reduce_table(const void* table_dev, int count, long total_blocks, void* stream);


/* ---- BatchNorm2d(momentum=0.1) + leaky_relu (+ residual) (model/UNet_onset.py:183,196-199,221-223) --
 * coef [5C] = mean, invstd, scale, shift, unbiased batch variance (saved for backward).  training: 0 eval, 1 train,
 * 2 train without touching the running statistics (rv_bn_running_update applies that update later, in sequence).  workspace: rv_bn_workspace_bytes(C) bytes that are
 * ALL-ZERO on entry (fp64 per-channel sums accumulate there); the host carves them from one arena cleared per step.
 * sums_ready != 0: the workspace already holds the sums of z (rv_conv_fwd's bn_sums) and the statistics pass is skipped. */
long rv_bn_workspace_bytes(int C);
int rv_bn_lrelu_fwd(const float* z, int z_ld, long P, int C, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, long* num_batches_tracked, float momentum, float eps, int training, float slope,
                    const float* res, int res_ld, float* y, int y_ld, float* coef, void* workspace, int sums_ready,
                    void* stream);
/* the same with the residual evaluated in place: y = leaky_relu(bn(z)) + skip(x), skip = the 1x1 convolution of an encoder block (model/UNet_onset.py:186-201:
 * `x12 += self.skip(x)`), x [P][cin] at pixel stride x_ld (floats), w [C][cin] (the PyTorch Conv2d weight), b [C] nullable; cin = 1 (block 1: the single-channel
 * spectrogram, one fma per element) or 16 / 32 / 64 (an fmaf chain per element in the k order of rv_conv_fwd's MFMA kernel; ksplit != 0: the K-split form of
 * that kernel, algo family 0x5NM).  BIT-IDENTICAL to rv_conv_fwd(mode 1) + rv_bn_lrelu_fwd(res = its output): v_mfma_f32_16x16x4_f32 is a chain of fused
 * multiply-adds in k order (tools/probes/mfma_f32_order.hip).  Saves the conv launch, the write of its result and the read of it here. */
int rv_bn_lrelu_fwd_skip(const float* z, int z_ld, long P, int C, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, long* num_batches_tracked, float momentum, float eps, int training, float slope,
                         const float* x, int x_ld, int cin, const float* w, const float* b, int ksplit, float* y, int y_ld, float* coef,
                         void* workspace, int sums_ready, void* stream);
int rv_bn_running_update(float* running_mean, float* running_var, long* num_batches_tracked, const float* coef, int C,
                         float momentum, void* stream);
/* all deferred running-statistic updates of a step in one launch: table (DEVICE int64 words) = nlayers x {running_mean,
 * running_var, num_batches_tracked, C, first, count} followed by the coef pointers; layer l applies coefs[first .. first+count)
 * in order. */
int rv_bn_running_update_table(const long* table, int nlayers, float momentum, void* stream);
int rv_bn_lrelu_bwd(const float* dy, int dy_ld, const float* z, int z_ld, long P, int C, const float* coef, float slope,
                    int frozen, float* dz, int dz_ld, float* dgamma, float* dbeta, int param_accumulate, void* workspace,
                    int sums_ready, void* stream);

/* ---- linear layers (nn.Linear / torch.sigmoid call sites, model/UNet_onset.py:50-52,62-64,275,
 * 292-293,307-313,324,330): C[m*scm+n*scn] (+)= act(sum_k A[m*sam+k*sak]*B[k*sbk+n*sbn] + bias[n]);
 * splitk > 1: the reduction is split over workgroups; splitk_ws == NULL: fp32 atomic accumulation (arrival-order rounding; act 0,
 * no C2; the parameter-gradient GEMMs); splitk_ws != NULL: DETERMINISTICALLY -- every k slice parks its partial tile in splitk_ws
 * (rv_gemm_splitk_workspace_bytes, uninitialised) and a second launch on the same stream adds the slices in k order and runs the
 * epilogue, so the result does not depend on arrival order and no atomics touch C (splitk_tickets: unused since round 5, may be
 * NULL; rv_gemm_splitk_ticket_bytes returns 0 -- the in-kernel ticketed fold it served needed device-scope fences that cost
 * ~30 us per slice on this multi-XCD part); batch > 1: problem z of `batch` equal-shape problems lives at A + z*bsa,
 * B + z*bsb, C + z*bsc (the per-head relative-position gradient of the attention).  a_rowsum (nullable, batch == 1):
 * a_rowsum[m] += sum_k A[m][k] (k slices folded in order): the bias gradient of a linear layer rides on its weight-gradient
 * GEMM (A = dY^T). */
long rv_gemm_splitk_workspace_bytes(int M, int N, int splitk, int batch);
long rv_gemm_splitk_ticket_bytes(int M, int N, int splitk, int batch);
int rv_gemm(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long scm, long scn, float* C2,
            long sc2m, long sc2n, const float* bias, int M, int N, int K, int act, int accumulate, int splitk, int batch,
            long bsa, long bsb, long bsc, float* a_rowsum, void* splitk_ws, void* splitk_tickets, void* stream);
/* grouped launch of independent ACCUMULATING problems of one operand orientation (the parameter-gradient GEMMs of a backward
 * pass, each too small to fill the chip): fill HOST entries (returns the orientation code, <0 on error), finalize (returns the
 * total workgroup count; *fold_blocks <- that of the fold launch), copy the table to the device, run.  The problems ADD into their
 * destinations (two entries may share one): final adds are fp32 atomics.  Split-K inside a table: with a per-entry workspace
 * (rv_gemm_splitk_workspace_bytes) the k slices are parked and a second grouped launch folds them in k order -- one atomic per
 * output element; splitk_ws == NULL: every slice adds atomically. */
long rv_gemm_table_entry_bytes(void);
long rv_gemm_table_fill(void* entry_host, const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long scm,
                        long scn, const float* bias, int M, int N, int K, int splitk, int batch, long bsa, long bsb, long bsc,
                        float* a_rowsum, void* splitk_ws);
long rv_gemm_table_finalize(void* table_host, int count, long* fold_blocks);
int rv_gemm_table_run(const void* table_dev, int count, long total_blocks, long fold_blocks, int orientation, void* stream);
int rv_sigmoid_bwd(const float* g1, int ld1, const float* g2, int ld2, const float* y, int ldy, float* dz, int ldz, long M,
                   int N, void* stream);
int rv_colsum(const float* x, int ld, long M, int N, float* out, int accumulate, void* stream);
/* the same without atomics (the host side's RV_DETERMINISTIC=1 mode: bit-reproducible parameter gradients): row blocks leave their
 * partial sums in ws (rv_colsum_ordered_workspace_bytes, uninitialised), a second pass folds them in block order */
long rv_colsum_ordered_workspace_bytes(long M, int N);
int rv_colsum_ordered(const float* x, int ld, long M, int N, float* out, int accumulate, void* ws, void* stream);
/* out[i] (+)= per-channel sum c0 + i of a statistics workspace a conv's fused epilogue filled (rv_conv_fwd bn_sums, C channels): the
 * column sums of that conv's output = the bias gradient of the layer consuming it as dY (the 2x2 up-conv), without re-reading it */
int rv_sums_fold(const double* sums, int C, int c0, int n, float* out, int accumulate, void* stream);

/* ---- 31-frame local multi-head attention (MutliHeadAttention1D.forward, model/UNet_onset.py:56-91)
 * q,k,v (and dq,dk,dv): rows of G*dh floats with row stride ld / dld (column slices of one fused projection buffer
 * are fine); out, dout [B,L,G*dh] contiguous; relT [31,G*dh] = the `rel` parameter transposed (rv_pack_weights with
 * taps=1, kdim=31, ndim=G*dh, s_k=1, s_n=31, force_plain=1 produces it); att, de [B,L,G,31]. */
int rv_local_attn_fwd(const float* q, const float* k, const float* v, long ld, const float* relT, float* out, float* att, int B,
                      int L, int G, int dh, void* stream);
int rv_local_attn_bwd(const float* dout, const float* q, const float* k, const float* v, long ld, const float* relT,
                      const float* att, float* dq, float* dk, float* dv, long dld, float* de, int B, int L, int G, int dh,
                      void* stream);

/* ---- VAT primitives (UNet_VAT.forward / _l2_normalize, model/UNet_onset.py:126-151,165-171) --------
 * x_adv = clamp(x + scale * rownormalise(prescale*d), 0, 1) over rows of n elements. */
int rv_vat_perturb_fwd(const float* x, const float* d, long rows, int n, float prescale, float scale, float* x_adv,
                       float* r_out, float* dn_out, int* nan_flag, void* stream);
int rv_vat_perturb_bwd(const float* g, const float* x, const float* d, long rows, int n, float prescale, float scale,
                       float* gd, void* stream);

/* ---- losses (F.binary_cross_entropy / F.mse_loss / .abs().mean(), model/UNet_onset.py:136-137,
 * 157-158,471-483); kind 0 BCE, 1 MSE, 2 mean|p|, 3 sqrt(sum p^2).  workspace: rv_reduce_workspace_bytes(n).  ticket (nullable): a
 * zeroed device word (left zero): the last workgroup folds the partial sums itself -- one launch instead of two. */
long rv_reduce_workspace_bytes(long n);
int rv_reduce_mean(int kind, const float* p, const float* t, long n, float* out, void* workspace, unsigned* ticket, void* stream);
int rv_loss_bwd(int kind, const float* p, const float* t, long n, const float* gout, float* gp, void* stream);

/* ---- optimiser (torch.optim.Adam + StepLR + clip_grad_norm_, train_UNet_Onset_VAT.py:113,124;
 * model/helper_functions.py:602-607) on flat buffers; *step = optimiser steps already taken.  skip (nullable): device int;
 * when *skip != 0 (a kernel of this step flagged its results invalid, see rv_lstm_fwd) the update is not applied. */
int rv_adam_step(float* p, const float* g, float* m, float* v, long n, const long* step, float lr0, long decay_steps,
                 float decay_rate, float beta1, float beta2, float eps, float grad_scale, const int* skip, void* stream);
int rv_counter_add(long* counter, long inc, const int* skip_if_set, void* stream);   /* skip_if_set nullable: no add while *skip != 0 */
int rv_clip_scale(float* g, long n, const float* total_norm, float max_norm, void* stream);
/* rv_adam_step with the optimiser options, all in the same pass: g is multiplied by grad_scale and by the clip
 * coefficient min(1, max_grad_norm / (*total_norm * grad_scale + 1e-6)) -- torch's clip_grad_norm_ BEFORE the step; 1 when
 * max_grad_norm <= 0 or total_norm is null; *total_norm = rv_reduce_mean(kind 3) of g as stored --, p is multiplied by
 * 1 - lr * weight_decay before the Adam update (torch.optim.AdamW), and ema (nullable) = ema_decay * ema + (1 - ema_decay) * p.
 * An element with zero gradient and zero moments keeps its p (torch skips tensors without a gradient; the only deviation: an
 * element of a touched tensor whose gradient has been exactly zero since step 1 is not decayed).  While *skip != 0 nothing is
 * written.  weight_decay = 0, max_grad_norm = 0, ema null: bit-identical to rv_adam_step. */
int rv_adamw_step(float* p, const float* g, float* m, float* v, long n, const long* step, float lr0, long decay_steps,
                  float decay_rate, float beta1, float beta2, float eps, float grad_scale, const int* skip, float weight_decay,
                  float max_grad_norm, const float* total_norm, float* ema, float ema_decay, void* stream);
int rv_swap_floats(float* a, float* b, long n, void* stream);   /* exchange two buffers in place */

/* ---- data feed: PianoRollAudioDataset.__getitem__ (model/dataset.py:35-69) for a whole batch on the device.
 * audio: int16 corpus; label, velocity (nullable): uint8 corpora ([steps, n_keys] rolls, label 3 = onset, 2 = frame,
 * 1 = offset); audio_begin / label_begin: DEVICE arrays of B element offsets (the host draws them with the reference's
 * RandomState rule).  out_audio [B, seq_len] = int16 / 32768; onset / offset (nullable) / frame / out_velocity (nullable)
 * [B, n_steps, n_keys] = (label == 3) / (label == 1) / (label > 1) / velocity / 128, all float32, bit-exact. */
int rv_crop_segments(const short* audio, const unsigned char* label, const unsigned char* velocity, const long* audio_begin,
                     const long* label_begin, int B, long seq_len, int n_steps, int n_keys, float* out_audio, float* onset,
                     float* offset, float* frame, float* out_velocity, void* stream);

/* Pitch-shift augmentation of the feed: rv_crop_segments with item b transposed by k_b semitones -- the audio resampled
 * by the polyphase definition of rv_resample (y[m] = sum_n x[a0 + n] 2^-15 h[m M - n L] over the samples of the item's TRACK, zero
 * beyond its two ends), the labels moved k keys and rescaled in time in integer arithmetic (reconvat_amd/augment.py has the rule).
 * audio [n_audio] int16, label / velocity [n_label] uint8; banks [n_bank] float32, 16-byte aligned: the banks [L, Kp] of every shift
 * (layout of rv_resample), concatenated at multiples of 4 floats; items: DEVICE array [B, 12] of longs per item: a0, t_begin, t_end
 * (corpus indices of the crop's first sample and of the track's first / one-past-last sample), L, M, F, Kp, bank offset in floats,
 * byte offset of the crop's first row in the label corpora, source rows that exist from there, k, 0.  L, M <= 128 within a factor
 * of 2 of each other, Kp <= 256; a row outside these limits yields NaN outputs for its item (never an out-of-range access).
 * Outputs as rv_crop_segments, none nullable, 16-byte aligned; n_keys a multiple of 4.  A k = 0 item with the bank [1, 0, 0, 0]
 * (L = M = 1, F = 0, Kp = 4) equals rv_crop_segments bit for bit.  Two launches, no atomics, allocation or synchronisation; every
 * output is one accumulator summed in a fixed order, so its bits do not depend on B or on the item's place in the batch. */
int rv_crop_segments_shift(const short* audio, long n_audio, const unsigned char* label, const unsigned char* velocity, long n_label,
                           const float* banks, long n_bank, const long* items, int B, long seq_len, int n_steps, int n_keys,
                           float* out_audio, float* onset, float* offset, float* frame, float* out_velocity, void* stream);

/* Acoustic augmentation of the feed (reconvat_amd/acoustics.py has the definition): one FIR per item plus white noise,
 *   y[b][m] = sum_{j < W} h[b][j] x[b][m + lead - j] + noise_b[m],  m < n,  x[b][.] read as zero outside [0, n) of its own row
 * (by a select: whatever lies next to the row in memory never enters a sum).  x, y: B rows of n floats, row strides x_stride /
 * y_stride >= n, not overlapping; h [B][W] float32, 16-byte aligned; W a multiple of 16 in [16, 8256], 0 <= lead < W,
 * 1 <= n < 2^31, 1 <= B <= 65535.  seed, amp: DEVICE arrays [B], both null for no noise; else noise_b[m] = float32(t) * amp[b],
 * t = (v & 0xFFFF) + (v >> 16) - 65535, v = lowbias32(seed[b] ^ lowbias32(m + 0x9E3779B9)), added with one float32 add.
 * The sum runs on the f32 matrix pipe (Toeplitz x Hankel, nothing formed in memory) in an order fixed by W, lead and m: the bits
 * of an output do not depend on B or on the item's place in the batch.  One launch, no atomics, allocation or synchronisation. */
int rv_fir_items(const float* x, long x_stride, const float* h, int W, int lead, const unsigned* seed, const float* amp, int B, long n,
                 float* y, long y_stride, void* stream);

/* ---- audio ingest: rational-ratio polyphase FIR resampling with the channel downmix fused in.
 *   y[m] = sum_n x[n] h[m M - n L],  x[n] = mean over the C channels of input frame n (zero outside the signal), L/M = sr_out/sr_in
 * x: [T_in, C] interleaved frames, in_dtype 0 = int16 (scale 2^-15), 1 = int32 (2^-31), 2 = float32; it is the slice
 * [in_offset, in_offset + T_in) of the signal and must hold every sample of the signal that outputs [m_start, m_start + n_out)
 * touch (frames outside the slice read as zero).  bank [L, Kp] float32, 16-byte aligned: bank[p][u] = h[p + (F - u) L], F = half / L,
 * Kp = taps per phase rounded up to a multiple of 4 (reconvat_amd/resample.py::design_filter builds it); L * Kp must not exceed
 * rv_resample_max_coeffs().  y: n_out samples, out_dtype 0 = float32, 1 = int16 (round-half-even of 32768 y, saturated); y[0] is
 * output m_start.  Each output is summed in one fixed order, so cutting a signal into several calls does not change a bit. */
long rv_resample_max_coeffs(void);
int rv_resample(const void* x, int in_dtype, long T_in, int C, long in_offset, const float* bank, int L, int M, int F, int Kp, void* y,
                int out_dtype, long m_start, long n_out, void* stream);

/* ---- additive synthesiser (reconvat_amd/synth.py has the definition): a table of partial rows rendered to audio.
 * rows [n_rows][8] 32-bit words per row: s, e (int: first sample and end sample of the note, e > s), inc, ph (uint32: phase step per
 * sample and start phase in units of 2^-32 turn), amp, dec (float32, dec >= 0: amplitude, decay rate per sample), A, R (int >= 1:
 * attack and release lengths in samples).  With t = n - s, for s <= n < e + R the row contributes
 *   amp * att * decay * rel * osc,   att = min(t + 1, A) / A,   decay = exp(-dec t),   rel = 1 for n < e, else ((e + R - n) / R)^2,
 *   osc = sin(2 pi theta / 2^32),   theta = (ph + inc t) mod 2^32 in exact uint32 wrap-around arithmetic,
 * and y[n] is the sum over all rows in ascending row order (one float64 accumulator per sample, float32 terms).
 * tile_ptr [n_tiles + 1], tile_rows [tile_ptr[n_tiles]] (CSR): tile j covers the absolute samples [1024 j, 1024 (j + 1)) and lists,
 * in ascending order, the rows whose [s, e + R) meets it; 0 <= n_tiles < 2^21.  y: n_out samples, out_dtype 0 = float32, 1 = int16
 * (round-half-even of 32768 y, saturated); y[0] is sample n0, and [n0, n0 + n_out) must lie inside the n_tiles tiles (else -1 and
 * nothing is written).  A tile_rows entry outside [0, n_rows) is skipped; a tile without rows writes zeros.  Every output is summed
 * in the list's order, so its bits depend neither on n_out nor on where the calls of a long render are cut.  One launch, no
 * atomics, allocation or synchronisation. */
int rv_synth_render(const unsigned* rows, int n_rows, const int* tile_ptr, const int* tile_rows, int n_tiles, long n0, long n_out,
                    void* y, int out_dtype, void* stream);

/* ---- score-to-recording alignment (reconvat_amd/align.py has the definition): banded dynamic time warping, batched.
 * desc [P][9] int64 ON THE DEVICE, one row per pair: N (recording frames, rows), M (score frames, columns), W (band width), then the
 * ELEMENT offsets of the pair's X [N][D] and Y [M][D] in feats, of lo [N] in lo, of cost [N][W] in cost, of dirs [N][W] in dirs and of
 * its output in out.  Row i of a pair owns the columns lo[i] .. lo[i] + W - 1, cut off at M; lo is non-decreasing with lo[0] = 0.
 * 1 <= W <= min(M, 8192), N + M <= 2^18.  The host does not read the table: every buffer comes with its length in elements, the
 * kernels check each pair's row against them and against max_n / max_nm / max_w (upper bounds of N, N + M and W over the pairs, which
 * also size the launch), and a pair that does not fit is not touched but for status -1 in its output header, if that is in range.
 * max_w > 8192 or max_nm > 2^18 is refused with -3.
 * rv_align_cost: cost[i][k] = rint(clip(1 - <x_i, y_(lo[i] + k)>, 0, 1) * 4095) as uint16, 0xFFFF where lo[i] + k >= M; the products
 *   run on the f32 matrix pipe, the epilogue is float32.  1 <= D <= 4096.
 * rv_align_dtw: D[0][0] = 2 c, D[i][j] = min(D[i-1][j-1] + 2 c, D[i-1][j] + c, D[i][j-1] + c) in uint32 over the cells of the band (a
 *   predecessor outside it is infinite); dirs[i][k] = 0 diagonal, 1 from (i-1, j), 2 from (i, j-1), 3 unreachable or start, ties to
 *   the lowest code (cells with lo[i] + k >= M are not written).  out: 4 + 2 N + 2 M int32 per pair: total = D[N-1][M-1] (uint32
 *   bits), path length, status, 0, then row_lo [N], row_hi [N] (lowest / highest column of the path per row), col_lo [M], col_hi [M].
 *   A band that does not connect the corners gives total 0xFFFFFFFF, length 0 and -1 in all four arrays.  One workgroup per pair
 *   (anti-diagonal wavefront, three diagonals in LDS), recurrence and backtrack in one launch; all-integer, deterministic.
 * Each is one launch, without atomics, allocation or synchronisation. */
int rv_align_cost(const long* desc, int P, int D, int max_n, int max_w, const float* feats, long n_feats, const int* lo, long n_lo,
                  unsigned short* cost, long n_cost, void* stream);
int rv_align_dtw(const long* desc, int P, int max_nm, int max_w, const int* lo, long n_lo, const unsigned short* cost, long n_cost,
                 unsigned char* dirs, long n_dirs, int* out, long n_out, void* stream);

/* ---- whole-song evaluation on the device: note decoding, the painted roll, the frame-metric counters.
 * Rolls are [T, 88] row-major, 1 <= T <= 2^24.  rv_eval_workspace_bytes(T): device scratch either call needs (0 for a T out of range).
 * rv_eval_decode: onsets / frames float32 (16-byte aligned, may alias), thresholds compared in float32 (x > threshold), rule 1 = rule1
 *   (a note needs the frame roll on at its onset), 2 = rule2.  A note starts where the thresholded onset roll rises and ends at the
 *   first frame where neither roll is on (T if none).  notes [max_notes, 3] int32 rows (t, pitch, end) ordered by (t, pitch); *count
 *   (device int) = notes in the rolls; rows past max_notes are not written (88 * ceil(T / 2) rows always suffice).  painted [T, 88]
 *   uint8 (4-byte aligned): 1 on [t, end) of every note.  Three launches on `stream`, no host synchronisation, deterministic.
 * rv_eval_frame_counts: ref / est uint8 rolls (8-byte aligned, non-zero = on) -> out[14] int64 (device): for the plain set and then
 *   for the chroma set the sums over frames of c, n_ref, n_est, min(n_ref, n_est) - c, max(0, n_ref - n_est), max(0, n_est - n_ref),
 *   max(n_ref, n_est) - c; plain c = |ref & est|, chroma c = sum over the 12 pitch classes (21 + key) % 12 of min(ref_k, est_k).
 *   Integer arithmetic only, partial sums added in a fixed order.
 * rv_eval_decode_clean: rv_eval_decode with note clean-up.  bridge_gap = g, 0..31: per pitch, a maximal run of
 *   inactive frames (neither roll on) of at most g frames that has an active frame directly before and directly after it counts as
 *   active -- the starts, and rule1's look at the frame roll, stay those of the unbridged rolls, and a run that touches frame 0 or
 *   frame T - 1 is never bridged.  min_frames = m, 1..32: a note runs from its start to the first inactive frame of the bridged
 *   activity (T if none) and is written and painted only if end - start >= m; *count counts the written notes.  Same workspace,
 *   same three launches, same order of the rows; rv_eval_decode is its (1, 0) case. */
long rv_eval_workspace_bytes(long T);
int rv_eval_decode(const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold, int rule, int* notes,
                   long max_notes, int* count, unsigned char* painted, void* workspace, long workspace_bytes, void* stream);
int rv_eval_decode_clean(const float* onsets, const float* frames, long T, float onset_threshold, float frame_threshold, int rule,
                         int min_frames, int bridge_gap, int* notes, long max_notes, int* count, unsigned char* painted, void* workspace,
                         long workspace_bytes, void* stream);
int rv_eval_frame_counts(const unsigned char* ref, const unsigned char* est, long T, long* out, void* workspace, long workspace_bytes,
                         void* stream);

/* ---- decoding thresholds swept over a grid: the integer counters behind note and frame precision / recall at every
 * pair of n_on onset and n_fr frame thresholds (1..32 each, float32 on the device, any order, duplicates allowed), for one song.
 * rv_eval_sweep_workspace_bytes: device scratch for the bit masks (0 for arguments out of range).
 * onsets / frames as for rv_eval_decode (may alias).  ref_notes [n_ref, 5] int32 rows (t, pitch, end, early, late) SORTED BY
 *   (pitch, t): the notes rv_eval_decode finds in the labels, plus the number of frames an estimate may end before (`early`) or
 *   after (`late`) `end` and still pass the offset test -- the caller evaluates its float64 tolerance once per reference note, the
 *   kernels stay all-integer.  n_ref may be 0.  ref_roll [T, 88] uint8 (4-byte aligned): the painted roll of those notes.
 * counts [n_on][n_fr][5] int64 (device): estimated notes; reference notes matched one-to-one to an estimate of the same pitch that
 *   starts within one frame (a maximum matching); the same with the offset test; frames painted by both; frames painted by the
 *   estimate -- each what rv_eval_decode + the host matcher + rv_eval_frame_counts give at that pair.  ref_totals [2] int64: n_ref,
 *   frames painted by the reference.  Two launches on `stream`, no host synchronisation, no atomics, deterministic.
 * rv_eval_sweep_clean: rv_eval_sweep with the note clean-up of rv_eval_decode_clean applied to the ESTIMATE -- one (min_frames,
 *   bridge_gap) per call, for the whole grid: the counters are those of the kept notes and their painted frames, and a candidate of the
 *   matching is a kept note with its end in the bridged activity.  ref_notes / ref_roll are handed over decoded (by convention
 *   without clean-up).  Same workspace, same two launches; rv_eval_sweep is its (1, 0) case. */
long rv_eval_sweep_workspace_bytes(long T, int n_on, int n_fr);
int rv_eval_sweep_clean(const float* onsets, const float* frames, long T, const float* onset_thresholds, int n_on,
                        const float* frame_thresholds, int n_fr, int rule, int min_frames, int bridge_gap, const int* ref_notes, long n_ref,
                        const unsigned char* ref_roll, long* counts, long* ref_totals, void* workspace, long workspace_bytes,
                        void* stream);
int rv_eval_sweep(const float* onsets, const float* frames, long T, const float* onset_thresholds, int n_on,
                  const float* frame_thresholds, int n_fr, int rule, const int* ref_notes, long n_ref, const unsigned char* ref_roll,
                  long* counts, long* ref_totals, void* workspace, long workspace_bytes, void* stream);

/* ---- Onsets&Frames baseline pieces (model/onset_frame_VAT.py:321-415,603-635) -------------------------------------
 * Bidirectional one-layer nn.LSTM(batch_first=True) recurrence (the `sequence_model` of Onset_Stack / Combine_Stack,
 * model/onset_frame_VAT.py:614,370-381,401-410).  The caller computes the input projections of every step with rv_gemm:
 *   xg [B,T,2,4H] = x W_ih^T + b_ih + b_hh   (direction-major halves, PyTorch gate order i,f,g,o)
 * and this entry runs the T sequential steps of both directions in ONE persistent launch (W_hh [4H,H] per direction held
 * in registers as MFMA operands, h exchanged through `out`, per-workgroup step counters in `flags`).
 * out [B,T,2H] (forward half | reverse half, as nn.LSTM returns it); gates [B,T,2,4,H] (activated) and cs [B,T,2,H]
 * are saved for the backward pass (both NULL = inference).  flags: rv_lstm_flag_bytes(H) bytes of device scratch, reset by
 * the call itself; the last int is non-zero afterwards if a workgroup gave up waiting (co-residency violated).  sticky_err
 * (nullable): ONE persistent device int per device that the kernels atomicOr a time-out into and never clear -- the host
 * reads and clears it at its own sync points, and rv_adam_step(skip = sticky_err) refuses to apply a poisoned step.
 * B <= 16 (the batch is the N side of one 16-wide MFMA tile); H in {384, 32}.  rv_lstm_bwd: dout [B,T,2H] -> dxg [B,T,2,4H]; dW_ih, dW_hh, db and dx are GEMMs / column sums
 * of dxg done by the caller. */
long rv_lstm_flag_bytes(int H);
int rv_lstm_fwd(const float* xg, const float* whh_fwd, const float* whh_rev, float* out, float* gates, float* cs, int* flags,
                int* sticky_err, int B, int T, int H, void* stream);
int rv_lstm_bwd(const float* dout, const float* whh_fwd, const float* whh_rev, const float* gates, const float* cs, float* dxg,
                int* flags, int* sticky_err, int B, int T, int H, void* stream);

/* nn.MaxPool2d((1,2)) over the frequency axis of an NHWC tensor x [rows, W, C] -> y [rows, W/2, C] fused with the
 * nn.Dropout(p) that follows it in ConvStack (model/onset_frame_VAT.py:336-343; p = 0 disables the drop).  code
 * [rows, W/2, C] bytes: bit 0 = the odd column was the max, bit 1 = kept.  Kept values are scaled by 1/(1-p).  The mask is a
 * counter hash of (seed, *epoch, index); epoch (nullable) is a device counter bumped per training step, which keeps the
 * draws fresh when the launch is replayed from a hipGraph. */
int rv_maxpool_w2_dropout_fwd(const float* x, float* y, unsigned char* code, long rows, int W, int C, float p, unsigned seed,
                              const long* epoch, void* stream);
int rv_maxpool_w2_dropout_bwd(const float* dy, const unsigned char* code, float* dx, long rows, int W, int C, float p,
                              void* stream);
/* nn.Dropout(p) (model/onset_frame_VAT.py:346-348).  Forward: code_in NULL, code_out receives the keep mask.  Backward:
 * pass the saved mask as code_in (seed unused) and dy as x. */
int rv_dropout(const float* x, float* y, unsigned char* code_out, const unsigned char* code_in, long n, float p, unsigned seed,
               const long* epoch, void* stream);

/* ---- Thickstun CNN baseline (model/Thickstun_model.py) in its window-sharing form ------------------------------------------
 * The reference cuts the padded spectrogram into one 229 x 25 window per frame (:57-59) and runs CNN_freq, CNN_time and the
 * linear layer on that batch of windows (:30-35).  Here z2 = relu(CNN_freq) is computed once per padded frame and kept
 * channels-last, z2 [B, 51, Tin + 2*pad, 128]; z3 = relu(CNN_time) is a GEMM over a Hankel view of z2, z3 [B, T, 51, N]
 * with T = Tin + 2*pad - 24.  (pad = 12: run_on_batch's F.pad; pad = 0, Tin = 25: forward() on ready-made windows.)
 *
 * rv_thick_freq_fwd (:30, torch.relu(self.CNN_freq(x.unsqueeze(1)))): x [B, Tin, 229] time-major, w [128][128] (channel, tap:
 *   the checkpoint's [128,1,128,1]), bias [128]; the 2*pad zero frames become relu(bias).
 * rv_thick_freq_bwd (autograd of :30): dw [128][128], db [128] (accumulate: += ) from dz2, with the ReLU mask of z2 applied on
 *   load; partial sums per 8 frames are added in a fixed order (no float atomics).  workspace: rv_thick_freq_bwd_workspace_bytes.
 * rv_thick_tconv_fwd (:32, torch.relu(self.CNN_time(z2))): wj [25][N][128] = rv_pack_weights(plain, taps = 25, kdim = N,
 *   ndim = 128, s_k = 3200, s_n = 25) of the checkpoint's [N,128,1,25]; bias [N]; N % 128 == 0; 16-byte aligned operands.
 * rv_thick_linear_dz (autograd of :34, the gradient of self.linear's input through the ReLU of :32): dy [M, N] logit gradients,
 *   wt [K, N] the linear weight transposed and in z3's feature order, z3 / dz3 [M, K]; dz3 = z3 > 0 ? dy @ wt^T : 0.
 *   N <= 96, N % 4 == 0, K % 4 == 0. */
int rv_thick_freq_fwd(const float* x, const float* w, const float* bias, float* z2, int B, int Tin, int pad, void* stream);
long rv_thick_freq_bwd_workspace_bytes(int B, int Tin, int pad);
int rv_thick_freq_bwd(const float* dz2, const float* z2, const float* x, float* dw, float* db, int B, int Tin, int pad, int accumulate,
                      void* workspace, long workspace_bytes, void* stream);
int rv_thick_tconv_fwd(const float* z2, const float* wj, const float* bias, float* z3, int B, int T, int N, void* stream);
int rv_thick_linear_dz(const float* dy, const float* wt, const float* z3, float* dz3, long M, long K, int N, void* stream);

/* ---- note velocities (reconvat_amd/velocity.py has the definition) --------------------------------------------
 * A head shared by the 88 keys: the cell (b, t, p) sees x[8 j + k] = spec[b][clamp(t - 1 + j, 0, T - 1)][table[p][k]] (0 where the
 * table says -1), j = 0..3, k = 0..7, and x[32] = p / 88; v = sigmoid(b2 + sum_h w2[h] sigmoid(b1[h] + sum_i w1[h][i] x[i])).
 * spec [B, T, n_bins] float32 (n_spec floats; n_bins <= 384); table [88][8] int32 ON THE HOST: every entry is checked against
 * [-1, n_bins) before anything is launched; params: w1 [32][33], b1 [32], w2 [32], b2 = 1121 floats (n_params).  Device buffers are
 * 4-byte aligned.
 * rv_velocity_roll: out [B, T, 88] float32 (n_out floats), every cell.  One launch.
 * rv_velocity_loss_grad: target, mask [B, T, 88] float32 (n_cells floats each) -> loss[0] = sum m (v - target)^2 / sum m and
 *   grad [1121] (n_grad floats) = its gradient in params; both 0 when sum m = 0.  Only cells with m != 0 are evaluated.  Two launches:
 *   per-workgroup partial sums in a fixed order into workspace (rv_velocity_workspace_bytes, 0 for arguments out of range), then a
 *   float64 fold in workgroup order.  No atomics: the same bits on every run.  spec gets no gradient.
 * rv_eval_note_velocity: onsets, velocity [T, 88] float32, notes [n][3] int32 rows (t, pitch, end) on the device as
 *   rv_eval_decode_clean writes them -> out[i] (n_out >= n floats) = the mean of velocity[s][pitch] over t <= s < min(end, T) with
 *   onsets[s][pitch] > onset_threshold, summed in float64 in ascending s and rounded once; 0 without such a frame.  n = 0 launches
 *   nothing. */
int rv_velocity_roll(const float* spec, long n_spec, int B, int T, int n_bins, const int* table, const float* params, long n_params,
                     float* out, long n_out, void* stream);
long rv_velocity_workspace_bytes(int B, int T);
int rv_velocity_loss_grad(const float* spec, long n_spec, int B, int T, int n_bins, const int* table, const float* params, long n_params,
                          const float* target, const float* mask, long n_cells, float* loss, float* grad, long n_grad, void* workspace,
                          long workspace_bytes, void* stream);
int rv_eval_note_velocity(const float* onsets, const float* velocity, long T, float onset_threshold, const int* notes, long n, float* out,
                          long n_out, void* stream);

/* ---- Viterbi note decoding: per key a three-state hidden Markov model (0 = OFF, 1 = ONSET, 2 = SUSTAIN) over the two
 * posteriorgrams, for G parameter sets at once.  1 <= T <= 2^20, 1 <= G <= 16; rv_hmm_workspace_bytes(T, G): device scratch the call
 * needs (0 for arguments out of range).
 * rv_hmm_decode: onsets / frames [T, 88] float32 as for rv_eval_decode (16-byte aligned, may alias), quantised once to
 *   q(x) = 0 unless x >= 0 (NaN, negatives), else min(255, floor(256 x)) in float32.  tables (DEVICE) [G][6][256] uint16 = EO[OFF],
 *   EO[ONSET], EO[SUSTAIN], EF[OFF], EF[ONSET], EF[SUSTAIN]: state s costs EO[s][q(onset)] + EF[s][q(frame)] at a frame; every value
 *   is legal.  trans (HOST) [G][12] int32 = init[3], A[3][3] row-major with A[from][to]; an entry is -1 (forbidden) or in 0..65535,
 *   init[0] and A[0][0] must be allowed; all of it is checked before anything is launched.
 *   alpha_0(s) = init[s] + E_0(s), alpha_t(s) = min_s' (alpha_{t-1}(s') + A[s'][s]) + E_t(s) in exact 64-bit integers; the
 *   back-pointer of (t, s) is the LOWEST s' attaining the minimum, the last state the lowest s attaining min_s alpha_{T-1}(s).
 *   -> states [G][T][88] uint8, the path of every key under every set, and cost [G][88] int64 (device, 8-byte aligned), that minimum.
 *   A null pointer, T or G out of range, a trans entry out of range, a forbidden init[0] or A[0][0], or a short workspace returns
 *   non-zero, names rv_hmm_decode in rv_last_error and launches nothing.  Parallel over time (chunks of 64 frames, the recurrence as
 *   a product in the (min, +) semiring); six launches on `stream`, no allocation, no host synchronisation, no atomics: the same
 *   bits on every run.  `states` holds back-pointers between the launches. */
long rv_hmm_workspace_bytes(long T, int G);
int rv_hmm_decode(const float* onsets, const float* frames, long T, const unsigned short* tables, const int* trans, int G,
                  unsigned char* states, long* cost, void* workspace, long workspace_bytes, void* stream);

/* ---- sub-frame note onsets (the definition: reconvat_amd/onset_time.py).  Per note (key p in 0..87, onset frame t in
 * 0..2^22 - 1) the amplitudes A[m][q] of the key's harmonics q = 1..8 (valid iff q f0(p) <= 7200 Hz) in Hann windows of 512 samples at
 * the 49 positions 512 t - 768 + 32 m of audio [T] (float32, 1 <= T < 2^31, zero outside [0, T)), the rise d[m][q] = A[m + 1][q] -
 * A[m - 1][q], per valid harmonic the first m in 1..47 with the largest rise, and the lower median k of those:
 *   out_sample[i] = clamp(512 t - 768 + 32 k - lead, 0, T - 1) (int32 [n]);  out_amp (float32 [n][49][8], or null) = A, 0 for the
 *   invalid harmonics.
 * table (DEVICE, 16-byte aligned) [88][8][2][512] float32 = window x (cos, -sin), as onset_time.basis_table() builds it; notes (DEVICE)
 * int32 [n][2] = (key, frame): a row outside the ranges above gets out_sample = -1 and zero amplitudes, and the table is not read for
 * it.  Every other buffer 4-byte aligned.  0 <= lead < 2^30.  One workgroup per note on v_mfma_f32_16x16x4_f32 (512 MFMAs, each from a
 * zero accumulator: four products in float32, their sums in float64; A is rounded to float32 once, d is a float32 difference), one
 * launch per 2^20 notes, n = 0 launches nothing; no allocation, no host synchronisation, no atomics; a note's results do not depend on
 * n or on its place in the list.  A null pointer, a misaligned buffer, T, n or lead out of range returns non-zero, names
 * rv_onset_refine in rv_last_error and launches nothing. */
int rv_onset_refine(const float* audio, long T, const float* table, const int* notes, long n, int lead, int* out_sample, float* out_amp,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
