/*
 * floodunet.h -- C ABI of libfloodunet.so: the MI355X (gfx950) UNet segmentation training
 * path of the FloodPlanet st_water_seg pipeline.
 *
 * The reference has no native layer: its hot path is torch.nn modules driven by Lightning
 * ("C ABI (new; nothing to mirror in the reference)").  Each entry
 * point below therefore cites the *Python* call it replaces (paths relative to the
 * reference checkout):
 *
 *   fu_create / fu_destroy      UNet(n_channels, n_classes, bilinear)        st_water_seg/models/unet.py:80-98
 *                               built by WaterSegmentationModel._build_model st_water_seg/models/water_seg_model.py:79-85
 *   fu_param_info / fu_bind_*   UNet.state_dict() / .parameters()            (state-dict keys of unet.py:6-98)
 *   fu_forward[_srcs]           UNet.forward (+ the early-fusion concat)     st_water_seg/models/unet.py:100-111, ef_model.py:28-44
 *                               (train: nn.BatchNorm2d batch statistics; eval: running statistics,
 *                                water_seg_model.py:92-96)
 *   fu_loss_ce                  nn.CrossEntropyLoss(ignore_index) + nan_to_num + argmax + metric counts
 *                                                                            st_water_seg/models/water_seg_model.py:40,103-113
 *   fu_loss_ce_weighted         (new) nn.CrossEntropyLoss(weight, ignore_index, label_smoothing) on the same path
 *   fu_loss_ce_focal            (new) the same with focal modulation (1 - p[t])^gamma of every pixel's term
 *   fu_loss_ce_region           (new) any of the three plus a soft Dice / Jaccard / Tversky region term over all classes
 *   fu_label_class_counts       (new) class frequencies of resident label rasters, for "balanced" weights
 *   fu_label_box_counts         (new) the label content of every box of a table, for content-aware tile sampling
 *   fu_scene_valid_mask         (new) which pixels of a resident scene hold data, on its output grid, for infer --nodata
 *   fu_mask_box_counts          (new) the valid pixels of every crop box of such a mask, so all-fill crops are not forwarded
 *   fu_tiff_unpack              (new) decoded TIFF segments -> the fp32 band raster, on the device: predictor, byte swap,
 *                               tiles, band choice and conversion in one launch (tifffile.imread + the host's astype)
 *   fu_tiff_lzw_decode /        (new) the host's LZW and PackBits decoders in front of it
 *   fu_tiff_packbits_decode
 *   fu_tiff_pack                (new) the inverse for the rasters infer writes: a strided device raster -> the byte buffer
 *                               a TIFF writer deflates -- planes, tiles or strips, edge padding, predictor -- in one launch
 *   fu_map_overviews            (new) the overview pyramid of such a raster: mode / mean / any over 2 x 2 blocks, six levels
 *                               per launch from one read of the base (gdaladdo's role, on the device)
 *   fu_backward[_block]         loss.backward() issued by Lightning's automatic optimisation
 *                                                                            st_water_seg/fit.py:95-97
 *   fu_adam_step                optim.Adam(self.parameters(), lr).step()     st_water_seg/models/water_seg_model.py:198-205
 *   fu_augment                  torchvision hflip / vflip / rotate of sample_transforms + apply_transforms
 *                                                                            st_water_seg/datasets/base_dataset.py:494-555
 *   fu_scene_train_tiles        crop + normalise + pad + label decode + augment of resident scenes in one pass (new)
 *   fu_scene_train_tiles_ex     (new) the same pass with per-band gain / bias / counter-based noise and a per-sample zoom
 *   fu_block_param_range        (new) gradient bucket of one backward block, for RCCL all-reduce overlap
 *   fu_dp_* / fu_allreduce_*    (new) the bucketed gradient all-reduce itself, RCCL resolved at run time
 *   fu_op_*                     single operators for per-op parity tests (conv2d, batch_norm, max_pool2d,
 *                               upsample, cross_entropy as used in unet.py / water_seg_model.py)
 *
 * Conventions
 *   - every pointer argument that carries tensor data is a DEVICE pointer owned by the caller
 *     (borrowed for the duration of the call); the context owns workspaces and saved activations.
 *   - all work is enqueued on the hipStream_t passed as `stream` (void* so that this header
 *     needs no HIP include); nothing synchronises the device unless documented.
 *   - every function returns FU_OK (0) or an error code; fu_last_error() returns a thread-local
 *     message.  No C++ exception crosses this boundary.
 *   - one context per device per process; calls on one context must be serialised by the caller.
 *     Contexts are independent of each other: no launch depends on which device launched first or on
 *     what a call on another context left behind (per-device launch facts are kept per device index,
 *     exact-sync and fp16 loss-scale state per context).
 */
#ifndef FLOODUNET_H_
#define FLOODUNET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FU_ABI_VERSION 5
#define FU_MAX_ENCODERS 6

typedef struct fu_ctx fu_ctx;
typedef void* fu_stream; /* hipStream_t */

enum fu_status {
  FU_OK = 0,
  FU_ERR_INVALID = 1,     /* bad argument / shape */
  FU_ERR_HIP = 2,         /* a HIP runtime call failed */
  FU_ERR_STATE = 3,       /* call order violated (e.g. backward before forward) */
  FU_ERR_UNSUPPORTED = 4  /* valid request this build does not implement */
};

enum fu_precision {
  FU_F32 = 0, /* fp32 storage, fp32 MFMA (exact fmaf chains): the 1e-4 parity mode */
  FU_BF16 = 1, /* bf16 activations/weights, fp32 accumulate, fp32 master weights / BN / loss */
  FU_F16 = 2   /* IEEE fp16 activations / weights / gradient maps on the matrix cores (v_mfma_f32_32x32x16_f16, the bf16
                * rate), fp32 accumulation, fp32 master weights, BN statistics, loss and Dice reductions (BASELINE configs[3]:
                * "mixed fp16 with fp32 Dice reduction").  The gradient maps carry a power-of-two loss scale chosen on the
                * device from max|dL/dlogits| at the start of every backward and removed where parameter gradients are
                * written: the flat gradient buffer holds true gradients, no caller-side GradScaler is needed (a step whose
                * gradients overflowed all the same is skipped on the device: fu_fp16_guard_state).  Inputs are
                * expected in fp16's range (the reference scales every sensor to [0, 1], datasets/floodplanet.py:347-525). */
};

enum fu_loss_kind {
  FU_LOSS_CE = 0,      /* softmax cross entropy with ignore_index (the reference's loss) */
  FU_LOSS_BCE_DICE = 1 /* north-star extension: per-pixel BCE + soft Dice on class 1 (parity unpinned) */
};

typedef struct fu_config {
  int32_t struct_size;   /* = sizeof(fu_config) */
  int32_t n_channels;    /* sum of in_channels.values() (water_seg_model.py:81-84) */
  int32_t n_classes;     /* 3 for FloodPlanet (datasets/floodplanet.py:63) */
  int32_t base_channels; /* 64 = UNet; other widths = UNetEncoder/Decoder(base_feat_channels) */
  int32_t bilinear;      /* 1 = nn.Upsample(bilinear, align_corners=True) (default), 0 = ConvTranspose2d */
  int32_t max_batch;     /* workspace is sized for this many tiles */
  int32_t height, width; /* tile size (any size >= 16; odd sizes take the F.pad path of unet.py:57-62) */
  int32_t precision;     /* enum fu_precision */
  int32_t device;        /* HIP device ordinal */
  /* Late fusion (lf_model.py:29-92, feat_fusion='concat_conv'): n_encoders >= 1 builds one UNetEncoder per input over
   * consecutive channel windows of the input (enc_channels[e] channels each, summing to n_channels, in the order
   * lf_model.py:58-76 gathers them), five 1x1 fusion convs (n_encoders*fs -> fs at fs = 64,128,256,512,512 for
   * base 64) and one UNetDecoder.  Parameter names: encoders.<e>.*, concat_convs.<level>.*, decoder.* (the host side
   * maps <e> to the reference's ModuleDict keys).  0 = the plain UNet.  Needs bilinear = 1. */
  int32_t n_encoders;
  int32_t enc_channels[FU_MAX_ENCODERS];
} fu_config;

/* ---- lifetime ---------------------------------------------------------------------------- */
int fu_abi_version(void);
const char* fu_last_error(void);
int fu_create(const fu_config* cfg, fu_ctx** out);
int fu_destroy(fu_ctx* ctx);

/* ---- parameter table (canonical = reference state_dict order) ----------------------------- */
int fu_num_params(const fu_ctx* ctx);        /* trainable tensors (74 for the bilinear net) */
int64_t fu_total_param_elems(const fu_ctx* ctx);
/* name: state-dict key without the Lightning "model." prefix; shape: up to 4 dims (OIHW for convs);
 * flat_offset: element offset inside the flat parameter / gradient buffers. */
int fu_param_info(const fu_ctx* ctx, int index, const char** name, int32_t* ndim, int64_t shape[4],
                  int64_t* flat_offset);
int fu_num_bn(const fu_ctx* ctx);            /* BatchNorm2d layers (18) */
int64_t fu_total_bn_channels(const fu_ctx* ctx);
/* name: key prefix of the BN module ("inc.double_conv.1"); offset into the flat running buffers */
int fu_bn_info(const fu_ctx* ctx, int index, const char** name, int32_t* channels, int64_t* flat_offset);

/* Bind caller-owned flat device buffers.  params/grads: fp32 [fu_total_param_elems];
 * running_mean/running_var: fp32 [fu_total_bn_channels]; num_batches_tracked: int64 [fu_num_bn].
 * grads may be NULL for inference-only use. */
int fu_bind_buffers(fu_ctx* ctx, float* params, float* grads, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked);
/* Tell the context the bound parameters were modified by someone else (torch optimiser,
 * load_state_dict): device-side packed copies are refreshed on the next forward. */
int fu_params_changed(fu_ctx* ctx);

/* ---- the hot path -------------------------------------------------------------------------- */
/* x: fp32 NCHW [batch, n_channels, height, width].  logits_out: fp32 NCHW [batch, n_classes, H, W] or NULL.
 * training != 0: batch-statistics BN, running buffers updated, activations kept for backward. */
int fu_forward(fu_ctx* ctx, const float* x, int batch, int training, float* logits_out, fu_stream stream);

/* The same with the input given as n_src (<= 8) fp32 NCHW tensors [batch, src_channels[k], H, W] that the model sees
 * side by side along the channel axis (sum src_channels = n_channels): the reference's
 * `torch.concat([images, dem, slope, ...], dim=1)` (ef_model.py:28-44) / stacked sensors (BASELINE configs[4]) without the
 * concatenated copy -- the channels are gathered by the NCHW -> NHWC conversion the first conv needs anyway.  srcs /
 * src_channels: HOST arrays. */
int fu_forward_srcs(fu_ctx* ctx, const float* const* srcs, const int32_t* src_channels, int n_src, int batch,
                    int training, float* logits_out, fu_stream stream);

/* Loss on the logits of the last fu_forward.  target: int64 [batch, H, W].
 * loss_out: device fp32 scalar (mean over non-ignored pixels; 0 when every pixel is ignored).
 * confusion_out: optional device int64 [n_classes*n_classes], M[t*n_classes+p] over non-ignored pixels
 * (argmax prediction), ADDED to the existing contents.  n_valid_out: optional device int64 scalar. */
int fu_loss_ce(fu_ctx* ctx, const int64_t* target, int ignore_index, float* loss_out, int64_t* confusion_out,
               int64_t* n_valid_out, fu_stream stream);
/* Class-weighted, label-smoothed cross entropy (added within ABI 5: purely additive, no version bump; the reference has no
 * such loss -- the specification is torch.nn.functional.cross_entropy(logits, target, weight, ignore_index=...,
 * label_smoothing=...)).  With p = softmax(z), w = class_weight, W = sum_c w[c], eps = label_smoothing, C = n_classes and
 * the sums over the valid pixels (target != ignore_index, 0 <= target < C):
 *   loss = [(1 - eps) * sum_i w[t_i] (lse(z_i) - z_i[t_i]) + (eps / C) * sum_i sum_c w[c] (lse(z_i) - z_i[c])] / D,
 *   D = sum_i w[t_i];  dL/dz_k = [(1 - eps) w[t] (p_k - [k == t]) + (eps / C) (p_k W - w[k])] / D.
 * D == 0 (every pixel ignored, or only zero-weight classes present): loss 0 and a zero gradient, where torch gives NaN.
 * class_weight_dev: fp32 [n_classes] on the device, or NULL = all ones.  The call TRUSTS that memory: the weights must be
 * finite and >= 0, which only a host-side copy could check -- the caller validates them where they come from (HipUNet
 * does).  label_smoothing must lie in [0, 1).  loss_out / confusion_out / n_valid_out as for fu_loss_ce (the counts are
 * pixels, not weights); weight_sum_out: optional device fp32 scalar = D.  Reductions as fu_loss_ce: fp32 per-workgroup
 * partials, a fixed fp64 tree, no floating-point atomics; in exact data-parallel mode the partials are summed over the ranks
 * so that D is global.  All-ones weights (or NULL) with label_smoothing 0 give fu_loss_ce's loss, counts and gradient bit
 * for bit.  State rules of fu_loss_ce. */
int fu_loss_ce_weighted(fu_ctx* ctx, const int64_t* target, int ignore_index, const float* class_weight_dev,
                        float label_smoothing, float* loss_out, int64_t* confusion_out, int64_t* n_valid_out,
                        float* weight_sum_out, fu_stream stream);
/* Focal cross entropy (Lin et al., "Focal Loss for Dense Object Detection"), class-weighted (added within ABI 5: purely
 * additive, no version bump; the reference has no such loss -- the specification is tests/tools/focal_ref.py).  With
 * p = softmax(z), q = p[t], u = 1 - q, w = class_weight, gamma = focal_gamma and the sums over the valid pixels:
 *   loss = sum_i w[t_i] u_i^gamma (-log q_i) / D,   D = sum_i w[t_i];
 *   dL/dz_k = w[t] (p_k - [k == t]) m / D,          m = u^gamma - gamma q u^(gamma-1) log q.
 * u is formed as the other classes' exponentials over the total and log q as (z_t - max) - log(sum) (log1p of the others'
 * sum where the target holds the maximum), so neither loses digits for q near 1.  u == 0 (the others' exponentials
 * underflow in fp32) with gamma > 0: the pixel contributes loss 0 and gradient 0, never a NaN.  D == 0: loss 0 and a
 * zero gradient, as fu_loss_ce_weighted.  focal_gamma must be finite and >= 0.  focal_gamma == 0 runs
 * fu_loss_ce_weighted's kernels with label_smoothing 0: the same bits (and with NULL weights fu_loss_ce's).  Label smoothing
 * has no agreed focal form and no argument here.  Every other argument, the counts (pixels, not weights), the
 * reductions, exact data-parallel mode and the state rules: as fu_loss_ce_weighted. */
int fu_loss_ce_focal(fu_ctx* ctx, const int64_t* target, int ignore_index, const float* class_weight_dev,
                     float focal_gamma, float* loss_out, int64_t* confusion_out, int64_t* n_valid_out,
                     float* weight_sum_out, fu_stream stream);
/* Cross entropy plus a soft Dice / Jaccard / Tversky region term over all classes (added within ABI 5: purely additive, no
 * version bump; the reference has no such loss -- the specification is tests/tools/region_ref.py).  With p = softmax(z),
 * y_ik = [t_i == k], the sums over the valid pixels of fu_loss_ce, lambda = region->weight, s = region->smooth:
 *   I_k = sum_i p_ik y_ik,  P_k = sum_i p_ik,  T_k = sum_i y_ik,
 *   TI_k = (I_k + s) / (I_k + alpha (P_k - I_k) + beta (T_k - I_k) + s)                  (the soft Tversky index)
 *   R = sum_{k in K} (1 - TI_k) / |K|,  K = the classes 0..n_classes-1 without ignore_index;   loss = CE + lambda R.
 * alpha = beta = 0.5 is soft Dice (with s = 0.5 the (2I + 1) / (P + T + 1) of fu_loss_bce_dice, for every class), alpha =
 * beta = 1 soft Jaccard; alpha weighs false positives, beta false negatives.  With Num_k and Den_k the fraction's parts,
 *   d(lambda R)/dz_ij = lambda p_ij (g_ij - sum_k g_ik p_ik),   g_ik = A_k where t_i == k, else B_k,
 *   A_k = -(alpha (P_k - I_k) + beta (T_k + s)) / (|K| Den_k^2),   B_k = alpha Num_k / (|K| Den_k^2)   (0 outside K).
 * CE is one of the three forms above, unchanged, with its own normaliser: class_weight_dev == NULL, label_smoothing == 0
 * and focal_gamma == 0 select fu_loss_ce's kernels; focal_gamma > 0 fu_loss_ce_focal's (rejected together with
 * label_smoothing != 0); anything else fu_loss_ce_weighted's.  loss_out, the counts and the state rules are that form's;
 * weight_sum_out is written by the weighted and focal forms only.  Class weights do not enter R.
 * Zero rules: invalid pixels get a gradient of exactly 0; with no valid pixel R = 0 exactly (TI_k = s / s) and the gradient
 * is 0.  The region term follows pixel validity, NOT the CE's summed weight D: a batch whose valid pixels all carry class
 * weight 0 has CE 0 and still a live region term.
 * region: HOST struct.  weight must be finite and >= 0, alpha and beta finite and >= 0 with alpha + beta > 0, smooth finite
 * and > 0, n_classes >= 2 when weight > 0; a rejected call launches nothing.  region == NULL or weight == 0 launches nothing
 * new: loss, counts, D and gradient are then fu_loss_ce's, fu_loss_ce_weighted's or fu_loss_ce_focal's bit for bit.
 * region_out: optional device fp32 [1 + n_classes]: [0] = R (before lambda), [1 + k] = TI_k, 1.0 for the class equal to
 * ignore_index; written only when weight > 0.
 * Reductions: passes of their own after the CE's -- fp32 per-workgroup partials of I, P and T (at most 4096 / (3 KMAX) workgroups
 * of 256 pixels per trip, KMAX = n_classes up to 4, else 8), a fixed fp64 tree, no floating-point atomics: the same bits on every run.  The coefficients A, B and
 * lambda stay on the device for the gradient pass (training forwards only), which adds to the stored CE gradient.  In exact
 * data-parallel mode the partials are summed over the ranks: I, P, T, R, region_out and the coefficients are the whole
 * batch's on every rank. */
typedef struct fu_region_loss { float weight, alpha, beta, smooth; } fu_region_loss;
int fu_loss_ce_region(fu_ctx* ctx, const int64_t* target, int ignore_index, const float* class_weight_dev,
                      float label_smoothing, float focal_gamma, const fu_region_loss* region, float* loss_out,
                      int64_t* confusion_out, int64_t* n_valid_out, float* weight_sum_out, float* region_out,
                      fu_stream stream);
/* North-star extension (no reference counterpart; specification = oracle/unet_oracle.py:bce_dice_loss):
 * BCE on p = softmax(z)[1] vs [target == 1] + dice_weight * soft Dice, over target != ignore_index, fp32 wave-shuffle
 * reductions; stores its logits gradient for fu_backward like fu_loss_ce.  log(1 - p) is the logsumexp over the other classes
 * (with their own maximum) minus the logsumexp over all: finite, with a gradient row that sums to zero, however far class 1
 * leads.  Every pixel ignored: loss 0 and a zero gradient. */
int fu_loss_bce_dice(fu_ctx* ctx, const int64_t* target, int ignore_index, float dice_weight, float* loss_out,
                     fu_stream stream);

/* Backward of everything enqueued by the last training fu_forward.  dlogits: fp32 NCHW gradient w.r.t.
 * the logits, or NULL to use the gradient of the last fu_loss_* call.  Gradients are written
 * (not accumulated) into the bound flat gradient buffer. */
int fu_backward(fu_ctx* ctx, const float* dlogits, fu_stream stream);
/* The weight-gradient chain of every conv (wgrad, slab reduce, transpose) runs on a context-owned side stream,
 * concurrently with the data-gradient / BatchNorm-backward chain on the caller's stream, which does not wait for it
 * anywhere inside a backward (every conv has its own bias-gradient partials; the side stream only ever waits for the
 * caller's); fu_backward joins the two before it returns its work to the caller's stream order, fu_backward_block at
 * the end of every block (the block's gradients are then final for a bucketed all-reduce).  After a join every launch
 * queued on the side stream so far has finished in `stream` order, and only then may the next backward start: one that
 * finds chains unjoined (mode 2 without fu_backward_join) joins them itself before its first launch.  mode 0 keeps everything on the caller's stream (the default
 * when the environment variable FU_NO_SIDE_STREAM is set at fu_create, for bilinear = 0 and in fp32 mode); mode 1
 * (default) as described; mode 2: fu_backward_block does not join -- the caller calls fu_backward_join(stream) before
 * it consumes gradients on `stream` (e.g. once per all-reduce bucket instead of once per block). */
int fu_set_side_stream(fu_ctx* ctx, int mode);
/* The upstream gradient autograd hands to `loss.backward()` (fit.py:95-97) as a device scalar: the next backward
 * multiplies the stored loss gradient (dL/dlogits of the last fu_loss_* call) by *scale_dev on its way into the head --
 * once, on the logits gradient, instead of on every parameter gradient, and without a host read.  The stored gradient is
 * not modified: repeating the call replaces the factor, repeating the backward (retain_graph) repeats the result; the
 * factor is dropped by the next fu_forward / fu_loss_* call. */
int fu_scale_loss_grad(fu_ctx* ctx, const float* scale_dev, fu_stream stream);
int fu_backward_join(fu_ctx* ctx, fu_stream stream);
/* Mode 2, without stalling the compute stream: `waiter` (any other stream, e.g. the one a collective is launched from) waits
 * for every gradient-producing launch enqueued so far -- the work on `stream` and the weight-gradient chain on the side
 * stream.  Neither `stream` nor the side stream waits for anything: the backward blocks that follow start at once, the
 * bucket's all-reduce starts when both chains have reached this point.  (fu_allreduce_begin does the same internally.)
 * The last bucket still needs fu_backward_join before the optimizer step reads the gradients on `stream`. */
int fu_backward_fence(fu_ctx* ctx, fu_stream stream, fu_stream waiter);

/* The same, one block at a time in backward order: block 0 = outc, 1..4 = up4..up1, 5..8 = down4..down1,
 * 9 = inc.  After block k returns, the gradient range fu_block_param_range(k) is final on `stream`. */
int fu_num_blocks(const fu_ctx* ctx);
int fu_backward_block(fu_ctx* ctx, int block, const float* dlogits, fu_stream stream);
int fu_block_param_range(const fu_ctx* ctx, int block, int64_t* flat_offset, int64_t* numel);

/* torch.optim.Adam semantics (water_seg_model.py:198-205) on the bound flat buffers.  The moments are CALLER-owned
 * flat fp32 device buffers [fu_total_param_elems] in parameter order, zero-initialised by the caller (the state of
 * torch.optim.Adam: exp_avg, exp_avg_sq); they outlive the context, so re-creating a context for another tile size or
 * a larger batch does not reset the optimiser (ABI 2 kept them inside the context).  fu_adam_step without bound moments
 * returns FU_ERR_STATE.  step is 1-based.  grad_scale multiplies the gradient first (1/world_size after a sum
 * all-reduce).  The scalars are doubles, formed and rounded to float exactly as torch.optim.Adam forms its Python
 * scalars; every operation of the update rounds on its own in ATen's order, so that with identical inputs the result
 * is torch's. */
int fu_bind_adam_state(fu_ctx* ctx, float* exp_avg, float* exp_avg_sq);
int fu_adam_step(fu_ctx* ctx, double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                 fu_stream stream);
int fu_adam_state(fu_ctx* ctx, float** exp_avg, float** exp_avg_sq); /* the bound pointers (NULL when none) */
/* FU_F16 only: the device-side loss scale follows max|dL/dlogits|, but a layer deep in the chain (a BatchNorm with a tiny
 * variance) can still overflow an fp16 gradient map.  fu_adam_step[_dev] therefore checks the gradient buffer on the device;
 * if a value is not finite the update of that step is left out entirely (parameters and moments untouched) and the next
 * backward scales the loss by a further 1/2 (taken back by one every 64 clean steps) -- what a GradScaler does, without a
 * host read.  This call reads the counters (it synchronises the device): steps skipped so far, current back-off exponent. */
int fu_fp16_guard_state(fu_ctx* ctx, int64_t* skipped_steps, int32_t* backoff_exponent);
/* The same update for a CAPTURED step (hipGraph): the seven float scalars of the kernel -- which depend on the step count --
 * are read from device memory, so one captured launch serves every replay.  fu_adam_scalars forms them on the host exactly
 * as fu_adam_step does (out[7]: 1-beta1, beta2, 1-beta2, sqrt(bias_correction2), eps, -lr/bias_correction1, grad_scale);
 * the caller copies them to scalars_dev before each replay.  All entry points of the hot path enqueue work only (no
 * allocation, no synchronisation, events and the side stream fork and re-join inside fu_backward), so a caller may capture
 * fu_forward + fu_loss_* + fu_backward + fu_adam_step_dev on one stream into a graph and replay it. */
int fu_adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, float out[7]);
int fu_adam_step_dev(fu_ctx* ctx, const float* scalars_dev, fu_stream stream);
/* Weight EMA fused into the Adam step.  The three buffers are CALLER-owned flat fp32 device memory --
 * [fu_total_param_elems], [fu_total_bn_channels], [fu_total_bn_channels], in the order of the parameter / running buffers --
 * initialised by the caller (usually to copies of the live values); like the moments they outlive the context.  All NULL
 * unbinds.  fu_adam_ema_step is fu_adam_step's update (the same float sequence, bit for bit) followed, in the same pass over
 * the parameters, by ema = lerp(ema, p_new, w) with w = (float)ema_weight, and in the same launch by
 * ema_running_mean = lerp(ema_running_mean, running_mean, w) and likewise the variance, the running buffers holding what
 * this step's training forward left in them.  lerp is torch's CPU Tensor.lerp_(end, w) on float32, one fused multiply-add in
 * either branch: w < 0.5: fma(w, end - self, self); w >= 0.5: fma(w - 1, end - self, end).  Without bound moments or without
 * bound EMA buffers the call returns FU_ERR_STATE.  FU_F16: a step the guard skips leaves the EMA buffers untouched too. */
int fu_bind_ema_state(fu_ctx* ctx, float* ema_params, float* ema_running_mean, float* ema_running_var);
int fu_adam_ema_step(fu_ctx* ctx, double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                     double ema_weight, fu_stream stream);
/* The captured form: out[0..6] are exactly fu_adam_scalars' seven values, out[7] = (float)ema_weight; the lerp branch is
 * chosen on the device from out[7], so one captured launch serves a warm-up whose weight crosses 0.5. */
int fu_adam_ema_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                        double ema_weight, float out[8]);
int fu_adam_ema_step_dev(fu_ctx* ctx, const float* scalars_dev, fu_stream stream);
/* Global-norm gradient clipping ahead of the optimiser step: torch.nn.utils.clip_grad_norm_(parameters, max_norm) in front
 * of optimizer.step() (Lightning's gradient_clip_val), without touching the gradient buffer.  max_norm > 0 arms it, 0
 * disarms it, a negative or non-finite value is an error.  The first arming call builds a chunk table of the parameter
 * table and a small state block in device memory (so arm before capturing a step).  While armed, every fu_adam_step[_dev] /
 * fu_adam_ema_step[_dev] first runs two launches on `stream`: one pass over the gradient buffer that writes the sum of
 * squares of every chunk (at most 16384 floats, never across two tensors) in double, and one workgroup that sums the chunks
 * of each tensor in chunk order, the tensors in parameter order (fixed orders: the same gradients give the same bits), and
 * forms, with gscale_in = the step's (float)grad_scale (slot 6 of the scalars):
 *     N      = sqrt(total) * fabs((double)gscale_in)            the norm of the gradients as Adam consumes them
 *     finite = isfinite(N)
 *     coef   = (finite && max_norm / (N + 1e-6) < 1.0) ? (float)(max_norm / (N + 1e-6)) : 1.0f
 *     scalars[6] = gscale_in * coef                             one fp32 multiply; the other scalars are copied
 * The Adam launch then reads these scalars from the context's own memory -- the caller's scalars_dev is only read -- so
 * the update is, bit for bit, the unclipped update with grad_scale = gscale_in * coef.  Skip rule: a step whose N is not
 * finite is left out entirely (parameters, moments and EMA buffers untouched), in every precision; the flag is rewritten by
 * every step.  FU_F16: the existing guard decides (fu_fp16_guard_state) -- a non-finite gradient sets both flags together.
 * With clipping disarmed the step issues exactly the launches it issues without this feature. */
int fu_set_grad_clip(fu_ctx* ctx, double max_norm);
/* What the last armed step left behind (synchronises the device, like fu_fp16_guard_state): (float)N, coef, and three
 * counters -- armed steps seen, steps clipped (coef < 1), steps with a non-finite norm.  All zero when clipping was never
 * armed on this context.  Any pointer may be NULL. */
int fu_grad_clip_state(fu_ctx* ctx, float* last_norm, float* last_coef, int64_t* steps, int64_t* clipped_steps,
                       int64_t* nonfinite_steps);
/* Decoupled weight decay (torch.optim.AdamW, single-tensor path) inside the same one launch.  weight_decay > 0 arms it, 0
 * disarms it, a negative or non-finite value is FU_ERR_INVALID.  decay_mask is a HOST array of n_mask == fu_num_params()
 * flags in parameter order (non-zero: the tensor decays), or NULL for the default rule: every tensor with ndim >= 2 (conv,
 * transposed-conv, 1x1 fusion and head weights) decays, biases and BatchNorm weight / bias do not.  A wrong n_mask, or a mask
 * whose flagged tensors form more than 512 separate ranges of the flat buffer, is FU_ERR_INVALID.  The call copies the
 * sorted bounds of those ranges into device memory it allocates once per context (and synchronises the device), so arm
 * before capturing a step; after a change of the setting a captured step must be captured again.
 * While armed with at least one flagged tensor, every fu_adam_step[_dev] / fu_adam_ema_step[_dev] launches the decay-aware
 * twin of its kernel (k_adamw, k_adamw_ema, k_adamw_dev, k_adamw_ema_dev): each element of a flagged tensor is first
 * multiplied by d = (float)(1.0 - lr * weight_decay) -- param.mul_(1 - lr * weight_decay): d formed in double and rounded
 * once, one fp32 multiply -- and the update of fu_adam_step then runs on that value, the same float sequence bit for bit.
 * The moments see the gradient only; the gradient norm and the clip coefficient are unaffected; the EMA takes the value
 * after decay and update; a skipped step (the FU_F16 guard, a non-finite clip norm) skips the decay too.
 * fu_adam_step / fu_adam_ema_step form d from their own lr.  The _dev forms read NINE floats from scalars_dev while decay is
 * armed -- fu_adamw_scalars' -- in the plain form too (slot 7, the EMA weight, is then ignored): a buffer of 7 or 8 floats
 * is TOO SHORT for an armed context.  With decay disarmed, or armed with no tensor flagged, the step issues exactly the
 * launches it issues without this feature and reads 7 (8) floats. */
int fu_set_weight_decay(fu_ctx* ctx, double weight_decay, const uint8_t* decay_mask, int n_mask);
/* The nine scalars of the captured form: out[0..6] are fu_adam_scalars' seven values bit for bit, out[7] = (float)ema_weight
 * (0 for the plain form), out[8] = (float)(1.0 - lr * weight_decay) -- exactly 1.0f for weight_decay = 0. */
int fu_adamw_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, double ema_weight,
                     double weight_decay, float out[9]);
/* What is armed: *weight_decay (0 when disarmed) and, in mask_out[0 .. n_mask - 1] with n_mask == fu_num_params(), the
 * per-tensor flags (all 0 when disarmed).  Either pointer may be NULL.  Host bookkeeping only. */
int fu_weight_decay_state(const fu_ctx* ctx, double* weight_decay, uint8_t* mask_out, int n_mask);
/* The gradient norms without a copy to the host: torch.linalg.vector_norm(p.grad) per parameter and of all of them.
 * norms_out_dev: fu_num_params() + 1 device floats -- every tensor's L2 norm times |grad_scale| in parameter order, then
 * the total -- from the same two launches (squares and sums in double, rounded to float once).  Works whether or not
 * clipping is armed (the first call may allocate: do not capture it); changes neither the clip state nor the optimiser. */
int fu_grad_norms(fu_ctx* ctx, double grad_scale, float* norms_out_dev, fu_stream stream);
int fu_zero_grads(fu_ctx* ctx, fu_stream stream);

/* ---- exact data-parallel mode (SyncBN statistics + global N_valid) ----------------
 * The reference trains on one device; with tiles sharded over ranks the default (DDP) semantics use per-rank
 * BatchNorm statistics and a per-rank 1/N_valid.  After fu_set_exact_sync every training fu_forward / fu_loss_ce /
 * fu_backward* sums its statistics partials over the ranks before they are finalised -- BN forward (sum y, sum y^2),
 * BN backward (sum g, sum g*xhat), CE (sum loss, N_valid) -- so that W ranks x B tiles reproduce one device with W*B
 * tiles up to fp32 summation order.  At each of those points the library copies the partials into `exchange`
 * (caller-owned device memory, >= fu_exact_sync_bytes), calls hook(user, n_elems, is_double) -- which must sum
 * exchange[0..n_elems) (double or float) over the ranks in place, ordered on the stream of the running call -- and
 * copies the result back.  Parameter gradients then hold each rank's SHARE of the global gradient: all-reduce them with
 * SUM and call fu_adam_step with grad_scale 1.  world <= 1 or hook == NULL switches the mode off. */
typedef int (*fu_sync_hook)(void* user, int64_t n_elems, int is_double);
int fu_set_exact_sync(fu_ctx* ctx, fu_sync_hook hook, void* user, int world, void* exchange, int64_t exchange_bytes);
int64_t fu_exact_sync_bytes(const fu_ctx* ctx);

/* ---- gradient all-reduce behind the C ABI (one process per GPU, RCCL over xGMI) ---------------
 * For hosts without torch.distributed.  RCCL (librccl.so) is resolved at run time on the first of these calls; nothing
 * else in the library depends on it.  One communicator per context.  The semantics are DESIGN.md section 6's: every rank
 * runs the step on its own tiles; per backward bucket (a contiguous range of the flat gradient buffer,
 * fu_block_param_range) fu_allreduce_begin starts a SUM all-reduce on the context's communication stream, ordered behind
 * the work enqueued on `stream` so far and, in side-stream mode 2, behind the weight-gradient chain enqueued so far (the
 * communication stream waits for both; `stream` is not joined: call fu_backward_join once, after the last block, before the
 * optimizer step), while the remaining backward blocks keep `stream` busy; fu_allreduce_wait makes
 * `stream` wait for every all-reduce begun so far; then fu_adam_step(..., grad_scale = 1 / world, ...).
 *   rank 0: fu_dp_unique_id(&id); ship the 128 bytes to the other ranks by any means (file, socket, MPI, environment);
 *   every rank: fu_dp_init(ctx, &id, rank, world); fu_dp_broadcast_state(ctx, stream) once (rank 0's parameters and
 *   BatchNorm buffers to everyone); ... steps ...; fu_dp_destroy (fu_destroy calls it). */
typedef struct fu_dp_id { char bytes[128]; } fu_dp_id;   /* ncclUniqueId */
int fu_dp_unique_id(fu_dp_id* id);
int fu_dp_init(fu_ctx* ctx, const fu_dp_id* id, int rank, int world);
int fu_dp_broadcast_state(fu_ctx* ctx, fu_stream stream);
int fu_allreduce_begin(fu_ctx* ctx, int64_t flat_offset, int64_t numel, fu_stream stream);
int fu_allreduce_wait(fu_ctx* ctx, fu_stream stream);
int fu_dp_destroy(fu_ctx* ctx);

/* ---- on-GPU tile augmentation (datasets/base_dataset.py:494-555) ------- */
/* Per sample b: hflip (flags[b] & 1), then vflip (& 2), then rotate by angles_deg[b] (& 4) with torchvision's
 * tensor semantics (nearest, expand=False, centre = image centre, image fill 0), applied identically to
 * image fp32 NCHW [B,C,H,W] and target int64 [B,H,W] (fill = target_fill; the reference fills 0).  Out of place.
 * The random draws (which transforms, which angle) stay on the host, as in sample_transforms(). */
enum { FU_AUG_HFLIP = 1, FU_AUG_VFLIP = 2, FU_AUG_ROTATE = 4 };
int fu_augment(const float* image, const int64_t* target, float* image_out, int64_t* target_out, const int32_t* flags,
               const float* angles_deg, int B, int C, int H, int W, int64_t target_fill, fu_stream stream);

/* Tile assembly of a batch that is already in HBM (datasets/base_dataset.py:77-113 `normalize`, :271-325
 * `_add_buffer_to_image`; ef_model.py:28-44 / stacked sensors: channel concatenation).  srcs: HOST array of n_src (<= 8)
 * device pointers, source k fp32 NCHW [B, src_channels[k], H, W]; the valid crop of sample b is the top-left
 * valid_h[b] x valid_w[b] corner (device int32 [B]; NULL = the whole tile).  out: fp32 NCHW [B, sum C, H, W] =
 * (x - mean) / std inside the crop, pad_value outside (the reference pads the image with 0 AFTER normalising).
 * norm_mode 0 = None (mean 0, std 1), 1 = 'local' (per sample and channel mean / population std over the crop, numpy
 * semantics; written to mean_out / std_out fp32 [B, sum C]), 2 = 'global' (global_mean / global_std fp32 [sum C]). */
int fu_assemble_tiles(const float* const* srcs, const int32_t* src_channels, int n_src, int B, int H, int W,
                      const int32_t* valid_h, const int32_t* valid_w, int norm_mode, const float* global_mean,
                      const float* global_std, float pad_value, float* out, float* mean_out, float* std_out,
                      fu_stream stream);

/* Streaming per-band statistics of tiles that are already in HBM (added within ABI 5: purely additive, no version bump).
 * What st_water_seg/misc/compute_dataset_normalization_parameters.py:12-91 gathers on the host (np.concatenate in a loop,
 * 10 % of the pixels) as one pass over every pixel on the device; also the percentiles of misc/compute_input_feature_stats.py.
 * The batch is described as for fu_assemble_tiles: srcs = HOST array of n_src (1..8) device pointers, source k fp32 NCHW
 * [B, src_channels[k], H, W], at most 16 channels in all; the valid crop of sample b is the top-left valid_h[b] x valid_w[b]
 * corner (device int32 [B], clamped to the tile; NULL = the whole tile).
 * mask_mode 0: every pixel of the valid crop counts.  mask_mode 1, the reference's rule (:19-24): a pixel counts when the
 * fp32 sum, in channel order, of the FIRST source's channels at that pixel is not 0; that one mask applies to every source
 * (the reference uses the image's mask for dem / slope too).  In both modes a pixel where any channel of any source is NaN
 * or Inf is left out of every channel and counted in n_nonfinite (the reference would return NaN statistics there).
 * Every field of fu_band_accum is a CALLER-owned device buffer that the call ADDS to, so a data set is streamed through
 * batch by batch: count / n_nonfinite int64 [C] (every channel gets the same numbers: the mask is per pixel), sum / sumsq
 * fp64 [C], vmin / vmax fp32 [C] (the caller initialises them to +inf / -inf, the sums and counts to 0), hist int64
 * [C][n_bins] or NULL (no histogram): n_bins (1..65536) equal bins over [lo, hi], bin = floor((x - lo) * (n_bins / (hi - lo)))
 * in fp32 with n_bins / (hi - lo) rounded once, values outside go to the edge bins.
 * Every input element is read once.  The result is bit-reproducible: no floating-point atomics -- per-workgroup fp64
 * partials go to `workspace` (device memory, 16-byte aligned, >= fu_band_stats_workspace_bytes(C, n_bins or 0); contents
 * are scratch) and are folded in a fixed order; the histogram is counted with integer atomics in LDS.  Calls that share
 * accumulators or a workspace must be ordered on one stream.  A rejected call (FU_ERR_INVALID) launches nothing. */
typedef struct fu_band_accum {
  int64_t* count;        /* [C] pixels taken */
  double* sum;           /* [C] */
  double* sumsq;         /* [C] */
  float* vmin;           /* [C], +inf before the first call */
  float* vmax;           /* [C], -inf before the first call */
  int64_t* n_nonfinite;  /* [C] pixels left out because a channel was NaN / Inf */
  int64_t* hist;         /* [C][n_bins], or NULL */
  int32_t n_bins;
  float lo, hi;
} fu_band_accum;
int64_t fu_band_stats_workspace_bytes(int n_channels, int n_bins);
int fu_band_stats(const float* const* srcs, const int32_t* src_channels, int n_src, int B, int H, int W,
                  const int32_t* valid_h, const int32_t* valid_w, int mask_mode, const fu_band_accum* acc,
                  void* workspace, int64_t workspace_bytes, fu_stream stream);

/* Lanczos-4 resampling of a batch of tiles on the device (ABI 5).  Replaces the per-item WHOLE-RASTER resample of the reference's
 * loader (st_water_seg/datasets/floodplanet.py:338-340 -> utils/utils_image.py:11-54, cv2.INTER_LANCZOS4) by a per-tile one:
 * Lanczos is local, so the tile [Y0, Y0 + tile_h) x [X0, X0 + tile_w) of the resampled raster depends only on a window of the
 * source raster.  windows: fp32 [B][C][win_h][win_w] (the host's cut-outs, padded to a common size); iy / wy: int32 / fp32
 * [B][tile_h][8], ix / wx: [B][tile_w][8] -- per output row / column the 8 window-relative source indices (borders replicated)
 * and the normalised Lanczos weights (all-zero rows / columns beyond the raster's edge).  out: fp32 [B][C][tile_h][tile_w] =
 * the crop of the resampled raster, then the sensor scaling that follows the crop in the reference: scale_mode 0 none, 1 S1
 * clip((x + 50) / 100, 0, 1) with NaN -> 0 (:347), 2 S2 clip(x / 2^12, 0, 1) (:406), 3 L8 clip(x, 0, 18607.72) / 18607.72 (:525),
 * 4 PS stored as uint16 x / 2^16 (:467-468).  fp32, taps accumulated in order with separate multiply / add roundings: equal bit
 * for bit to the host restatement floodplanet_code_amd/datasets/resize.py (OpenCV itself is absent: parity unpinned vs cv2). */
int fu_resize_lanczos4_tiles(const float* windows, int B, int C, int win_h, int win_w, const int32_t* iy, const float* wy,
                             const int32_t* ix, const float* wx, int tile_h, int tile_w, int scale_mode, float* out,
                             fu_stream stream);

/* Crops of scenes that are resident on the device (label-free inference; infer.py of the reference cuts them on the host).
 * Entry b names a scene (fp32 [C, scene_h, scene_w] on the device) and a box [h0, hE) x [w0, wE) inside it, with
 * 1 <= hE - h0 <= tile_h and 1 <= wE - w0 <= tile_w.  out: fp32 [n, C, tile_h, tile_w], equal bit for bit to cutting each
 * box into the top-left corner of a zero [n, C, tile_h, tile_w] batch and calling fu_assemble_tiles on it with
 * valid_h = hE - h0, valid_w = wE - w0 and the same norm_mode / global parameters / pad_value (mean_out / std_out: fp32
 * [n, C], needed for 'local').  One launch, two with 'local'.  `entries` is a host array; it is copied into a
 * library-owned device buffer ordered on `stream`, so calls on different streams must be ordered by the caller.  Every
 * entry and argument is checked before anything is launched: a rejected call launches nothing. */
typedef struct fu_scene_crop {
  const float* scene;        /* fp32 [C, scene_h, scene_w] on the device */
  int32_t scene_h, scene_w;
  int32_t h0, w0, hE, wE;    /* the box, inside the scene, at most the tile */
} fu_scene_crop;
int fu_scene_crops(fu_ctx* ctx, int n, const fu_scene_crop* entries, int C, int tile_h, int tile_w, int norm_mode,
                   const float* global_mean, const float* global_std, float pad_value, float* out, float* mean_out,
                   float* std_out, fu_stream stream);

/* Finished training batches from scenes that are resident on the device (added within ABI 5: purely additive, no version
 * bump).  Entry b names a scene and a box as for fu_scene_crops, the scene's label raster (uint8 [scene_h, scene_w] on the
 * device, the RAW values of the label file; NULL when no target is wanted) and the sample's transforms (FU_AUG_* flags and
 * the rotation angle in degrees, as fu_augment takes them).  image_out fp32 [n, C, tile_h, tile_w] and target_out int64
 * [n, tile_h, tile_w] (optional) equal, bit for bit, fu_scene_crops (same norm_mode, parameters, pad_value) followed by
 * fu_augment (same flags / angles, image fill 0, target_fill), where the un-augmented target of entry b is its label box
 * decoded as the data set decodes it (raw 2 -> 1, raw 0 -> nodata_value, anything else -> 0) in the top-left corner of a
 * tile filled with target_fill.  mean_out / std_out: fp32 [n, C], written (and needed) for 'local' only, the statistics of
 * the un-augmented crop.  One launch, two with 'local'; no intermediate batch is written.  16-byte stores need
 * tile_w % 4 == 0 and 16-byte aligned outputs; otherwise the kernel stores element by element.  The table is copied into a
 * library-owned device buffer ordered on `stream`, as for fu_scene_crops, and every entry and argument is checked before
 * anything is launched (tile_h * tile_w <= 2^25): a rejected call launches nothing. */
typedef struct fu_scene_train_entry {
  const float* scene;        /* fp32 [C, scene_h, scene_w] on the device (the resampled, sensor-scaled grid) */
  const uint8_t* label;      /* uint8 [scene_h, scene_w] on the device, or NULL */
  int32_t scene_h, scene_w;
  int32_t h0, w0, hE, wE;    /* the box, inside the scene, at most the tile */
  int32_t flags;             /* FU_AUG_HFLIP | FU_AUG_VFLIP | FU_AUG_ROTATE */
  float angle_deg;
} fu_scene_train_entry;
int fu_scene_train_tiles(fu_ctx* ctx, int n, const fu_scene_train_entry* entries, int C, int tile_h, int tile_w,
                         int norm_mode, const float* global_mean, const float* global_std, float pad_value,
                         int64_t nodata_value, int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out,
                         float* std_out, fu_stream stream);

/* fu_scene_train_tiles with radiometric and zoom augmentation in the same pass (added within ABI 5: purely additive).
 * aug == NULL, or a struct whose gain, bias, sigma, out_h and out_w are all NULL, IS fu_scene_train_tiles: the same
 * launch, the same bits.  Every array of the struct is a HOST array; they travel in the same library-owned device table
 * as the boxes, one upload ordered on `stream`.
 *
 * Radiometric part (gain / bias / sigma: fp32 [n * C], sample-major, each optional -- a NULL term is skipped).  Every image
 * pixel that comes from the scene becomes, after normalisation and with each operation rounded on its own,
 *     t = v * gain[b][c];  t = t + bias[b][c];  t = t + sigma[b][c] * z
 * in units of the normalised batch.  Pad pixels keep pad_value, rotation corners 0, targets are untouched.  z is a
 * unit-variance pseudo-normal without a transcendental: Philox4x32-10 with key = (low, high word of noise_key) and counter
 * = (oy * tile_w + ox of the OUTPUT pixel, channel, low word of noise_stream[b], high word of noise_stream[b]); S = the sum
 * of the eight 16-bit halves of the four output words; z = (float)(2 * S - 524280) * k, k = (float)(1 / sqrt(32 * (65536^2
 * - 1) / 12)).  So the noise of a sample depends on its stream and the pixel alone, not on its place in the batch, the
 * launch grid or the store width.  sigma needs noise_stream (uint64 [n]).  gain and bias must be finite, sigma finite and
 * >= 0.  floodplanet_code_amd/augment.py (photometric_host) restates all of it in numpy, bit for bit.
 *
 * Zoom part (out_h, out_w: int32 [n], both or neither; 1 <= out_h[b] <= tile_h, 1 <= out_w[b] <= tile_w).  With them the
 * box of entry b may be any non-empty box inside its scene, LARGER THAN THE TILE INCLUDED, and is resampled onto the
 * top-left out_h x out_w region of the tile; the rest is padded as before.  Flips and the rotation yield an integer pixel
 * of the un-augmented tile as they always did; zoom maps that pixel into the box, per axis and in fp32 with every
 * operation rounded on its own (src = the box's size, out = the out size, i = the pixel):
 *     scale = (float)src / (float)out;  f = max(((float)i + 0.5f) * scale - 0.5f, 0);
 *     i0 = min((int)floorf(f), src - 1);  i1 = min(i0 + 1, src - 1);  w = f - (float)i0
 * The image is interpolated along x, then along y, with lerp(p, q, w) = p + w * (q - p), and normalised after that (then
 * the radiometric part).  Labels take the raw byte at min((int)floorf(((float)i + 0.5f) * scale), src - 1) per axis
 * (torch's 'nearest-exact') and are decoded as usual.  src == out gives w = 0 and the source pixel itself.  Under norm_mode
 * 'local' the statistics are those of the SOURCE BOX's own pixels (the stats kernel of fu_scene_crops, which has no
 * tile-size limit), not of the resampled tile; at zoom 1 that is fu_scene_train_tiles' behaviour.
 * floodplanet_code_amd/datasets/sampling.py (zoom_tile_host) is the numpy statement.
 *
 * Every entry and every array element is checked before anything is copied or launched: a rejected call launches
 * nothing.  Without the zoom part a box is still at most the tile. */
typedef struct fu_scene_aug {
  const float* gain;             /* host fp32 [n * C] or NULL */
  const float* bias;             /* host fp32 [n * C] or NULL */
  const float* sigma;            /* host fp32 [n * C] or NULL */
  const uint64_t* noise_stream;  /* host uint64 [n]; needed with sigma */
  uint64_t noise_key;
  const int32_t* out_h;          /* host int32 [n] or NULL (with out_w) */
  const int32_t* out_w;
} fu_scene_aug;
int fu_scene_train_tiles_ex(fu_ctx* ctx, int n, const fu_scene_train_entry* entries, int C, int tile_h, int tile_w,
                            int norm_mode, const float* global_mean, const float* global_std, float pad_value,
                            int64_t nodata_value, int64_t target_fill, float* image_out, int64_t* target_out,
                            float* mean_out, float* std_out, const fu_scene_aug* aug, fu_stream stream);

/* Class frequencies of resident label rasters (added within ABI 5: purely additive), for "balanced" class weights.
 * entries: a host table of n fu_scene_train_entry; only label, scene_h, scene_w and the box are read (scene, flags and
 * angle_deg are ignored), a NULL label is rejected, and a box may be as large as its raster.  Every pixel of every box is
 * decoded as fu_scene_train_tiles decodes it (raw 2 -> 1, raw 0 -> nodata_value, anything else -> 0) and counts_out[d]
 * (device int64 [n_classes], caller-owned) is ADDED to for 0 <= d < n_classes; other values are dropped.  Integer
 * arithmetic only (LDS histogram per workgroup, then 64-bit integer atomics): exact and order-independent.  One launch.
 * The table goes through a library-owned device buffer ordered on `stream` (shared with fu_scene_train_tiles), and every
 * entry is checked before anything is launched: a rejected call launches nothing and leaves counts_out untouched. */
int fu_label_class_counts(fu_ctx* ctx, int n, const fu_scene_train_entry* entries, int64_t nodata_value, int n_classes,
                          int64_t* counts_out, fu_stream stream);

/* The label content of every box of a table, separately (added within ABI 5: purely additive), for content-aware tile
 * sampling.  entries: as for fu_label_class_counts -- only label, scene_h, scene_w and the box are read, a NULL label is
 * rejected, and a box may be as large as its raster.  Row i of counts_out (device int64 [n][3], caller-owned) is WRITTEN,
 * not added to: the pixels of box i by raw label category -- column 0 = raw neither 0 nor 2 (decodes to class 0), column 1
 * = raw 2 (decodes to class 1), column 2 = raw 0 (no data).  The three sum to the box's area; mapping them to decoded
 * classes (no data -> nodata_value) is the caller's job.  Integer arithmetic only, exact; one workgroup per box owns its
 * row, so there are no global atomics and nothing to zero beforehand.  One launch.  The table goes through the same
 * library-owned device buffer ordered on `stream`, and every entry is checked (the checks and messages of
 * fu_label_class_counts) before anything is copied or launched: a rejected call launches nothing and leaves counts_out
 * untouched. */
int fu_label_box_counts(fu_ctx* ctx, int n, const fu_scene_train_entry* entries, int64_t* counts_out, fu_stream stream);

/* ---- inference stitching (ImageStitcher_v2, utils/utils_image.py:410-494) ------------- */
/* canvas[h0:hE, w0:wE, :] += softmax(logits of sample `sample` of the last fu_forward)[:hE-h0, :wE-w0, :];
 * weight[h0:hE, w0:wE] += 1.  canvas: fp32 [canvas_h, canvas_w, n_classes], weight: fp32 [canvas_h, canvas_w]. */
int fu_stitch_add(fu_ctx* ctx, int sample, float* canvas, float* weight, int canvas_h, int canvas_w, int h0, int w0,
                  int hE, int wE, fu_stream stream);
/* canvas /= (weight + 1e-5) in place (ImageStitcher_v2._combine_images); argmax_out: optional int64 [canvas_h, canvas_w] */
int fu_stitch_finalize(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w,
                       int64_t* argmax_out, fu_stream stream);
/* One crop of a batched stitch: sample `sample` of the last fu_forward goes to canvas[h0:hE, w0:wE] as in fu_stitch_add.
 * Entries that name the same canvas must name the same weight and canvas size; distinct canvases, distinct weights. */
typedef struct fu_stitch_entry {
  float* canvas;        /* fp32 [canvas_h, canvas_w, n_classes] */
  float* weight;        /* fp32 [canvas_h, canvas_w] */
  int32_t sample;
  int32_t canvas_h, canvas_w;
  int32_t h0, w0, hE, wE;
  int32_t reserved;     /* 0 */
} fu_stitch_entry;
/* fu_stitch_add for entries[0..n-1] in one launch, bit-identical to the n calls in table order (canvas and weight), also
 * when boxes of the table overlap on one canvas: each canvas pixel is written by one thread, which adds the covering
 * entries' softmax in table order (no float atomics).  `entries` is a host array; every box must be non-empty and lie
 * inside its canvas and the tile.  The table is copied into a library-owned device buffer ordered on `stream`, so calls
 * on different streams must be ordered by the caller. */
int fu_stitch_add_batch(fu_ctx* ctx, int n, const fu_stitch_entry* entries, fu_stream stream);

/* ---- test-time augmentation ------------------------------------------------------------------- */
/* A view code is a bit set; the view of an image t is, in this order and in torch terms:
 *   if (code & 4) t = t.transpose(-1, -2);  if (code & 1) t = t.flip(-1);  if (code & 2) t = t.flip(-2);
 * and its inverse runs the three steps in reverse order.  Codes 0..7 are the eight symmetries of the square (3 = rot180,
 * 5 and 6 = the two 90-degree rotations, 7 = anti-transpose); the transposing codes need a square tile.  The reference
 * has no test-time augmentation: this section is an extension, and nothing in it restates reference code. */
enum { FU_VIEW_HFLIP = 1, FU_VIEW_VFLIP = 2, FU_VIEW_TRANSPOSE = 4 };
/* Eval forward of n_views * batch samples: sample v * batch + b is view codes[v] of crop b of the sources (as
 * fu_forward_srcs).  The views are taken inside the NCHW -> NHWC input gather of every encoder: no transformed copy of
 * the batch is written.  codes: HOST array of n_views (1..8) distinct codes in 0..7; n_views * batch <= max_batch.
 * logits_out: optional fp32 NCHW [n_views * batch, k, H, W].  The context remembers the codes for fu_merge_views; any
 * later forward forgets them.  A rejected call launches nothing. */
int fu_forward_views(fu_ctx* ctx, const float* const* srcs, const int32_t* src_channels, int n_src, int batch,
                     int n_views, const int32_t* codes, float* logits_out, fu_stream stream);
/* After fu_forward_views, one launch: P_b = (sum over v in view order of inverse view codes[v] of softmax(logits of
 * sample v * batch + b)) / n_views, the softmax with fu_stitch_add's expression.  probs_out: optional fp32
 * [batch, H, W, k] = P.  counts_out: optional int64 [batch][k][k], ADDED to, counts_out[b][t * k + p] = #pixels of crop b
 * with target t and p = argmax P (first maximum wins), over pixels whose target is neither ignore_index nor out of [0, k)
 * (as fu_eval_confusion); target int64 [batch, H, W] comes with it.  At least one of probs_out / counts_out. */
int fu_merge_views(fu_ctx* ctx, float* probs_out, const int64_t* target, int ignore_index, int64_t* counts_out,
                   fu_stream stream);
/* fu_stitch_add_batch with entries[i].sample indexing probs (fp32 [batch, H, W, k], e.g. fu_merge_views' probs_out)
 * instead of the resident logits: the probabilities are added as they are (no softmax), with the same ownership scheme,
 * table order and entry checks -- bit-identical to canvas[box] += probs[sample, :dh, :dw]; weight[box] += 1 in table
 * order.  Needs no forward pass. */
int fu_stitch_add_batch_probs(fu_ctx* ctx, int n, const fu_stitch_entry* entries, const float* probs, int batch,
                              fu_stream stream);

/* fu_stitch_add_batch (probs == NULL: the resident logits of the last forward) or fu_stitch_add_batch_probs (probs given,
 * `batch` samples) with a separable window: win_y / win_x are caller-owned fp32 DEVICE arrays of H and W elements (the
 * context's tile size), indexed by the tile-local coordinate ly = cy - h0, lx = cx - w0 of the canvas pixel (cy, cx),
 * also in an edge-clipped box.  Same ownership scheme, table order and entry checks; per covering entry, each operation
 * rounding on its own in fp32 (nothing contracts into an fma):
 *   w = win_y[ly] * win_x[lx];  p[k] = probs[sample][ly][lx][k]  or  e[k] * inv (the softmax terms of fu_stitch_add, the
 *   product rounded first);  canvas[k] = canvas[k] + w * p[k] (product rounded, then the add);  weight = weight + w
 * -- bit-identical to canvas[box] += probs[s, :dh, :dw] * (win_y[:dh, None] * win_x[None, :dw])[..., None];
 * weight[box] += win_y[:dh, None] * win_x[None, :dw] in table order, and the logits source adds what the probs source
 * adds of fu_merge_views' single-view probabilities.  The library knows nothing about window shapes.  A rejected call
 * (the checks of fu_stitch_add_batch, or a null window) launches nothing. */
int fu_stitch_add_batch_windowed(fu_ctx* ctx, int n, const fu_stitch_entry* entries, const float* probs, int batch,
                                 const float* win_y, const float* win_x, fu_stream stream);
/* Fused finalisation of a canvas, one launch.  Per pixel, each operation rounding on its own: s = weight + eps; if
 * s > 0: inv = 1.f / s, v[k] = canvas[k] * inv (fu_stitch_finalize's expression: with eps = 1e-5f the normalised canvas
 * and the argmax are bit-identical to it); otherwise the pixel is uncovered: v[k] = 0, class index 0, every map 0, and
 * the pixel is not counted.  The argmax takes the first maximum.  Outputs, each optional (NULL = skip), at least one:
 *   normalize_in_place != 0: canvas[k] = v[k] (0: the raw sums stay);
 *   class_out  uint8 [canvas_h, canvas_w] = class_values[argmax]; class_values: HOST array of n_classes bytes, NULL =
 *              identity (an uncovered pixel gets class_values[0]);
 *   prob_out   uint8 [n_classes, canvas_h, canvas_w] (bands first) = (uint8) rintf(fminf(fmaxf(v[k], 0), 1) * 255);
 *   margin_out uint8 [canvas_h, canvas_w] = the same quantisation of v[top1] - v[top2] (v[0] for n_classes == 1; 0 at
 *              a tie);
 *   counts_out int64 [n_classes], ADDED to: covered pixels per argmax class (integer atomics: exact, order-free).
 * eps must be finite and >= 0, n_classes in 1..8.  A rejected call launches nothing. */
int fu_stitch_finalize_maps(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                            int normalize_in_place, const uint8_t* class_values, uint8_t* class_out, uint8_t* prob_out,
                            uint8_t* margin_out, int64_t* counts_out, fu_stream stream);

/* fu_stitch_finalize_maps with a one-class-versus-rest decision rule.  thr == NULL: fu_stitch_finalize_maps bit for bit
 * (which forwards here).  Otherwise the decided class index of a covered pixel is thr->cls when v[thr->cls] >=
 * thr->threshold (v the normalised values above, compared in fp32), and when it is not, the first maximum over the classes
 * other than thr->cls.  class_out (= class_values[decided]) and counts_out follow the decided class; the normalised canvas,
 * prob_out, margin_out (still top-1 minus top-2 of v) and the uncovered-pixel rule are unchanged.  Rejected, launching
 * nothing: n_classes < 2, cls outside [0, n_classes), a threshold that is not finite or lies outside [0, 1]. */
typedef struct fu_class_threshold { int32_t cls; float threshold; } fu_class_threshold;
int fu_stitch_finalize_maps_ex(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                               int normalize_in_place, const uint8_t* class_values, uint8_t* class_out, uint8_t* prob_out,
                               uint8_t* margin_out, int64_t* counts_out, const fu_class_threshold* thr, fu_stream stream);

#define FU_MAP_MAX_PIXELS (1 << 28)

/* ---- nodata in scene inference (added within ABI 5: purely additive) ---------------------------- */
/* fu_stitch_finalize_maps_ex with a valid-pixel mask.  valid == NULL: fu_stitch_finalize_maps_ex bit for bit (which
 * forwards here; nodata_value is then not looked at).  Otherwise valid is a device uint8 [canvas_h, canvas_w], and a pixel
 * with valid[p] == 0 is treated as the uncovered pixel is -- v[k] = 0, prob_out and margin_out 0, not counted in
 * counts_out, normalised canvas 0 -- except that class_out = nodata_value.  One launch; the mask is one more byte per
 * pixel.  Rejected, launching nothing and leaving every output untouched: what fu_stitch_finalize_maps_ex rejects, and with
 * a mask a canvas that is empty or has more than FU_MAP_MAX_PIXELS pixels, a nodata_value outside 0..255, a nodata_value
 * below n_classes when class_values == NULL, a nodata_value equal to one of class_values. */
int fu_stitch_finalize_maps_masked(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                                   int normalize_in_place, const uint8_t* class_values, uint8_t* class_out,
                                   uint8_t* prob_out, uint8_t* margin_out, int64_t* counts_out,
                                   const fu_class_threshold* thr, const uint8_t* valid, int nodata_value, fu_stream stream);

/* The valid-pixel mask of a resident scene on its output grid (floodplanet_code_amd/datasets/valid_mask.py holds the numpy
 * statements, source_valid_host then grid_valid_host; integer-exact).  raster: fp32 [C, src_h, src_w] as uploaded, before
 * sensor scaling.  A source pixel is valid when every band is finite and, with use_nodata != 0, not every band == nodata
 * (fp32 ==).  iy / wy [grid_h][8], ix / wx [grid_w][8]: the tables of fu_resize_lanczos4_tiles for the whole grid (B = 1);
 * grid pixel (Y, X) is valid when every source pixel (iy[Y][a], ix[X][b]) with wy[Y][a] != 0 and wx[X][b] != 0 is valid;
 * a tap index is clamped into the source before it is used.  src_valid: caller-owned scratch uint8 [src_h, src_w] (holds
 * the source mask afterwards); valid_out: uint8 [grid_h, grid_w], 0 / 1; n_valid_out: int64 [1], WRITTEN (zeroed on
 * `stream`, then one integer atomic per workgroup): the number of valid grid pixels.  Two launches, no host read.  Every
 * argument is checked before anything is launched -- null pointers, C outside 1..16, a size < 1 or above
 * FU_MAP_MAX_PIXELS pixels, a non-finite nodata with use_nodata -- and a rejected call leaves the outputs untouched. */
int fu_scene_valid_mask(const float* raster, int C, int src_h, int src_w, int use_nodata, float nodata, const int32_t* iy,
                        const float* wy, const int32_t* ix, const float* wx, int grid_h, int grid_w, uint8_t* src_valid,
                        uint8_t* valid_out, int64_t* n_valid_out, fu_stream stream);

/* The census of a table of boxes of byte masks, the twin of fu_label_box_counts: counts_out[i] (device int64 [n],
 * caller-owned) is WRITTEN, not added to: the non-zero bytes of mask[h0:hE, w0:wE].  A box may be as large as its mask.
 * One workgroup per box owns its cell: no global atomics, nothing to zero beforehand.  One launch.  `entries` is a host
 * array; the table goes through the library-owned device buffer of fu_scene_crops, ordered on `stream`.  Every entry is
 * checked before anything is copied or launched (n < 1, a null mask, a mask that is empty or above FU_MAP_MAX_PIXELS, a
 * box that is empty or lies outside its mask): a rejected call launches nothing and leaves counts_out untouched. */
typedef struct fu_mask_box { const uint8_t* mask; int32_t mask_h, mask_w; int32_t h0, w0, hE, wE; } fu_mask_box;
int fu_mask_box_counts(fu_ctx* ctx, int n, const fu_mask_box* entries, int64_t* counts_out /* [n], WRITTEN */,
                       fu_stream stream);

/* ---- tiled / compressed / BigTIFF scenes (added within ABI 5: purely additive); no context needed ---- */
/* The host's entropy decoders (csrc/fu_tiff_codec.cpp: plain C++, no HIP call -- using them never opens the GPU).  Both
 * read src[0, n_src) only and write dst[0, n_dst) only, on any input: they stop at n_dst or at the end of the stream and
 * return the bytes written (fewer than n_dst when the stream ends first), or a negative code: -1 a null buffer or negative
 * size, -2 a corrupt stream (a code that cannot occur; a PackBits run cut off), -3 the LSB-first LZW of old writers.
 * LZW is TIFF 6.0's: MSB-first codes of 9 to 12 bits, Clear 256, EndOfInformation 257, the width growing one code early,
 * the code-equals-next-free-entry case.  floodplanet_code_amd/datasets/geotiff.py holds the Python statements
 * (lzw_decode_host, packbits_decode_host). */
int64_t fu_tiff_lzw_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst);
int64_t fu_tiff_packbits_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst);

#define FU_TIFF_MAX_BANDS 16
#define FU_TIFF_UNPACK_CHUNK 256 /* pixels of a segment row a wave takes per pass; longer rows carry the scan along */
enum fu_tiff_sample_kind { FU_TIFF_UINT = 1, FU_TIFF_INT = 2, FU_TIFF_FLOAT = 3 }; /* TIFF SampleFormat */
/* How the decoded segments of a TIFF's first image lie in one buffer.  Segments follow each other in the order of the
 * file's offset array (PlanarConfiguration 2: plane after plane), each at its nominal size: a tile is always seg_h x seg_w
 * (an edge tile is full size; what lies outside the image is dropped), strip s holds min(seg_h, height - s * seg_h) rows of
 * the image's width.  So every offset is arithmetic and no table is needed. */
typedef struct fu_tiff_layout {
  int32_t width, height;
  int32_t samples;          /* samples per pixel, 1..64 */
  int32_t bytes_per_sample; /* 1, 2, 4 or 8 */
  int32_t sample_kind;      /* enum fu_tiff_sample_kind */
  int32_t big_endian;       /* the file's byte order is MM */
  int32_t planar;           /* PlanarConfiguration 2: one plane of segments per sample */
  int32_t tiled;            /* segments are tiles (0: strips, seg_w == width, seg_h = RowsPerStrip) */
  int32_t seg_w, seg_h;
  int32_t predictor;        /* 1 none, 2 horizontal differencing (integers), 3 floating point (IEEE samples) */
  int32_t reserved;         /* 0 */
} fu_tiff_layout;
/* Decoded segments -> out fp32 [n_bands, height, width], out[n] = sample bands[n] (host array, n_bands in
 * 1..FU_TIFF_MAX_BANDS, output order; an index may repeat): undo the predictor, swap bytes, take tiles apart, pick bands,
 * convert -- bit for bit np.float32 of datasets/geotiff.py's read_raster: 8- and 16-bit integers exactly, 32- and 64-bit
 * integers and float64 rounded to nearest even (subnormal results kept), float32 copied bit for bit.  Predictor 2 sums
 * modulo 2^bits after the byte swap, per sample component, per segment row; predictor 3 sums bytes modulo 2^8 with stride
 * samples-per-pixel-in-the-segment along the row, whose byte b (most significant first) of value i is then byte
 * b * (seg_w * samples in the segment) + i, in both byte orders.  src: device, 8-byte aligned, n_bytes long.  ONE launch
 * (a wave per segment row, wave-level scan with a carry along the row; under predictor 3 the row is read twice, the plane
 * totals first), no atomics, no host read.  Every argument is checked first -- null pointers, sizes (an image or segment
 * above FU_MAP_MAX_PIXELS pixels), n_bytes != the layout's arithmetic total, a band index >= samples, predictor 3 on
 * integers, predictor 2 on floats -- and a rejected call launches nothing and leaves out untouched. */
int fu_tiff_unpack(const uint8_t* src, int64_t n_bytes, fu_tiff_layout layout, const int32_t* bands, int n_bands, float* out,
                   fu_stream stream);
/* The inverse, for writing: a device-resident raster -> dst, the bytes a TIFF writer hands its entropy coder, bit for bit
 * datasets/geotiff_write.py's pack_host, every byte of dst included; fu_tiff_unpack of dst with the same layout gives the
 * raster back.  src: the base pointer of sample (band 0, row 0, column 0); sample (b, y, x) lies at element b * band_stride +
 * y * row_stride + x * col_stride (strides in elements, >= 0; element size and kind from the layout), so an [H, W, k] canvas
 * (strides 1, W * k, k) and a [k, H, W] tensor are both sources without a copy.  Segments lie back to back at their nominal
 * size in the order of the offset array: a tile is always seg_h x seg_w and a position outside the image holds the nearest
 * image pixel (the index clamped per axis), padded before the predictor so that padding differences to zeros; the last
 * strip holds the rows that are left.  Predictor 2: per segment row v[x] - v[x - 1] modulo 2^bits, the first value as it is.
 * Predictor 3: the row's values as bytes_per_sample byte planes of seg_w bytes, most significant first, then the whole row
 * differenced byte-wise, across the plane boundaries, the first byte as it is.  Supported: little-endian (big_endian 0),
 * bytes_per_sample 1, 2 or 4, float samples of 4 bytes, samples 1..FU_TIFF_MAX_BANDS and planar != 0 whenever samples > 1
 * (chunky output is rejected), strips (seg_w == width) or tiles whose sides are multiples of 16.  dst: device, 16-byte
 * aligned, n_bytes long.  ONE launch, a streaming gather: a lane produces whole 16-byte groups of dst (where rows are
 * multiples of 16 values it loads 16 values once and stores a group in each byte plane), no atomics, no host read, 64-bit
 * byte offsets.  Every argument is checked first -- null pointers, alignment, negative strides, sizes (an image or segment
 * above FU_MAP_MAX_PIXELS pixels), n_bytes != the layout's arithmetic total, an unsupported layout, predictor 3 on integers,
 * predictor 2 on floats -- and a rejected call launches nothing and leaves dst untouched. */
int fu_tiff_pack(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, fu_tiff_layout layout,
                 uint8_t* dst, int64_t n_bytes, fu_stream stream);

/* ---- overview pyramids of the rasters infer writes (fu_overview.hip; added within ABI 5: purely additive) ---------- */
/* The reduced-resolution levels of a device-resident raster, bit for bit datasets/overviews.py's overviews_host.  src,
 * the strides (in elements, >= 0), bands (1..FU_TIFF_MAX_BANDS), h and w (h * w <= FU_MAP_MAX_PIXELS) describe the raster
 * as for fu_tiff_pack, so an [H, W, k] canvas and a [k, H, W] tensor are both sources without a copy.  Level l >= 1 is
 * ceil(h / 2^l) x ceil(w / 2^l); its pixel (y, x) is reduced from the pixels (2y..2y+1, 2x..2x+1) of level l - 1 that exist
 * -- one, two or four -- so the levels are a cascade, never taken from the base.  kind:
 *   FU_OVERVIEW_MODE_U8   uint8: the most frequent value among the block's pixels that differ from nodata_value (-1..255;
 *                         -1: none is excluded), ties to the smaller value; nodata_value where every pixel is nodata.
 *   FU_OVERVIEW_MEAN_U8   uint8: over the block's valid pixels (2 * sum + n) / (2 * n) in integers, which rounds half up; 0
 *                         where none is valid.
 *   FU_OVERVIEW_MEAN_F32  fp32: the valid pixels summed in row-major order from +0, one rounding per add, then ONE correctly
 *                         rounded division by float(n); 0 where none is valid.
 *   FU_OVERVIEW_ANY_U8    uint8: 1 where a pixel of the block is non-zero, else 0.
 * valid: device uint8 [h, w] or NULL (every pixel valid), the mean kinds only; a pixel is valid where its byte is non-zero,
 * and the mask of level l is `any` of the mask of level l - 1.  nodata_value is -1 for every kind but mode_u8.
 * dst: the levels back to back, each a contiguous [bands, h_l, w_l] of the source's sample type; dst_elems >= bands * the sum
 * of h_l * w_l.  valid_dst: the mask levels back to back, uint8 [h_l, w_l] each (the sum of h_l * w_l bytes, caller-owned);
 * required exactly when valid is given.  n_levels: 0 .. the number of levels down to 1 x 1, ceil(log2(max(h, w))).
 * One pass per launch: a workgroup loads a 64 x 64 base tile (and the mask's) into LDS once, 16-byte loads where col_stride
 * == 1, reduces it there level by level and writes every level's block, so one launch gives six levels and reads the base
 * once; deeper levels come from one further launch per six whose source is the last level written.  wave64, no atomics, no
 * workgroup waits for another, 64-bit offsets, no host read.  Every argument is checked first -- null src / dst, an unknown
 * kind, bands, sizes, negative strides, n_levels, valid without valid_dst or the reverse, valid with a kind that takes none,
 * nodata_value, alignment to the sample size, a short dst_elems -- and a rejected call launches nothing and leaves dst
 * untouched.  n_levels = 0 is FU_OK with no launch. */
enum fu_overview_kind { FU_OVERVIEW_MODE_U8 = 0, FU_OVERVIEW_MEAN_U8 = 1, FU_OVERVIEW_MEAN_F32 = 2, FU_OVERVIEW_ANY_U8 = 3 };
int fu_map_overviews(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, int bands, int h, int w,
                     int kind, const uint8_t* valid, int nodata_value, int n_levels, void* dst, int64_t dst_elems,
                     uint8_t* valid_dst, fu_stream stream);

/* ---- class-map post-processing (fu_post.hip); no context needed --------------------------------- */
/* Connected components of a uint8 map [h, w] on the device: a component is a maximal set of pixels of equal value joined
 * through 4-neighbours (connectivity 4) or 8-neighbours (8).  labels_out int32 [h, w]: the smallest linear index y * w + x
 * of the pixel's component -- canonical, so two labellings compare bit for bit (postprocess.label_components_host is the
 * statement).  Union-find with integer atomics: exact, reproducible; three launches.  1 <= h, w and h * w <= 2^28.  A
 * rejected call launches nothing. */
int fu_map_components(const uint8_t* map, int h, int w, int connectivity, int32_t* labels_out, fu_stream stream);
/* Bytes of fu_map_sieve's workspace: 16 per pixel (labels, component sizes, a 64-bit donor key); 0 for a size it rejects. */
int64_t fu_sieve_workspace_bytes(int h, int w);
/* Connected-component sieve (postprocess.sieve_host is the statement, bit for bit, stats included).  One pass: components
 * and sizes of the pass's input; a component is small when its size < min_pixels and its value is not frozen_value
 * (-1 = none); a donor of a small component is a component that is not small, not of frozen_value, and shares a pixel
 * edge with it (edges under both connectivities); the small component takes the value of its largest donor, ties to the
 * smallest value, and keeps its own when it has no donor.  `passes` (1..8) passes, each on the previous result.
 * out uint8 [h, w]; out == map (in place) is allowed.  min_pixels <= 1: a copy.  workspace: device memory, 16-byte
 * aligned, >= fu_sieve_workspace_bytes(h, w), contents undefined before and after.  stats_out: device int64 [2] or NULL,
 * ADDED to: [0] components re-valued, [1] pixels changed, summed over the passes.  Five launches per pass, no host read.
 * Every argument is checked before anything is launched: a rejected call leaves out and stats_out untouched. */
int fu_map_sieve(const uint8_t* map, uint8_t* out, int h, int w, int connectivity, int min_pixels, int frozen_value,
                 int passes, void* workspace, int64_t workspace_bytes, int64_t* stats_out, fu_stream stream);

/* Vector output (fu_vector.hip; added within ABI 5: purely additive).  floodplanet_code_amd/vectorize.py holds the numpy
 * statements, edge_offsets_host and edge_rings_host, and the definitions: a pixel whose value v has select[v] != 0 (select:
 * HOST uint8 [256]) owns a directed unit edge on every side -- 0 top, 1 right, 2 bottom, 3 left, heading E, S, W, N with the
 * pixel on its right -- where the neighbour lies outside the map or has another value; edges are numbered by owner pixel
 * y * w + x, then side.  Everything is integer-exact and canonical.  1 <= h, w and h * w <= FU_MAP_MAX_PIXELS, so the edge
 * count is at most 2^30 and every vertex index y * (w + 1) + x fits an int32.
 * fu_map_edge_offsets: offsets_out device int32 [h * w + 1] = the exclusive prefix sum of the per-pixel edge counts; the
 * last element is n_edges.  Three launches (block-local scan with block totals, scan of the totals, add) ordered by the
 * stream; no workgroup waits for another.  workspace: device, 16-byte aligned, >= fu_map_edges_workspace_bytes(h, w)
 * (4 B per 2048 pixels; 0 for a size the call rejects). */
int64_t fu_map_edges_workspace_bytes(int h, int w);
int fu_map_edge_offsets(const uint8_t* map, int h, int w, const uint8_t* select /* host [256] */,
                        int32_t* offsets_out /* device [h*w+1] */, void* workspace, int64_t workspace_bytes, fu_stream stream);
/* fu_map_edge_rings: labels = fu_map_components of the map under `connectivity`, offsets = fu_map_edge_offsets of the map
 * and select.  The five outputs are device int32 [capacity]: start (the edge's start vertex), comp (its owner's label),
 * ring (the smallest edge index on the edge's cycle under the successor rule of vectorize.py), rank (the steps from that
 * edge), flags (heading | corner << 2; corner: the predecessor has another heading).  One emit launch, then pointer
 * jumping with ping-pong buffers, ceil(log2(max(capacity, 2))) rounds for ring and as many for rank; no host read.  The
 * kernels take n = offsets[h * w] on the device: n > capacity writes nothing, otherwise every store and every gather
 * through the successor array is guarded by n and elements at n and beyond stay untouched, so a stale offsets array
 * can give wrong rings but no access outside the buffers.  capacity == 0 launches nothing.  workspace: device, 16-byte
 * aligned, >= fu_map_rings_workspace_bytes(capacity) (20 B per edge; 0 for a capacity outside 0..2^30).
 * Both calls check every argument before anything is launched -- null pointers, sizes, connectivity, workspace bytes and
 * alignment -- and a rejected call leaves the outputs untouched. */
int64_t fu_map_rings_workspace_bytes(int64_t capacity);
int fu_map_edge_rings(const uint8_t* map, const int32_t* labels, int h, int w, const uint8_t* select, int connectivity,
                      const int32_t* offsets, int64_t capacity, int32_t* start_out, int32_t* comp_out, int32_t* ring_out,
                      int32_t* rank_out, int32_t* flags_out, void* workspace, int64_t workspace_bytes, fu_stream stream);

/* ---- eval metrics ---------------------------------------------------------------------------- */
/* Per-sample confusion counts of the last fu_forward (eval or training): counts_out[b][t * k + p] += #pixels of sample b
 * with target t and p = argmax of the resident logits (first maximum wins, as fu_loss_ce), over pixels whose target is
 * neither ignore_index nor out of [0, k).  counts_out: int64 [last batch][k][k] (k = n_classes), ADDED to.  No loss, no
 * logits gradient; one launch, integer atomics (exact). */
int fu_eval_confusion(fu_ctx* ctx, const int64_t* target, int ignore_index, int64_t* counts_out, fu_stream stream);

/* Histogram of class probability against target class, one pass, for threshold sweeps and calibration
 * (floodplanet_code_amd/calibration.py).  Both outputs are int64, ADDED to, and at least one must be given:
 *   hist_out [k][k][n_bins]: hist_out[c][t][b] += #pixels with target t whose probability of class c falls in bin b;
 *   top_out  [2][n_bins], optional: row 1 counts the pixels whose argmax (first maximum wins) equals the target, row 0 the
 *            others, binned by the winning probability.
 * A pixel counts when its target is neither ignore_index nor out of [0, k): the rule of fu_eval_confusion.
 * Bin rule.  n_bins is a power of two in 2..1024.  s = p * n_bins in fp32 -- exact, a power of two only moves the
 * exponent -- and bin = s >= 1 ? min((int)s, n_bins - 1) : 0.  So for 1 <= j < n_bins: bin >= j exactly when s >= j exactly
 * when p >= j / n_bins, and j / n_bins is itself an fp32 number: a sweep over the histogram's cumulative sums equals, count
 * for count, thresholding the fp32 probabilities at T = j / n_bins (and T = 0 keeps every counted pixel).  A NaN and a
 * negative probability go to bin 0 (a NaN never passes p >= T for T > 0), p == 1 and anything above go to the last bin.
 * Integer counts: exact and order-free, so everything derived from the histogram is reproducible bit for bit, and the
 * tests compare with equality, without a tolerance.
 * Limits, all checked before anything is launched (a rejected call launches nothing and leaves the outputs untouched):
 * k in 1..8; n_pixels >= 1; one histogram copy, (k * k + 2) * n_bins * 4 bytes, must fit the FU_PROB_HIST_LDS_BYTES the
 * kernel reserves at most (gfx950's LDS per workgroup; k = 8 goes up to 512 bins, k <= 6 up to 1024).
 * One launch, no finalisation pass, no host read: LDS bins per wave, lanes of one bin pre-aggregated by ballot, 64-bit
 * integer atomics for the non-zero bins. */
#define FU_PROB_HIST_LDS_BYTES 163840
/* The probabilities of the resident logits of the last fu_forward / fu_forward_srcs / fu_forward_views (all samples of
 * that batch, k = n_classes; target int64 [last batch, H, W]): p[c] = e[c] * inv, the softmax terms of fu_stitch_add with
 * the product rounded on its own (nothing contracts into an fma) -- bit for bit what fu_merge_views writes to probs_out
 * for one view of code 0.  That identity is this entry point's test oracle: fu_prob_hist on those probabilities gives
 * the same counts. */
int fu_eval_prob_hist(fu_ctx* ctx, const int64_t* target, int ignore_index, int n_bins, int64_t* hist_out,
                      int64_t* top_out, fu_stream stream);
/* The same over any fp32 probabilities [n_pixels, n_classes] (fu_merge_views' probs_out, a normalised canvas); needs no
 * context.  probs 4-byte aligned (16-byte loads are used where the alignment allows), target int64 [n_pixels]. */
int fu_prob_hist(const float* probs, const int64_t* target, int64_t n_pixels, int n_classes, int ignore_index, int n_bins,
                 int64_t* hist_out, int64_t* top_out, fu_stream stream);

/* ---- introspection ------------------------------------------------------------------------- */
int64_t fu_workspace_bytes(const fu_ctx* ctx);
/* algorithmic conv FLOPs of one tile: forward, and forward+backward */
int fu_flops_per_tile(const fu_ctx* ctx, double* fwd, double* train);

/* ---- profiling: HIP events around the convolution kernels (bench.py's roofline object) -------- */
enum fu_kernel_class {
  FU_K_CONV3X3 = 0, /* implicit-GEMM 3x3 conv kernels: forward and dgrad launches (16-bit: k_conv3x3_*_rs + k_conv3x3_*_fast) */
  FU_K_WGRAD = 1,   /* weight-gradient kernel (without its slab reduce) */
  FU_K_NUM = 2
};
/* enable == 1: allocate/reset the event pool and time every launch of the classes above on the stream it is
 * launched on; enable == 2: resume without dropping what was recorded (sampling some steps of a run: an event pair
 * around every launch costs ~2 us of serialisation each, 4 % of the bench step when every step is timed);
 * enable == 0: stop.  fu_profile_read synchronises the device and sums what was recorded. */
int fu_profile_enable(fu_ctx* ctx, int enable);
int fu_profile_read(fu_ctx* ctx, int kernel_class, int64_t* launches, double* total_ms, double* total_flops,
                    const char** kernel_name);

/* ---- TEST HOOKS: process-wide switches that let the parity tests run every shape on every kernel variant.  NOT part of
 * the stable ABI (no version bump when they change); never needed by a caller. -------------------------------------- */
/* Testing hook: on != 0 makes every bf16 3x3 convolution (forward / dgrad) run on the general kernel even when the
 * shape is eligible for the aligned-shape fast kernel, so that the parity tests can cover both.  Process-wide. */
void fu_test_force_general_conv(int on);
/* Testing hook: on = 1 runs the bf16 weight gradient of c_in > 64 on the lock-step kernel k_wgrad_bf16<4,8> instead of
 * the ping-pong kernel k_wgrad_bf16_pp, on = 2 keeps the ping-pong kernel but with its general (any-shape) staging where
 * the whole-tile staging would be chosen (same accumulation order: all three are bit-identical).  Process-wide. */
void fu_test_force_lockstep_wgrad(int on);
/* Testing hook: workgroup tile of the aligned-shape bf16 conv kernel at 64 output channels: 0 = heuristic (default),
 * 1 = never the tall 16x32-pixel tile (nor the row-stationary kernel), 2 = the tall tile wherever 64-channel tiles run,
 * 3 = the row-stationary kernel (fu_conv_rs.hip) wherever the shape is eligible, 4 = the persistent ping-pong kernel
 * (fu_conv_pp.hip) wherever the shape is eligible.  Modes 1-4 also keep the first conv off its 8-channel kernel; the
 * one-tap and the general kernel's launches are not affected.  Process-wide. */
void fu_test_conv_tile_mode(int mode);
/* Testing hook: on != 0 computes every BatchNorm-backward pair of sums with its own reduce pass; by default the 16-bit
 * modes take them from the kernel that produces the gradient where it can (row-stationary dgrad, head backward).
 * Process-wide. */
void fu_test_bnb_separate(int on);
/* Testing hook: on != 0 makes the head backward store its data gradient g = dlogits . W even where (16-bit modes, fused
 * sums) the BatchNorm-backward apply pass of the last conv would recompute it from dlogits and W.  Process-wide. */
void fu_test_head_store_g(int on);
/* Testing hook: on != 0 runs the late-fusion 1x1 convs (weights embedded as the centre tap of a 3x3) through all nine taps
 * instead of the 1-tap instantiation of the fast kernel; the other eight taps multiply exact zeros, so the results are
 * bit-identical.  Process-wide. */
void fu_test_force_full_taps(int on);
/* Testing hook: on != 0 makes fu_op_conv3x3_fwd, fu_op_conv3x3_dgrad and fu_op_conv3x3_wgrad mark their launch as an embedded
 * 1x1 (ConvIn::center_only, the late-fusion convs): the caller's weights must be zero off the centre tap, the 16-bit launches
 * take the one-tap routes (unless fu_test_force_full_taps) and the weight gradient's other taps come back as 0.  Process-wide. */
void fu_test_op_center_only(int on);
/* Testing hook: the tile height (8 or 4 rows of 16 pixels) of the fp32 forward / dgrad kernel for a launch of this shape with N
 * output channels -- the launcher's own choice, asked without a launch. */
int fu_test_conv_f32_tile_rows(int B, int H, int W, int N);

/* Testing hook: which kernel a 16-bit 3x3 conv launch of these shapes runs under the switches currently set -- the launcher's
 * own decision, asked without a launch (no HIP call: works without a GPU).  kind 0 = forward (bias and statistics), 1 =
 * dgrad (want_bnsums: the launch is asked for fused BatchNorm-backward sums), 2 = weight gradient (D0 = c_out; D1 and
 * want_bnsums ignored).  has_bn0: source 0 carries a BatchNorm + ReLU prologue; C1 / D1 = 0: no second source /
 * destination.  Returns the route id (-1: unknown kind); fu_test_conv_route_name names it ("pp", "rs8", "fast32", ...). */
int fu_test_conv_route(int kind, int C0, int has_bn0, int C1, int D0, int D1, int center_only, int want_bnsums, int B,
                       int H, int W);
const char* fu_test_conv_route_name(int kind, int route);
/* Testing hook: the weight-gradient route as above, the split-K slab elements its launch writes (used_elems) and the
 * bound the workspace is sized from (bound_elems). */
int fu_test_wgrad_slab(int C0, int has_bn0, int C1, int Cout, int center_only, int B, int H, int W, int64_t* used_elems,
                       int64_t* bound_elems);

/* Testing hook: every BatchNorm-backward pair of sums that a producer kernel emitted (row-stationary dgrad epilogue, head
 * backward) is multiplied by `factor` before it is consumed -- the negative control of the parity tests (a wrong fused sum
 * must make them fail).  1 = off.  Process-wide. */
void fu_test_perturb_bnb_sums(float factor);
/* Testing hook: device pointer and element count (at max_batch) of one saved tensor of plan block `block` (0..4 = inc,
 * down1..4; 5..8 = up1..4 for the plain UNet): which 0 = y of the first conv, 1 = its gradient buffer, 2 / 3 = the same
 * for the second conv, 4 = dL/d(pooled input) (down blocks), 5 = dL/d(upsampled input) (up blocks).  Elements are of
 * the context's precision. */
int fu_test_get_buffer(fu_ctx* ctx, int block, int which, void** ptr, int64_t* elems);
/* Testing hook: the context's resident fp32 NHWC logits [B, H, W, n_classes] (what fu_forward leaves and fu_loss_* reads),
 * the stored loss gradient of the same shape (what fu_loss_* writes in training mode) and their element count at
 * max_batch.  The op-level loss tests copy constructed logits over the resident ones after a forward, call one fu_loss_*
 * entry and read the gradient back; nothing in the library calls this. */
int fu_test_loss_buffers(fu_ctx* ctx, float** logits, float** dlogits, int64_t* elems);
/* Testing hook: where one packed 3x3 weight copy of the context lives and what it was packed from -- what the forward /
 * dgrad kernels of a real step read (fu_forward packs when the parameters changed or the mode switched; the pack of eval mode
 * has the BatchNorm behind the conv folded in).  Read-only: launches nothing, synchronises nothing.
 *   kind 0  a block's double conv: index = plan block (0 .. 5 nE + 3: per encoder inc, down1..4, then up1..4), which = 0 | 1
 *   kind 1  a late-fusion level's 1x1 conv embedded as a centre tap: index = level 0..4, which = 0; c_in = nE * c_out
 *   kind 2  an up block's ConvTranspose2d(2, 2) as a 1x1 conv to 4 c_out phase-major channels: index = plan block of
 *           up1..4, which = 0; c_out here is 4 * (the transposed conv's c_out), bias4[(p, co)] = bias[co], p = 2 ky + kx
 * present = 0 (everything else zero, the indices -1): the net has no such pack (kind 1 on a plain UNet, kind 2 on a
 * bilinear net).  Bad indices and null arguments: FU_ERR_INVALID.
 * Each copy holds 9 * cin_pad * cout elements of the context's precision, value w[co][ci][tap] (tap = 3 ky + kx; zero for
 * ci >= cin_real; times fold_scale[co] in eval mode, in fp32, then rounded once):
 *   bf16 / fp16   wf[tap][co][ci_pad]   wd[8 - tap][ci_pad][co]
 *   fp32          wf[tap][ci_pad][co]   wd[8 - tap][co][ci_pad]
 * wd is null for the first conv of an encoder (nothing needs its data gradient).  kind 0 only: fold_scale = gamma /
 * sqrt(running_var + eps) and fold_bias = fma(fold_scale, bias, beta - running_mean * fold_scale), written by the eval pack,
 * and a / b, the activation coefficients of the conv's consumers (1 / 0 after an eval pack); each [cout] fp32.
 * p_weight / p_bias: fu_param_info indices; bn: fu_bn_info index (-1: no BatchNorm behind this conv). */
typedef struct fu_test_pack {
  void* wf;
  void* wd;
  float* fold_scale;
  float* fold_bias;
  float* a;
  float* b;
  float* bias4;
  int32_t present, cout, cin_real, cin_pad, p_weight, p_bias, bn, reserved;
} fu_test_pack;
int fu_test_get_pack(fu_ctx* ctx, int kind, int index, int which, fu_test_pack* out);

/* ---- single operators (per-op parity tests; NHWC device buffers of the context's precision) -- */
/* element size of the activation type for `precision` */
int fu_elem_size(int precision);
/* fp32 NCHW -> NHWC (channels zero-padded to c_pad) and back (drops padding) */
int fu_op_nchw_to_nhwc(int precision, const float* src, void* dst, int B, int C, int H, int W, int c_pad,
                       fu_stream stream);
int fu_op_nhwc_to_nchw(int precision, const void* src, float* dst, int B, int C, int H, int W, int c_pad,
                       fu_stream stream);
/* The five operators below are test hooks of the layout kernels (like the fu_test_* switches: no ABI promise).  Each checks
 * every argument before it launches (FU_ERR_INVALID, the cause in fu_last_error, nothing launched) and none synchronises.
 * V = 4 (FU_F32) or 8 (16-bit) elements per 16-byte vector.
 * fu_op_nchw_to_nhwc on a channel window: dst [B,H,W,c_pad] <- channels [src_channel_offset, src_channel_offset + C) of
 * an fp32 NCHW tensor with src_channels per sample (0 = C), zeros above C.  Launches k_nchw_to_nhwc_v8 for a 16-bit type
 * with c_pad % 8 == 0 and k_nchw_to_nhwc otherwise, as every encoder's input conversion does. */
int fu_op_nchw_to_nhwc_window(int precision, const float* src, void* dst, int B, int C, int H, int W, int c_pad,
                              int src_channels, int src_channel_offset, fu_stream stream);
/* dst [B,H,W,c_pad] <- channels [ch_off, ch_off + C) of the n_src (1..8) fp32 NCHW tensors srcs[k] [B,src_channels[k],H,W]
 * taken side by side along the channel axis, zeros above C; c_pad a multiple of V.  n_views == 0 launches
 * k_gather_nchw_to_nhwc (the input conversion of fu_forward_srcs).  n_views in 1..8 launches k_gather_views_nchw_to_nhwc
 * (fu_forward_views): dst [n_views * B,H,W,c_pad], sample v * B + b = view view_codes[v] (0..7, repeats allowed here) of
 * sample b; a transposing code needs H == W. */
int fu_op_gather_nchw_to_nhwc(int precision, const float* const* srcs, const int32_t* src_channels, int n_src, void* dst,
                              int B, int C, int H, int W, int c_pad, int ch_off, int n_views, const int32_t* view_codes,
                              fu_stream stream);
/* k_copy_channels, the late-fusion concat and the split of its gradient: dst [npix][dstC] channels [dst_off, dst_off + C)
 * <- src [npix][srcC] channels [src_off, src_off + C), as they are (bn_a, bn_b null) or as relu(bn_a[c] * x + bn_b[c]) with
 * c counted from the window's start (both fp32 [C]; given together).  Every channel count and offset a multiple of V; the
 * rest of dst is not written. */
int fu_op_copy_channels(int precision, const void* src, int srcC, int src_off, const float* bn_a, const float* bn_b,
                        void* dst, int dstC, int dst_off, int C, int64_t npix, fu_stream stream);
/* k_center_to_w3: w3 [n][9] fp32 <- w [n] on tap 4 (the centre of a 3x3 kernel), +0.0 on the other eight.
 * k_center_from_w3: dw [n] <- dw3 [n][9]'s tap 4; the other taps are not read. */
int fu_op_center_to_w3(const float* w, int64_t n, float* w3, fu_stream stream);
int fu_op_center_from_w3(const float* dw3, int64_t n, float* dw, fu_stream stream);
/* y = conv3x3(cat(relu(a0*src0+b0) or src0, src1), w) + bias; w: fp32 OIHW [Cout, C0+C1, 3, 3].
 * stats_sum/stats_sqsum: optional fp32 [Cout] outputs (per-channel sum / sum of squares of y - bias). */
int fu_op_conv3x3_fwd(int precision, const void* src0, int C0, const float* bn_a0, const float* bn_b0,
                      const void* src1, int C1, const float* w_oihw, const float* bias, void* y, int Cout, int B,
                      int H, int W, float* stats_sum, float* stats_sqsum, fu_stream stream);
/* dx = conv3x3_transpose(dy, w): dx0 gets input channels [0,C0), dx1 gets [C0,C0+C1) */
int fu_op_conv3x3_dgrad(int precision, const void* dy, int Cout, const float* w_oihw, void* dx0, int C0, void* dx1,
                        int C1, int B, int H, int W, fu_stream stream);
/* dw (fp32 OIHW) = sum_p x[p+tap] * dy[p], x assembled exactly as in fu_op_conv3x3_fwd */
int fu_op_conv3x3_wgrad(int precision, const void* src0, int C0, const float* bn_a0, const float* bn_b0,
                        const void* src1, int C1, const void* dy, int Cout, float* dw_oihw, int B, int H, int W,
                        fu_stream stream);
int fu_op_maxpool2(int precision, const void* src, const float* bn_a, const float* bn_b, void* dst, int B, int H,
                   int W, int C, fu_stream stream);
/* bilinear x2, align_corners=True, result zero-padded (F.pad) to [outH, outW] */
int fu_op_upsample2(int precision, const void* src, const float* bn_a, const float* bn_b, void* dst, int B, int H,
                    int W, int C, int outH, int outW, fu_stream stream);
/* The three operators below are test hooks like the fu_test_* switches (no ABI promise).  Each checks its arguments
 * (precision, null pointers, C a multiple of the kernel's channel vector, target >= 2x the source) before its first HIP
 * call and synchronises the stream before it returns.
 * backward of fu_op_upsample2 without the prologue: g_src [B,H,W,C] = bilinear^T(crop(g_dst [B,outH,outW,C])); the pad
 * region of g_dst is ignored.  C: a multiple of 4 (fp32) or 8 (16-bit). */
int fu_op_upsample2_bwd(int precision, const void* g_dst, void* g_src, int B, int H, int W, int C, int outH, int outW,
                        fu_stream stream);
/* the two shuffles of ConvTranspose2d(k=2, s=2): up [B,outH,outW,C] = the four phases of y4 [B,h,w,4C] (channel
 * (2 ky + kx) C + c -> pixel (2y+ky, 2x+kx)) placed at the F.pad offset with zeros around it, and its adjoint
 * g4 [B,h,w,4C] from gup [B,outH,outW,C], which drops the pad.  Pure copies; C a multiple of 4. */
int fu_op_depth_to_space(int precision, const void* y4, void* up, int B, int h, int w, int C, int outH, int outW,
                         fu_stream stream);
int fu_op_space_to_depth(int precision, const void* gup, void* g4, int B, int h, int w, int C, int outH, int outW,
                         fu_stream stream);

/* The operators below exist for the code that only runs in the benched 16-bit dispatch (they are test hooks like the
 * fu_test_* switches: no ABI promise).
 * dgrad as fu_op_conv3x3_dgrad with ONE destination that is the output gradient of a BatchNorm+ReLU whose raw input is y
 * [B,H,W,C0] and whose coefficients are bn_a / bn_b / mean / invstd: also returns that BatchNorm's backward sums
 * sum_gm[c] = sum_p g*m and sum_gmx[c] = sum_p g*m*xhat (m = [a*y+b > 0], xhat = (y-mean)*invstd), taken from the conv
 * kernel's epilogue (BnbFuse).  FU_ERR_UNSUPPORTED when the kernel that ran does not emit them (select the
 * row-stationary kernel with fu_test_conv_tile_mode(3)). */
int fu_op_conv3x3_dgrad_bnsums(int precision, const void* dy, int Cout, const float* w_oihw, void* dx, int C0,
                               const void* y, const float* bn_a, const float* bn_b, const float* mean,
                               const float* invstd, float* sum_gm, float* sum_gmx, int B, int H, int W,
                               fu_stream stream);
/* The two head operators (OutConv 1x1) check every argument before their first HIP call -- precision, null pointers,
 * ncls in 1..8, C one of V, 2V, 4V, 8V, 16V with V = 4 (fp32) or 8 (16-bit) channels per vector, empty shapes -- and
 * synchronise the stream before they return.
 * head forward: logits[p][k] = bias[k] + sum_c z[p][c] * w[k][c] with z = relu(bn_a * y + bn_b), or z = y when bn_a and bn_b
 * are both null; y [B,H,W,C] of `precision`, w fp32 [ncls][C], logits fp32 NHWC [B,H,W,ncls] and, unless logits_nchw is
 * null, the same values as NCHW [B,ncls,H,W]. */
int fu_op_head_fwd(int precision, const void* y, const float* bn_a, const float* bn_b, const float* w, const float* bias,
                   int C, int ncls, int B, int H, int W, float* logits_nhwc, float* logits_nchw, fu_stream stream);
/* head backward: g = dlogits * W (element type of `precision`), dw [ncls][C], db [ncls]; z as in the forward (bn_a / bn_b
 * both null: z = y).  With mean / invstd / sum_gm / sum_gmx non-null (all four or none; needs bn_a / bn_b) also the
 * BatchNorm-backward sums of g as above: 16-bit precisions only, FU_ERR_UNSUPPORTED in fp32. */
int fu_op_head_bwd(int precision, const float* dlogits_nhwc, const void* y, const float* bn_a, const float* bn_b,
                   const float* w, int C, int ncls, int64_t npix, void* g, float* dw, float* db, const float* mean,
                   const float* invstd, float* sum_gm, float* sum_gmx, fu_stream stream);
/* BatchNorm + ReLU backward in place: g holds dL/d relu(bn(y)) on entry and dL/dy on return; g_pool (optional,
 * [B,H/2,W/2,C]) = dL/d maxpool2(relu(bn(y))), whose backward is folded in (first-maximum tie rule). */
int fu_op_bn_bwd(int precision, void* g, const void* y, int C, int B, int H, int W, const float* bn_a,
                 const float* bn_b, const float* mean, const float* invstd, const void* g_pool, float* dgamma,
                 float* dbeta, fu_stream stream);
/* The BatchNorm test hooks below, and fu_op_bn_bwd and fu_op_maxpool2, check every argument before their first allocation
 * or HIP call: precision, null operands, optional groups given whole, B, H, W > 0 (the pool: H, W >= 2), and for the
 * backward 4 <= C <= 1024 with C % 4 == 0 (pooled: C / 4 divides 256, no external sums, no head; head: a 16-bit type,
 * C / 8 divides 256, ncls in 1..8, external sums present).
 * fu_op_bn_bwd with optional extras (fu_op_bn_bwd is this call without them):
 *   ext_sums [ext_rows][C][2]: the two sums per row as their producer (a dgrad or the head backward) left them; the
 *     reduce pass is skipped.  Null with ext_rows = 0.
 *   head_dl [npix][ncls], head_w [ncls][C], ncls: g = dl . w is recomputed in the apply pass (g is output only).
 *   unscale: a device float installed as the gradient unscale factor (fp16 loss scaling) for this call.
 *   db [C]: the per-block sums of dy (the producing conv's bias gradient) added in fp64 in block order, rounded once.
 *   coef [C][2]: s1 / N and s2 / N as the apply pass reads them.
 *   two_level != 0: the sums are finalised by the two-launch form of the exact data-parallel mode, with one rank. */
int fu_op_bn_bwd_ex(int precision, void* g, const void* y, int C, int B, int H, int W, const float* bn_a,
                    const float* bn_b, const float* mean, const float* invstd, const void* g_pool, float* dgamma,
                    float* dbeta, const float* ext_sums, int ext_rows, const float* head_dl, const float* head_w, int ncls,
                    const float* unscale, float* db, float* coef, int two_level, fu_stream stream);
/* BatchNorm forward finalisation from given partial sums: partials [n_part][C][2] fp32 (sum y, sum y*y per tile) over
 * `count` elements per channel -> mean (+ conv_bias, may be null), invstd, a = gamma * invstd, b = beta - mean * a, and,
 * unless null, the running statistics rmean / rvar (null together) and nbt (+1 per call). */
int fu_op_bn_stats(const float* partials, int n_part, int C, int64_t count, const float* conv_bias, const float* gamma,
                   const float* beta, float eps, float momentum, float* mean, float* invstd, float* a, float* b,
                   float* rmean, float* rvar, int64_t* nbt, fu_stream stream);

/* The fp16 loss scale and overflow guard, one operator at a time (test hooks like the fu_test_* switches: no ABI promise).
 * None of the two operators synchronises; every buffer is device memory.
 * out[i] = dlogits[i] * f, dlogits never written.  scale == NULL: f = *up_dev (1 when NULL); partials is not touched.
 * scale != NULL (what an fp16 backward runs): f = *up_dev * S with S = 2^e, e = 6 - frexp(m).exponent for
 * m = max|dlogits| * |*up_dev| over the entries with |x| <= 3.0e38 (e = 0 when m is 0), minus guard[2] when guard is given,
 * clamped to [-60, 60]; scale[0] = S, scale[1] = 1 / S.  partials: at least 256 floats of scratch.  Null dlogits / out /
 * partials or n < 1: FU_ERR_INVALID. */
int fu_op_loss_grad_eff(const float* dlogits, float* out, int64_t n, const float* up_dev, float* partials, float* scale,
                        const int* guard, fu_stream stream);
/* guard[0] |= 1 when an element of g[0..n) is not |x| <= 3.0e38 (inf, NaN and the finite values above it); g at any
 * 4-byte alignment.  book != 0: then the bookkeeping launch of the optimiser step on guard[0..3] = {flag, skipped steps,
 * back-off exponent, clean steps}: a set flag counts a skipped step, raises the exponent (at most 14) and clears the clean
 * count and the flag; otherwise the 64th clean step in a row lowers the exponent (not below 0) and restarts the count. */
int fu_op_fp16_guard(const float* g, int64_t n, int* guard, int book, fu_stream stream);
/* Testing hook: the context's {S, 1 / S} of the last backward and its four guard integers, read after synchronising the
 * device; all zero for a context that is not FU_F16 (as fu_fp16_guard_state). */
int fu_test_fp16_state(fu_ctx* ctx, float scale[2], int32_t guard[4]);
/* Testing hook: writes the guard's back-off exponent (0..14) and clean-step count (0..63) in `stream`'s order, as if that
 * many steps had overflowed / passed.  Outside those ranges, or on a context that is not FU_F16: FU_ERR_INVALID. */
int fu_test_set_fp16_backoff(fu_ctx* ctx, int exponent, int clean_steps, fu_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOODUNET_H_ */
