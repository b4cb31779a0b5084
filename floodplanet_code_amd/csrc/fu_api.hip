// libfloodunet: the C ABI (include/floodunet.h) -- every entry point checks its arguments here and calls into the plan
// (fu_plan.hip), the step (fu_step.hip) or a launcher; the single operators are in fu_ops.hip, the optimiser's entry points
// in fu_optim_api.hip, data parallelism in fu_dp.hip, the context itself in fu_ctx.h.  Also the error-message storage.
//
// Data layout in HBM (all owned by the context, one arena allocation):
//   activations  NHWC, element type = precision (fp32 or bf16); for every 3x3 conv only its RAW output y
//                (pre-BatchNorm) is kept -- BN+ReLU is re-applied by whoever reads y (next conv's staging,
//                pool, upsample, head, and the backward kernels), so normalised tensors never touch HBM.
//   pooled[l], up[k]   the only materialised post-activation tensors (pool / bilinear outputs).
//   gradients    one buffer per y (same shape/type): first holds dL/d relu(bn(y)), then, in place, dL/dy.
//   parameters   caller-owned flat fp32 buffers in reference state_dict order (OIHW); the context keeps
//                packed per-tap copies (forward and tap-reversed dgrad layouts) refreshed after each update.
#include "fu_ctx.h"

#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

using namespace fu;

namespace fu {

// ------------------------------------------------------------------------------------------------
// error message storage
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

}  // namespace fu

namespace {

int check_fwd_args(fu_ctx* c, const float* x, int batch) {
  FU_REQUIRE(c != nullptr, "null context");
  FU_REQUIRE(c->P && c->RM && c->RV && c->NBT, "fu_forward: buffers not bound (fu_bind_buffers)");
  FU_REQUIRE(x != nullptr, "fu_forward: null input");
  FU_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, "fu_forward: batch %d outside 1..%d", batch, c->cfg.max_batch);
  return 0;
}

}  // namespace

// ======================================================================================================
// C ABI
// ======================================================================================================
extern "C" {

int fu_abi_version(void) { return FU_ABI_VERSION; }
const char* fu_last_error(void) { return get_error(); }

int fu_create(const fu_config* cfg, fu_ctx** out) {
  FU_REQUIRE(cfg && out, "fu_create: null argument");
  FU_REQUIRE(cfg->struct_size == (int32_t)sizeof(fu_config), "fu_create: fu_config size mismatch (%d vs %zu)",
             cfg->struct_size, sizeof(fu_config));
  FU_REQUIRE(cfg->n_channels >= 1 && cfg->n_channels <= 64, "n_channels must be 1..64");
  FU_REQUIRE(cfg->n_classes >= 1 && cfg->n_classes <= HEAD_MAX_CLS, "n_classes must be 1..%d", HEAD_MAX_CLS);
  const int b = cfg->base_channels;
  FU_REQUIRE(b == 4 || b == 8 || b == 16 || b == 32 || b == 64, "base_channels must be 4, 8, 16, 32 or 64");
  FU_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
  FU_REQUIRE(cfg->height >= 16 && cfg->width >= 16, "tile must be at least 16x16");
  FU_REQUIRE(cfg->precision == FU_F32 || cfg->precision == FU_BF16 || cfg->precision == FU_F16, "unknown precision %d",
             cfg->precision);
  FU_REQUIRE(cfg->bilinear || b == 64, "bilinear=0 exists only at base_channels 64 (the reference's UNetDecoder "
             "channel plan is inconsistent for bilinear=False, unet.py:176-183)");
  FU_REQUIRE(cfg->precision == FU_F32 || b >= 8, "bf16 / fp16 precision needs base_channels >= 8");
  FU_REQUIRE(cfg->n_encoders >= 0 && cfg->n_encoders <= FU_MAX_ENCODERS, "n_encoders must be 0..%d", FU_MAX_ENCODERS);
  if (cfg->n_encoders >= 1) {
    FU_REQUIRE(cfg->bilinear, "late fusion exists only with bilinear upsampling (lf_model.py:38)");
    int sum = 0;
    for (int e = 0; e < cfg->n_encoders; ++e) {
      FU_REQUIRE(cfg->enc_channels[e] >= 1, "enc_channels[%d] must be >= 1", e);
      sum += cfg->enc_channels[e];
    }
    FU_REQUIRE(sum == cfg->n_channels, "enc_channels sum to %d, n_channels is %d", sum, cfg->n_channels);
  }
  FU_HIP_CHECK(hipSetDevice(cfg->device));
  fu_ctx* c = new (std::nothrow) fu_ctx();
  FU_REQUIRE(c, "out of host memory");
  c->cfg = *cfg;
  c->prec = cfg->precision == FU_F32 ? PREC_F32 : (cfg->precision == FU_BF16 ? PREC_BF16 : PREC_F16);
  c->esize = c->prec == PREC_F32 ? 4 : 2;
  int st = build_plan(c);
  if (st == 0) st = alloc_workspace(c);
  // side stream for the weight-gradient chain (bilinear nets; the ConvTranspose variant shares the slab with its own
  // wgrad on the main stream).  FU_NO_SIDE_STREAM=1 keeps everything on the caller's stream.
  // (bf16 only: in fp32 mode the concurrency changes nothing in the step time -- both kernels are MFMA bound at 0.7 of
  //  the fp32 peak -- and only inflates the per-launch durations of the parity build)
  if (st == 0 && c->cfg.bilinear && c->prec != fu::PREC_F32 && !getenv("FU_NO_SIDE_STREAM")) {
    int plo = 0, phi = 0;
    (void)hipDeviceGetStreamPriorityRange(&plo, &phi);      // plo = the lowest priority (numerically largest)
    if (hipStreamCreateWithFlags(&c->side_def, hipStreamNonBlocking) != hipSuccess) c->side_def = nullptr;
    if (c->side_def && hipStreamCreateWithPriority(&c->side_lo, hipStreamNonBlocking, plo) != hipSuccess)
      c->side_lo = nullptr;
    c->side = c->side_lo ? c->side_lo : c->side_def;        // side_mode starts at 1
    if (c->side) {
      bool ok = hipEventCreateWithFlags(&c->ev_gy, EVENT_FLAGS) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_blk, EVENT_FLAGS) == hipSuccess;
      if (!ok) {
        if (c->side_lo) (void)hipStreamDestroy(c->side_lo);
        (void)hipStreamDestroy(c->side_def);
        c->side = c->side_lo = c->side_def = nullptr;
      }
    }
    if (c->side) {
      // the private split-K workspace of a backward's last weight-gradient chain (backward_conv): only beside a side
      // stream; without the memory that chain goes to the side stream like every other one
      const Conv& v = c->blk[0].c[0];
      const size_t bytes = conv3x3_wgrad_slab_elems(c->prec, v.cin_pad, v.cout, c->cfg.max_batch, c->Hs[0], c->Ws[0]) * sizeof(float);
      void* p = nullptr;
      if (hipMalloc(&p, bytes) == hipSuccess) {
        c->slab_tail = (float*)p;
        c->extra_allocs.push_back(p);
      } else {
        (void)hipGetLastError();
      }
    }
  }
  if (st != 0) { fu_destroy(c); return st; }
  *out = c;
  return FU_OK;
}

int fu_destroy(fu_ctx* c) {
  if (!c) return FU_OK;
  (void)hipSetDevice(c->cfg.device);
  (void)hipDeviceSynchronize();
  (void)fu_dp_destroy(c);
  for (hipEvent_t e : c->prof.pool) (void)hipEventDestroy(e);
  if (c->side) {
    if (c->side_lo) (void)hipStreamDestroy(c->side_lo);
    if (c->side_def) (void)hipStreamDestroy(c->side_def);
    for (hipEvent_t e : {c->ev_gy, c->ev_blk}) if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : c->ev_fence) if (e) (void)hipEventDestroy(e);   // (fu_backward_fence creates them without a side stream too)
  if (c->arena.base) (void)hipFree(c->arena.base);
  for (void* p : c->extra_allocs) (void)hipFree(p);
  c->stitch_table.release();
  c->scene_table.release();
  c->train_table.release();
  delete c;
  return FU_OK;
}

int fu_num_params(const fu_ctx* c) { return c ? (int)c->params.size() : 0; }
int64_t fu_total_param_elems(const fu_ctx* c) { return c ? c->total_params : 0; }
int fu_param_info(const fu_ctx* c, int index, const char** name, int32_t* ndim, int64_t shape[4], int64_t* flat_offset) {
  FU_REQUIRE(c && index >= 0 && index < (int)c->params.size(), "fu_param_info: bad index %d", index);
  const ParamInfo& p = c->params[index];
  if (name) *name = p.name.c_str();
  if (ndim) *ndim = p.ndim;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
  if (flat_offset) *flat_offset = p.off;
  return FU_OK;
}
int fu_num_bn(const fu_ctx* c) { return c ? (int)c->bns.size() : 0; }
int64_t fu_total_bn_channels(const fu_ctx* c) { return c ? c->total_bn : 0; }
int fu_bn_info(const fu_ctx* c, int index, const char** name, int32_t* channels, int64_t* flat_offset) {
  FU_REQUIRE(c && index >= 0 && index < (int)c->bns.size(), "fu_bn_info: bad index %d", index);
  if (name) *name = c->bns[index].name.c_str();
  if (channels) *channels = c->bns[index].C;
  if (flat_offset) *flat_offset = c->bns[index].off;
  return FU_OK;
}

int fu_bind_buffers(fu_ctx* c, float* params, float* grads, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked) {
  FU_REQUIRE(c && params && running_mean && running_var && num_batches_tracked, "fu_bind_buffers: null buffer");
  c->P = params; c->G = grads; c->RM = running_mean; c->RV = running_var; c->NBT = num_batches_tracked;
  c->packed_dirty = true;
  c->pack_tabs.clear();
  return FU_OK;
}
int fu_params_changed(fu_ctx* c) {
  FU_REQUIRE(c, "null context");
  c->packed_dirty = true;
  return FU_OK;
}


int fu_set_exact_sync(fu_ctx* c, fu_sync_hook hook, void* user, int world, void* exchange, int64_t exchange_bytes) {
  FU_REQUIRE(c, "null context");
  if (!hook || world <= 1) { c->sync = fu::SyncDesc(); return FU_OK; }
  if (c->prec == PREC_F16) {   // every rank picks its own loss scale: the summed BN-backward statistics would mix scales
    set_error("fu_set_exact_sync: the exact (SyncBN) mode is not available in fp16 precision; use bf16 or fp32");
    return FU_ERR_UNSUPPORTED;
  }
  FU_REQUIRE(exchange && exchange_bytes >= fu_exact_sync_bytes(c), "fu_set_exact_sync: exchange buffer of at least %lld bytes needed",
             (long long)fu_exact_sync_bytes(c));
  c->sync.hook = hook; c->sync.user = user; c->sync.world = world; c->sync.xbuf = exchange; c->sync.xbytes = exchange_bytes;
  return FU_OK;
}
int64_t fu_exact_sync_bytes(const fu_ctx* c) {
  if (!c) return 0;
  int max_c = 64;
  for (const BnInfo& b : c->bns) max_c = std::max(max_c, b.C);
  return std::max<int64_t>(fu::reduce_scratch_elems(max_c) * (int64_t)sizeof(double), 4 * 1024 * (int64_t)sizeof(float));
}

int fu_forward(fu_ctx* c, const float* x, int batch, int training, float* logits_out, fu_stream stream) {
  FU_TRY(check_fwd_args(c, x, batch));
  return forward_impl(c, x, nullptr, batch, training != 0, logits_out, (hipStream_t)stream);
}

namespace {
// the sources of one forward: make_src_list's checks (fu_layout.hip), and their channels add up to the model's
int model_src_list(const fu_ctx* c, const char* fn, const float* const* srcs, const int32_t* src_channels, int n_src,
                   SrcList* S) {
  FU_TRY(make_src_list(fn, srcs, src_channels, n_src, S));
  FU_REQUIRE(S->coff[n_src] == c->cfg.n_channels, "%s: the sources have %d channels in all, the model takes %d", fn,
             S->coff[n_src], c->cfg.n_channels);
  return 0;
}
}  // namespace

int fu_forward_srcs(fu_ctx* c, const float* const* srcs, const int32_t* src_channels, int n_src, int batch, int training,
                    float* logits_out, fu_stream stream) {
  FU_REQUIRE(srcs && src_channels && n_src >= 1 && n_src <= 8, "fu_forward_srcs: 1..8 sources");
  FU_TRY(check_fwd_args(c, srcs[0], batch));
  SrcList S;
  FU_TRY(model_src_list(c, "fu_forward_srcs", srcs, src_channels, n_src, &S));
  return forward_impl(c, nullptr, &S, batch, training != 0, logits_out, (hipStream_t)stream);
}

int fu_forward_views(fu_ctx* c, const float* const* srcs, const int32_t* src_channels, int n_src, int batch, int n_views,
                     const int32_t* codes, float* logits_out, fu_stream stream) {
  FU_REQUIRE(c, "fu_forward_views: null context");
  FU_REQUIRE(srcs && src_channels && n_src >= 1 && n_src <= 8, "fu_forward_views: 1..8 sources");
  unsigned packed = 0;
  FU_TRY(pack_view_codes("fu_forward_views", codes, n_views, true, &packed));
  // the square-tile rule of the transposing codes, in the words of the views gather's launcher (check_view_geometry)
  FU_TRY(check_view_geometry("fu_forward_views", n_views, packed, c->cfg.height, c->cfg.width));
  FU_REQUIRE(batch >= 1 && (int64_t)batch * n_views <= c->cfg.max_batch,
             "fu_forward_views: %d views x batch %d outside 1..%d samples (max_batch)", n_views, batch, c->cfg.max_batch);
  FU_TRY(check_fwd_args(c, srcs[0], batch * n_views));
  SrcList S;
  FU_TRY(model_src_list(c, "fu_forward_views", srcs, src_channels, n_src, &S));
  return forward_impl(c, nullptr, &S, batch * n_views, false, logits_out, (hipStream_t)stream, n_views, packed);
}

int fu_merge_views(fu_ctx* c, float* probs_out, const int64_t* target, int ignore_index, int64_t* counts_out,
                   fu_stream stream) {
  FU_REQUIRE(c, "fu_merge_views: null context");
  FU_REQUIRE(c->view_n > 0, "fu_merge_views: the last forward was not fu_forward_views");
  FU_REQUIRE(probs_out || counts_out, "fu_merge_views: nothing to write (probs_out and counts_out are both null)");
  FU_REQUIRE((target != nullptr) == (counts_out != nullptr), "fu_merge_views: target and counts_out go together");
  return launch_merge_views(c->logits, c->cfg.height, c->cfg.width, c->cfg.n_classes, c->view_batch, c->view_n,
                            c->view_codes, probs_out, target, ignore_index, counts_out, (hipStream_t)stream);
}

namespace {
// fu_loss_ce (cw == null), fu_loss_ce_weighted and fu_loss_ce_focal; fu_loss_ce_region: any of the three, then the region
// term (rg != null) with the same exact-sync descriptor
int loss_ce(fu_ctx* c, const char* who, const int64_t* target, int ignore_index, const CeWeighting* cw, float* loss_out,
            int64_t* confusion_out, int64_t* n_valid_out, fu_stream stream, const RegionTerm* rg = nullptr) {
  FU_REQUIRE(c->last_batch > 0, "%s: no forward pass yet", who);
  hipStream_t s = (hipStream_t)stream;
  const SyncDesc* sync = active_sync(c, c->fwd_training);
  const int64_t npix = (int64_t)c->last_batch * c->cfg.height * c->cfg.width;
  FU_TRY(launch_ce_loss(c->logits, target, c->cfg.n_classes, ignore_index, npix, cw, c->ce_part,
                        loss_out ? loss_out : c->loss_dev, c->n_valid, confusion_out, n_valid_out, c->conf_tmp, sync, s));
  if (c->fwd_training)
    FU_TRY(launch_ce_grad(c->logits, target, c->cfg.n_classes, ignore_index, npix, cw, c->n_valid, c->dlogits, s));
  if (rg)
    FU_TRY(launch_region_term(c->logits, target, c->cfg.n_classes, ignore_index, npix, *rg, c->ce_part,
                              loss_out ? loss_out : c->loss_dev, c->fwd_training ? c->dlogits : nullptr, sync, s));
  if (c->fwd_training) {
    c->have_loss = true;
    c->have_up_scale = false;
  }
  return FU_OK;
}
}  // namespace

int fu_loss_ce(fu_ctx* c, const int64_t* target, int ignore_index, float* loss_out, int64_t* confusion_out,
               int64_t* n_valid_out, fu_stream stream) {
  FU_REQUIRE(c && target, "fu_loss_ce: null argument");
  return loss_ce(c, "fu_loss_ce", target, ignore_index, nullptr, loss_out, confusion_out, n_valid_out, stream);
}

int fu_loss_ce_weighted(fu_ctx* c, const int64_t* target, int ignore_index, const float* class_weight_dev,
                        float label_smoothing, float* loss_out, int64_t* confusion_out, int64_t* n_valid_out,
                        float* weight_sum_out, fu_stream stream) {
  FU_REQUIRE(c && target, "fu_loss_ce_weighted: null argument");
  FU_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "fu_loss_ce_weighted: label_smoothing %g outside [0, 1)",
             (double)label_smoothing);
  const CeWeighting cw = {class_weight_dev, (float)(1.0 - (double)label_smoothing),
                          (float)((double)label_smoothing / c->cfg.n_classes), c->ce_wsum, weight_sum_out};
  return loss_ce(c, "fu_loss_ce_weighted", target, ignore_index, &cw, loss_out, confusion_out, n_valid_out, stream);
}

int fu_loss_ce_focal(fu_ctx* c, const int64_t* target, int ignore_index, const float* class_weight_dev, float focal_gamma,
                     float* loss_out, int64_t* confusion_out, int64_t* n_valid_out, float* weight_sum_out,
                     fu_stream stream) {
  FU_REQUIRE(c && target, "fu_loss_ce_focal: null argument");
  FU_REQUIRE(focal_gamma >= 0.f && focal_gamma < INFINITY, "fu_loss_ce_focal: focal_gamma %g is not a finite number >= 0",
             (double)focal_gamma);                          // (NaN fails both comparisons)
  // gamma == 0: launch_ce_loss / launch_ce_grad run the weighted instantiations -- fu_loss_ce_weighted(eps = 0) itself
  const CeWeighting cw = {class_weight_dev, 1.f, 0.f, c->ce_wsum, weight_sum_out, focal_gamma};
  return loss_ce(c, "fu_loss_ce_focal", target, ignore_index, &cw, loss_out, confusion_out, n_valid_out, stream);
}

int fu_loss_ce_region(fu_ctx* c, const int64_t* target, int ignore_index, const float* class_weight_dev,
                      float label_smoothing, float focal_gamma, const fu_region_loss* region, float* loss_out,
                      int64_t* confusion_out, int64_t* n_valid_out, float* weight_sum_out, float* region_out,
                      fu_stream stream) {
  FU_REQUIRE(c && target, "fu_loss_ce_region: null argument");
  FU_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "fu_loss_ce_region: label_smoothing %g outside [0, 1)",
             (double)label_smoothing);
  FU_REQUIRE(focal_gamma >= 0.f && focal_gamma < INFINITY, "fu_loss_ce_region: focal_gamma %g is not a finite number >= 0",
             (double)focal_gamma);
  FU_REQUIRE(!(focal_gamma > 0.f && label_smoothing != 0.f),
             "fu_loss_ce_region: focal_gamma %g together with label_smoothing %g (a smoothed focal loss is not defined)",
             (double)focal_gamma, (double)label_smoothing);
  RegionTerm rg = {0.f, 0.f, 0.f, 0.f, c->region_coef, region_out};
  if (region) {                                             // (NaN fails every comparison below)
    FU_REQUIRE(region->weight >= 0.f && region->weight < INFINITY,
               "fu_loss_ce_region: region weight %g is not a finite number >= 0", (double)region->weight);
    FU_REQUIRE(region->alpha >= 0.f && region->alpha < INFINITY && region->beta >= 0.f && region->beta < INFINITY &&
                   region->alpha + region->beta > 0.f,
               "fu_loss_ce_region: alpha %g, beta %g must be finite and >= 0, with alpha + beta > 0", (double)region->alpha,
               (double)region->beta);
    FU_REQUIRE(region->smooth > 0.f && region->smooth < INFINITY, "fu_loss_ce_region: smooth %g is not a finite number > 0",
               (double)region->smooth);
    FU_REQUIRE(region->weight == 0.f || c->cfg.n_classes >= 2, "fu_loss_ce_region: a region term needs n_classes >= 2");
    rg.weight = region->weight; rg.alpha = region->alpha; rg.beta = region->beta; rg.smooth = region->smooth;
  }
  const RegionTerm* term = rg.weight > 0.f ? &rg : nullptr;   // weight 0: nothing new is launched, the CE form's own bits
  if (!class_weight_dev && label_smoothing == 0.f && focal_gamma == 0.f)
    return loss_ce(c, "fu_loss_ce_region", target, ignore_index, nullptr, loss_out, confusion_out, n_valid_out, stream, term);
  const CeWeighting cw = focal_gamma > 0.f
                             ? CeWeighting{class_weight_dev, 1.f, 0.f, c->ce_wsum, weight_sum_out, focal_gamma}
                             : CeWeighting{class_weight_dev, (float)(1.0 - (double)label_smoothing),
                                           (float)((double)label_smoothing / c->cfg.n_classes), c->ce_wsum, weight_sum_out};
  return loss_ce(c, "fu_loss_ce_region", target, ignore_index, &cw, loss_out, confusion_out, n_valid_out, stream, term);
}

int fu_loss_bce_dice(fu_ctx* c, const int64_t* target, int ignore_index, float dice_weight, float* loss_out,
                     fu_stream stream) {
  FU_REQUIRE(c && target, "fu_loss_bce_dice: null argument");
  FU_REQUIRE(c->last_batch > 0, "fu_loss_bce_dice: no forward pass yet");
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)c->last_batch * c->cfg.height * c->cfg.width;
  FU_TRY(launch_bce_dice(c->logits, target, c->cfg.n_classes, ignore_index, npix, dice_weight, c->ce_part,
                         c->loss_dev + 8, loss_out ? loss_out : c->loss_dev, c->n_valid,
                         c->fwd_training ? c->dlogits : nullptr, s));
  if (c->fwd_training) { c->have_loss = true; c->have_up_scale = false; }
  return FU_OK;
}

int fu_scale_loss_grad(fu_ctx* c, const float* scale_dev, fu_stream stream) {
  FU_REQUIRE(c && scale_dev, "fu_scale_loss_grad: null argument");
  if (!(c->last_batch > 0 && c->fwd_training && c->have_loss)) {
    set_error("fu_scale_loss_grad: no loss gradient stored (training fu_forward + fu_loss_* first)");
    return FU_ERR_STATE;
  }
  // kept as a device scalar and applied when the backward forms the head's input (backward_block_impl, block 0): the stored
  // gradient is not touched, calling this twice for one loss replaces the factor instead of compounding it
  FU_HIP_CHECK(hipMemcpyAsync(c->up_scale, scale_dev, sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  c->have_up_scale = true;
  return FU_OK;
}

namespace {
// what fu_backward and fu_backward_block need before anything is launched
int check_backward(const fu_ctx* c) {
  if (!(c->last_batch > 0 && c->fwd_training)) {
    set_error("fu_backward: the last fu_forward was not a training forward");
    return FU_ERR_STATE;
  }
  FU_REQUIRE(c->G, "fu_backward: no gradient buffer bound");
  return 0;
}
}  // namespace

int fu_num_blocks(const fu_ctx* c) { return c ? num_backward_blocks(c) : 0; }

int fu_backward_block(fu_ctx* c, int block, const float* dlogits, fu_stream stream) {
  FU_REQUIRE(c, "null context");
  FU_REQUIRE(block >= 0 && block < num_backward_blocks(c), "fu_backward_block: block %d outside 0..%d", block,
             num_backward_blocks(c) - 1);
  FU_TRY(check_backward(c));
  return backward_block_impl(c, block, dlogits, (hipStream_t)stream, c->side_mode != 2);
}

int fu_set_side_stream(fu_ctx* c, int mode) {
  FU_REQUIRE(c && mode >= 0 && mode <= 2, "fu_set_side_stream: mode must be 0, 1 or 2");
  c->side_mode = mode;
  if (c->side) c->side = (mode == 2 || !c->side_lo) ? c->side_def : c->side_lo;
  return FU_OK;
}

int fu_backward_join(fu_ctx* c, fu_stream stream) {
  FU_REQUIRE(c, "null context");
  return join_side(c, (hipStream_t)stream);
}

int fu_backward_fence(fu_ctx* c, fu_stream stream, fu_stream waiter) {
  FU_REQUIRE(c, "null context");
  FU_REQUIRE(stream != waiter, "fu_backward_fence: the waiting stream must not be the compute stream (use fu_backward_join)");
  if (!c->ev_fence[0]) FU_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fence[0], EVENT_FLAGS));
  if (!c->ev_fence[1]) FU_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fence[1], EVENT_FLAGS));
  FU_HIP_CHECK(hipEventRecord(c->ev_fence[0], (hipStream_t)stream));
  FU_HIP_CHECK(hipStreamWaitEvent((hipStream_t)waiter, c->ev_fence[0], 0));
  if (c->side && c->side_mode != 0) {     // (nothing is pending there in mode 1: every block has joined already)
    FU_HIP_CHECK(hipEventRecord(c->ev_fence[1], c->side));
    FU_HIP_CHECK(hipStreamWaitEvent((hipStream_t)waiter, c->ev_fence[1], 0));
  }
  return FU_OK;
}

int fu_backward(fu_ctx* c, const float* dlogits, fu_stream stream) {
  FU_REQUIRE(c, "null context");
  FU_TRY(check_backward(c));
  // whole backward: the side stream (weight gradients) is joined once, after the last block
  const int nblk = num_backward_blocks(c);
  for (int b = 0; b < nblk; ++b) FU_TRY(backward_block_impl(c, b, dlogits, (hipStream_t)stream, b == nblk - 1));
  return FU_OK;
}

int fu_block_param_range(const fu_ctx* c, int block, int64_t* flat_offset, int64_t* numel) {
  FU_REQUIRE(c && block >= 0 && block < num_backward_blocks(c), "fu_block_param_range: bad block %d", block);
  int first, count;
  if (block == 0) { first = c->p_outw; count = 2; }
  else if (c->fusion && block == 5) { first = c->fuse[0].p_w; count = 10; }
  else { const Block& K = c->blk[backward_block_index(c, block)]; first = K.first_param; count = K.num_params; }
  const ParamInfo& a = c->params[first];
  const ParamInfo& z = c->params[first + count - 1];
  if (flat_offset) *flat_offset = a.off;
  if (numel) *numel = z.off + z.numel - a.off;
  return FU_OK;
}

int64_t fu_workspace_bytes(const fu_ctx* c) { return c ? (int64_t)c->arena.total : 0; }

int fu_flops_per_tile(const fu_ctx* c, double* fwd, double* train) {
  FU_REQUIRE(c, "null context");
  if (fwd) *fwd = conv_flops(const_cast<fu_ctx*>(c), false);
  if (train) *train = conv_flops(const_cast<fu_ctx*>(c), true);
  return FU_OK;
}

int fu_profile_enable(fu_ctx* c, int enable) {
  FU_REQUIRE(c, "null context");
  Profiler& pr = c->prof;
  if (enable) {
    const size_t want = 2 * 8192;
    while (pr.pool.size() < want) {
      hipEvent_t e;
      FU_HIP_CHECK(hipEventCreate(&e));
      pr.pool.push_back(e);
    }
    if (enable != 2) {          // 2 = resume: keep the records of the earlier enabled stretches
      pr.next = 0;
      pr.recs.clear();
      pr.overflow = false;
    }
    pr.on = true;
  } else {
    pr.on = false;
  }
  return FU_OK;
}

int fu_profile_read(fu_ctx* c, int kernel_class, int64_t* launches, double* total_ms, double* total_flops,
                    const char** kernel_name) {
  FU_REQUIRE(c && kernel_class >= 0 && kernel_class < FU_K_NUM, "fu_profile_read: bad class %d", kernel_class);
  FU_HIP_CHECK(hipDeviceSynchronize());
  int64_t n = 0;
  double ms = 0.0, fl = 0.0;
  for (const ProfRec& r : c->prof.recs) {
    if (r.cls != kernel_class) continue;
    float t = 0.f;
    FU_HIP_CHECK(hipEventElapsedTime(&t, r.e0, r.e1));
    ms += t; fl += r.flops; ++n;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (kernel_name)
    *kernel_name = kernel_class == FU_K_CONV3X3
                       // 16-bit: the class = every forward / dgrad launch, i.e. k_conv3x3_bf16_rs<8|4> and the
                       // k_conv3x3_bf16_fast<...> instantiations (the common prefix matches them all in a kernel trace)
                       ? (c->prec == PREC_F32 ? "k_conv3x3_f32" : (c->prec == PREC_BF16 ? "k_conv3x3_bf16" : "k_conv3x3_f16"))
                       : (c->prec == PREC_F32 ? "k_wgrad_f32" : (c->prec == PREC_BF16 ? "k_wgrad_bf16" : "k_wgrad_f16"));
  return FU_OK;
}

int fu_stitch_add(fu_ctx* c, int sample, float* canvas, float* weight, int canvas_h, int canvas_w, int h0, int w0,
                  int hE, int wE, fu_stream stream) {
  FU_REQUIRE(c && canvas && weight, "fu_stitch_add: null argument");
  FU_REQUIRE(c->last_batch > 0 && sample >= 0 && sample < c->last_batch, "fu_stitch_add: sample %d not in the last batch",
             sample);
  const int H = c->cfg.height, W = c->cfg.width;
  const int dh = hE - h0, dw = wE - w0;
  FU_REQUIRE(h0 >= 0 && w0 >= 0 && dh >= 0 && dw >= 0 && hE <= canvas_h && wE <= canvas_w && dh <= H && dw <= W,
             "fu_stitch_add: crop [%d:%d, %d:%d] does not fit canvas %dx%d / tile %dx%d", h0, hE, w0, wE, canvas_h,
             canvas_w, H, W);
  if (dh == 0 || dw == 0) return FU_OK;
  const float* lg = c->logits + (int64_t)sample * H * W * c->cfg.n_classes;
  return launch_stitch_add(lg, c->cfg.n_classes, W, canvas, weight, canvas_w, h0, w0, dh, dw, (hipStream_t)stream);
}

int fu_stitch_add_batch(fu_ctx* c, int n, const fu_stitch_entry* entries, fu_stream stream) {
  FU_REQUIRE(c && entries && n > 0, "fu_stitch_add_batch: null context / entries or n = %d <= 0", n);
  FU_REQUIRE(c->last_batch > 0, "fu_stitch_add_batch: no forward pass yet");
  return launch_stitch_add_batch(c->stitch_table, "fu_stitch_add_batch", "last batch", n, entries, c->logits, c->last_batch,
                                 false, c->cfg.height, c->cfg.width, c->cfg.n_classes, (hipStream_t)stream);
}

int fu_stitch_add_batch_probs(fu_ctx* c, int n, const fu_stitch_entry* entries, const float* probs, int batch,
                              fu_stream stream) {
  FU_REQUIRE(c && entries && probs && n > 0 && batch >= 1,
             "fu_stitch_add_batch_probs: null context / entries / probs, n = %d <= 0 or batch = %d < 1", n, batch);
  return launch_stitch_add_batch(c->stitch_table, "fu_stitch_add_batch_probs", "probabilities' batch", n, entries, probs,
                                 batch, true, c->cfg.height, c->cfg.width, c->cfg.n_classes, (hipStream_t)stream);
}

int fu_stitch_add_batch_windowed(fu_ctx* c, int n, const fu_stitch_entry* entries, const float* probs, int batch,
                                 const float* win_y, const float* win_x, fu_stream stream) {
  FU_REQUIRE(c && entries && n > 0, "fu_stitch_add_batch_windowed: null context / entries or n = %d <= 0", n);
  FU_REQUIRE(win_y && win_x, "fu_stitch_add_batch_windowed: null window");
  FU_REQUIRE(!probs || batch >= 1, "fu_stitch_add_batch_windowed: batch = %d < 1", batch);
  FU_REQUIRE(probs || c->last_batch > 0, "fu_stitch_add_batch_windowed: no forward pass yet");
  return launch_stitch_add_batch(c->stitch_table, "fu_stitch_add_batch_windowed", probs ? "probabilities' batch" : "last batch",
                                 n, entries, probs ? probs : c->logits, probs ? batch : c->last_batch, probs != nullptr,
                                 c->cfg.height, c->cfg.width, c->cfg.n_classes, (hipStream_t)stream, win_y, win_x);
}

int fu_eval_confusion(fu_ctx* c, const int64_t* target, int ignore_index, int64_t* counts_out, fu_stream stream) {
  FU_REQUIRE(c && target && counts_out, "fu_eval_confusion: null argument");
  FU_REQUIRE(c->last_batch > 0, "fu_eval_confusion: no forward pass yet");
  return launch_eval_confusion(c->logits, target, c->cfg.n_classes, ignore_index, c->last_batch,
                               (int64_t)c->cfg.height * c->cfg.width, counts_out, (hipStream_t)stream);
}

int fu_stitch_finalize(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w,
                       int64_t* argmax_out, fu_stream stream) {
  FU_REQUIRE(canvas && weight && n_classes >= 1 && n_classes <= HEAD_MAX_CLS, "fu_stitch_finalize: bad argument");
  return launch_stitch_finalize(canvas, weight, n_classes, (int64_t)canvas_h * canvas_w, argmax_out,
                                (hipStream_t)stream);
}

int fu_stitch_finalize_maps(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                            int normalize_in_place, const uint8_t* class_values, uint8_t* class_out, uint8_t* prob_out,
                            uint8_t* margin_out, int64_t* counts_out, fu_stream stream) {
  return fu_stitch_finalize_maps_ex(canvas, weight, n_classes, canvas_h, canvas_w, eps, normalize_in_place, class_values,
                                    class_out, prob_out, margin_out, counts_out, nullptr, stream);
}

// the messages keep fu_stitch_finalize_maps' name as their prefix: it is the forwarder's too
int fu_stitch_finalize_maps_ex(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                               int normalize_in_place, const uint8_t* class_values, uint8_t* class_out, uint8_t* prob_out,
                               uint8_t* margin_out, int64_t* counts_out, const fu_class_threshold* thr, fu_stream stream) {
  return fu_stitch_finalize_maps_masked(canvas, weight, n_classes, canvas_h, canvas_w, eps, normalize_in_place, class_values,
                                        class_out, prob_out, margin_out, counts_out, thr, nullptr, 0, stream);
}

// valid == NULL: fu_stitch_finalize_maps_ex, its checks, its messages and its kernels (nodata_value is not looked at)
int fu_stitch_finalize_maps_masked(float* canvas, const float* weight, int n_classes, int canvas_h, int canvas_w, float eps,
                                   int normalize_in_place, const uint8_t* class_values, uint8_t* class_out, uint8_t* prob_out,
                                   uint8_t* margin_out, int64_t* counts_out, const fu_class_threshold* thr,
                                   const uint8_t* valid, int nodata_value, fu_stream stream) {
  FU_REQUIRE(canvas && weight, "fu_stitch_finalize_maps: null canvas / weight");
  FU_REQUIRE(n_classes >= 1 && n_classes <= HEAD_MAX_CLS, "fu_stitch_finalize_maps: n_classes %d not in 1..%d", n_classes,
             HEAD_MAX_CLS);
  FU_REQUIRE(canvas_h >= 0 && canvas_w >= 0, "fu_stitch_finalize_maps: canvas %dx%d", canvas_h, canvas_w);
  FU_REQUIRE(isfinite(eps) && eps >= 0.f, "fu_stitch_finalize_maps: eps %g is negative or not finite", (double)eps);
  FU_REQUIRE(normalize_in_place || class_out || prob_out || margin_out || counts_out,
             "fu_stitch_finalize_maps: no output requested");
  if (thr) {
    FU_REQUIRE(n_classes >= 2, "fu_stitch_finalize_maps_ex: a threshold needs at least 2 classes, got %d", n_classes);
    FU_REQUIRE(thr->cls >= 0 && thr->cls < n_classes, "fu_stitch_finalize_maps_ex: threshold class %d not in 0..%d",
               (int)thr->cls, n_classes - 1);
    FU_REQUIRE(isfinite(thr->threshold) && thr->threshold >= 0.f && thr->threshold <= 1.f,
               "fu_stitch_finalize_maps_ex: threshold %g is not finite or outside [0, 1]", (double)thr->threshold);
  }
  if (valid) {
    const char* fn = "fu_stitch_finalize_maps_masked";
    FU_REQUIRE(canvas_h >= 1 && canvas_w >= 1 && (int64_t)canvas_h * canvas_w <= FU_MAP_MAX_PIXELS,
               "%s: canvas %dx%d is empty or has more than 2^28 pixels", fn, canvas_h, canvas_w);
    FU_REQUIRE(nodata_value >= 0 && nodata_value <= 255, "%s: nodata_value %d not in 0..255", fn, nodata_value);
    FU_REQUIRE(class_values || nodata_value >= n_classes,
               "%s: nodata_value %d is a class index (identity class values 0..%d)", fn, nodata_value, n_classes - 1);
    for (int k = 0; class_values && k < n_classes; ++k)
      FU_REQUIRE(class_values[k] != nodata_value, "%s: nodata_value %d is the value of class %d", fn, nodata_value, k);
  }
  return launch_stitch_finalize_maps(canvas, weight, n_classes, (int64_t)canvas_h * canvas_w, eps, normalize_in_place != 0,
                                     class_values, class_out, prob_out, margin_out, counts_out, thr, (hipStream_t)stream,
                                     valid, nodata_value);
}

int fu_scene_valid_mask(const float* raster, int C, int src_h, int src_w, int use_nodata, float nodata, const int32_t* iy,
                        const float* wy, const int32_t* ix, const float* wx, int grid_h, int grid_w, uint8_t* src_valid,
                        uint8_t* valid_out, int64_t* n_valid_out, fu_stream stream) {
  return launch_scene_valid_mask(raster, C, src_h, src_w, use_nodata != 0, nodata, iy, wy, ix, wx, grid_h, grid_w, src_valid,
                                 valid_out, n_valid_out, (hipStream_t)stream);
}

int fu_mask_box_counts(fu_ctx* c, int n, const fu_mask_box* entries, int64_t* counts_out, fu_stream stream) {
  FU_REQUIRE(c && entries && counts_out, "fu_mask_box_counts: null context / entries / counts_out");
  return launch_mask_box_counts(c->scene_table, n, entries, counts_out, (hipStream_t)stream);
}

int fu_tiff_unpack(const uint8_t* src, int64_t n_bytes, fu_tiff_layout layout, const int32_t* bands, int n_bands, float* out,
                   fu_stream stream) {
  return launch_tiff_unpack(src, n_bytes, layout, bands, n_bands, out, (hipStream_t)stream);
}

int fu_tiff_pack(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, fu_tiff_layout layout,
                 uint8_t* dst, int64_t n_bytes, fu_stream stream) {
  return launch_tiff_pack(src, band_stride, row_stride, col_stride, layout, dst, n_bytes, (hipStream_t)stream);
}

int fu_map_overviews(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, int bands, int h, int w,
                     int kind, const uint8_t* valid, int nodata_value, int n_levels, void* dst, int64_t dst_elems,
                     uint8_t* valid_dst, fu_stream stream) {
  return launch_map_overviews(src, band_stride, row_stride, col_stride, bands, h, w, kind, valid, nodata_value, n_levels, dst,
                              dst_elems, valid_dst, (hipStream_t)stream);
}

int fu_eval_prob_hist(fu_ctx* c, const int64_t* target, int ignore_index, int n_bins, int64_t* hist_out, int64_t* top_out,
                      fu_stream stream) {
  FU_REQUIRE(c && target, "fu_eval_prob_hist: null context / target");
  FU_REQUIRE(c->last_batch > 0, "fu_eval_prob_hist: no forward pass yet");
  return launch_prob_hist("fu_eval_prob_hist", c->logits, true, target, (int64_t)c->last_batch * c->cfg.height * c->cfg.width,
                          c->cfg.n_classes, ignore_index, n_bins, hist_out, top_out, (hipStream_t)stream);
}

int fu_prob_hist(const float* probs, const int64_t* target, int64_t n_pixels, int n_classes, int ignore_index, int n_bins,
                 int64_t* hist_out, int64_t* top_out, fu_stream stream) {
  return launch_prob_hist("fu_prob_hist", probs, false, target, n_pixels, n_classes, ignore_index, n_bins, hist_out, top_out,
                          (hipStream_t)stream);
}

// fu_map_components / fu_map_sieve share these checks; every one comes before anything is launched
static int check_map_args(const char* fn, const void* map, const void* out, int h, int w, int connectivity) {
  FU_REQUIRE(map && out, "%s: null map / output", fn);
  FU_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= FU_MAP_MAX_PIXELS, "%s: map %dx%d is empty or has more than 2^28 pixels", fn,
             h, w);
  FU_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  return 0;
}

int64_t fu_sieve_workspace_bytes(int h, int w) {
  if (h < 1 || w < 1 || (int64_t)h * w > FU_MAP_MAX_PIXELS) return 0;
  return sieve_workspace_bytes(h, w);
}

int fu_map_components(const uint8_t* map, int h, int w, int connectivity, int32_t* labels_out, fu_stream stream) {
  FU_TRY(check_map_args("fu_map_components", map, labels_out, h, w, connectivity));
  return launch_map_components(map, h, w, connectivity, labels_out, (hipStream_t)stream);
}

int fu_map_sieve(const uint8_t* map, uint8_t* out, int h, int w, int connectivity, int min_pixels, int frozen_value, int passes,
                 void* workspace, int64_t workspace_bytes, int64_t* stats_out, fu_stream stream) {
  FU_TRY(check_map_args("fu_map_sieve", map, out, h, w, connectivity));
  FU_REQUIRE(frozen_value >= -1 && frozen_value <= 255, "fu_map_sieve: frozen_value %d not in -1..255", frozen_value);
  FU_REQUIRE(passes >= 1 && passes <= 8, "fu_map_sieve: passes %d not in 1..8", passes);
  FU_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sieve_workspace_bytes(h, w),
             "fu_map_sieve: workspace missing, not 16-byte aligned or smaller than fu_sieve_workspace_bytes = %lld",
             (long long)sieve_workspace_bytes(h, w));
  return launch_map_sieve(map, out, h, w, connectivity, min_pixels, frozen_value, passes, workspace, stats_out,
                          (hipStream_t)stream);
}

int64_t fu_map_edges_workspace_bytes(int h, int w) { return map_edges_workspace_bytes(h, w); }

int fu_map_edge_offsets(const uint8_t* map, int h, int w, const uint8_t* select, int32_t* offsets_out, void* workspace,
                        int64_t workspace_bytes, fu_stream stream) {
  return launch_map_edge_offsets(map, h, w, select, offsets_out, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t fu_map_rings_workspace_bytes(int64_t capacity) { return map_rings_workspace_bytes(capacity); }

int fu_map_edge_rings(const uint8_t* map, const int32_t* labels, int h, int w, const uint8_t* select, int connectivity,
                      const int32_t* offsets, int64_t capacity, int32_t* start_out, int32_t* comp_out, int32_t* ring_out,
                      int32_t* rank_out, int32_t* flags_out, void* workspace, int64_t workspace_bytes, fu_stream stream) {
  return launch_map_edge_rings(map, labels, h, w, select, connectivity, offsets, capacity, start_out, comp_out, ring_out,
                               rank_out, flags_out, workspace, workspace_bytes, (hipStream_t)stream);
}

int fu_augment(const float* image, const int64_t* target, float* image_out, int64_t* target_out, const int32_t* flags,
               const float* angles_deg, int B, int C, int H, int W, int64_t target_fill, fu_stream stream) {
  FU_REQUIRE(image && image_out && flags && angles_deg, "fu_augment: null argument");
  FU_REQUIRE((target == nullptr) == (target_out == nullptr), "fu_augment: target and target_out go together");
  FU_REQUIRE(image != image_out && (!target || target != target_out), "fu_augment: in-place operation is not supported");
  return launch_augment(image, target, image_out, target_out, flags, angles_deg, B, C, H, W, target_fill,
                        (hipStream_t)stream);
}

int fu_assemble_tiles(const float* const* srcs, const int32_t* src_channels, int n_src, int B, int H, int W,
                      const int32_t* valid_h, const int32_t* valid_w, int norm_mode, const float* global_mean,
                      const float* global_std, float pad_value, float* out, float* mean_out, float* std_out,
                      fu_stream stream) {
  FU_REQUIRE(srcs && src_channels && out && B >= 1 && H >= 1 && W >= 1, "fu_assemble_tiles: bad argument");
  return launch_assemble_tiles(srcs, src_channels, n_src, B, H, W, valid_h, valid_w, norm_mode, global_mean, global_std,
                               pad_value, out, mean_out, std_out, (hipStream_t)stream);
}

int fu_scene_crops(fu_ctx* c, int n, const fu_scene_crop* entries, int C, int tile_h, int tile_w, int norm_mode,
                   const float* global_mean, const float* global_std, float pad_value, float* out, float* mean_out,
                   float* std_out, fu_stream stream) {
  FU_REQUIRE(c && entries && out, "fu_scene_crops: null context / entries / out");
  return launch_scene_crops(c->scene_table, n, entries, C, tile_h, tile_w, norm_mode, global_mean, global_std, pad_value, out,
                            mean_out, std_out, (hipStream_t)stream);
}

int fu_scene_train_tiles(fu_ctx* c, int n, const fu_scene_train_entry* entries, int C, int tile_h, int tile_w, int norm_mode,
                         const float* global_mean, const float* global_std, float pad_value, int64_t nodata_value,
                         int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out, float* std_out,
                         fu_stream stream) {
  FU_REQUIRE(c && entries && image_out, "fu_scene_train_tiles: null context / entries / image_out");
  return launch_scene_train_tiles(c->train_table, n, entries, C, tile_h, tile_w, norm_mode, global_mean, global_std,
                                  pad_value, nodata_value, target_fill, image_out, target_out, mean_out, std_out, nullptr,
                                  (hipStream_t)stream);
}

int fu_scene_train_tiles_ex(fu_ctx* c, int n, const fu_scene_train_entry* entries, int C, int tile_h, int tile_w,
                            int norm_mode, const float* global_mean, const float* global_std, float pad_value,
                            int64_t nodata_value, int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out,
                            float* std_out, const fu_scene_aug* aug, fu_stream stream) {
  FU_REQUIRE(c && entries && image_out, "fu_scene_train_tiles_ex: null context / entries / image_out");
  return launch_scene_train_tiles(c->train_table, n, entries, C, tile_h, tile_w, norm_mode, global_mean, global_std,
                                  pad_value, nodata_value, target_fill, image_out, target_out, mean_out, std_out, aug,
                                  (hipStream_t)stream);
}

int fu_label_class_counts(fu_ctx* c, int n, const fu_scene_train_entry* entries, int64_t nodata_value, int n_classes,
                          int64_t* counts_out, fu_stream stream) {
  FU_REQUIRE(c && entries && counts_out, "fu_label_class_counts: null context / entries / counts_out");
  return launch_label_class_counts(c->train_table, n, entries, nodata_value, n_classes, counts_out, (hipStream_t)stream);
}

int fu_label_box_counts(fu_ctx* c, int n, const fu_scene_train_entry* entries, int64_t* counts_out, fu_stream stream) {
  FU_REQUIRE(c && entries && counts_out, "fu_label_box_counts: null context / entries / counts_out");
  return launch_label_box_counts(c->train_table, n, entries, counts_out, (hipStream_t)stream);
}

int64_t fu_band_stats_workspace_bytes(int n_channels, int n_bins) {
  if (n_channels < 1 || n_bins < 0) return 0;
  return band_stats_workspace_bytes(n_channels, n_bins);
}

int fu_band_stats(const float* const* srcs, const int32_t* src_channels, int n_src, int B, int H, int W,
                  const int32_t* valid_h, const int32_t* valid_w, int mask_mode, const fu_band_accum* acc,
                  void* workspace, int64_t workspace_bytes, fu_stream stream) {
  FU_REQUIRE(srcs && src_channels && acc, "fu_band_stats: null sources / channel list / accumulators");
  const BandAccum a{acc->count, acc->sum, acc->sumsq, acc->vmin, acc->vmax, acc->n_nonfinite, acc->hist, acc->n_bins,
                    acc->lo, acc->hi};
  return launch_band_stats(srcs, src_channels, n_src, B, H, W, valid_h, valid_w, mask_mode, a, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

int fu_resize_lanczos4_tiles(const float* windows, int B, int C, int win_h, int win_w, const int32_t* iy, const float* wy,
                             const int32_t* ix, const float* wx, int tile_h, int tile_w, int scale_mode, float* out,
                             fu_stream stream) {
  FU_REQUIRE(windows && iy && wy && ix && wx && out && B >= 1 && C >= 1, "fu_resize_lanczos4_tiles: bad argument");
  return launch_resize_lanczos4_tiles(windows, B, C, win_h, win_w, iy, wy, ix, wx, tile_h, tile_w, scale_mode, out,
                                      (hipStream_t)stream);
}

}  // extern "C"
