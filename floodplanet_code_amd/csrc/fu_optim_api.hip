// libfloodunet: the optimiser's part of the C ABI (include/floodunet.h) -- binding the moments and the weight EMA, the
// fused Adam step in its four forms, its scalars, gradient clipping, decoupled weight decay, the gradient-norm report and
// the fp16 guard's state.  Every entry point checks its arguments here and calls a launcher of fu_optim.hip; what it keeps
// between calls is the context's OptimState (fu_ctx.h).  Host code only.
#include "fu_ctx.h"
#include "fu_optim.h"

#include <algorithm>
#include <math.h>

using namespace fu;

namespace {

// The nine float scalars of one optimiser step, the one place they are formed: adam_scalars' seven, the EMA weight, and
// the decay factor (float)(1 - lr * weight_decay), formed in double and rounded once (exactly 1 for weight_decay 0).  The
// three public *_scalars functions and the two host-scalar steps go through it; a mode reads only the slots it uses.
void step_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, double ema_weight,
                  double weight_decay, float out[9]) {
  adam_scalars(lr, beta1, beta2, eps, step, grad_scale, out);
  out[7] = (float)ema_weight;
  out[8] = (float)(1.0 - lr * weight_decay);
}
// fu_adam_ema_scalars' checks; fu_adam_ema_step and fu_adamw_scalars make them too, under its name
int check_ema_scalars(const float* out, int64_t step, double ema_weight) {
  FU_REQUIRE(out && step >= 1, "fu_adam_ema_scalars: bad argument");
  FU_REQUIRE(ema_weight >= 0.0 && ema_weight <= 1.0, "fu_adam_ema_scalars: ema_weight %g outside [0, 1]", ema_weight);
  return 0;
}

// The one optimiser step behind fu_adam_step[_dev] and fu_adam_ema_step[_dev] (ema: the averages go in the same launch):
// moments bound?, fp16 guard, launch, guard book.  sc: nine host scalars (step_scalars), or scalars_dev: the same floats on
// the device; how many of them the step means -- 7, 8 with ema, 9 with decay armed -- is decided here, once.
inline bool decay_armed(const OptimState& o) { return o.weight_decay > 0.0 && o.wd_nb > 0; }
int adam_step(fu_ctx* c, const char* who, bool ema, const float* sc, const float* scalars_dev, fu_stream stream) {
  OptimState& o = c->opt;
  if (!o.adam_m || !o.adam_v) {
    set_error("%s: no moment buffers bound (fu_bind_adam_state)", who);
    return FU_ERR_STATE;
  }
  if (ema && !o.ema_p) {
    set_error("%s: no EMA buffers bound (fu_bind_ema_state)", who);
    return FU_ERR_STATE;
  }
  // fp16: an overflowed gradient map leaves inf / NaN in the gradient buffer -- such a step is skipped and the loss scale
  // backs off (the guard kernels in fu_optim.hip); 13 us of the 69 MB gradient read per step, fp16 mode only
  const int* skip = nullptr;
  if (c->prec == PREC_F16) {
    FU_TRY(launch_grad_finite_check(c->G, c->total_params, c->guard, (hipStream_t)stream));
    skip = c->guard;
  }
  // clipping armed (fu_set_grad_clip): the norm pass and its one-workgroup finalize go first and leave the scalars, with the
  // coefficient folded into the gradient scale, in the context's own nine floats; the Adam launch is the _dev form on those,
  // whichever entry point was called.  A non-finite norm skips the step (fp16: the guard's flag, set together with it)
  // decay armed (fu_set_weight_decay) on at least one tensor: the scalars are nine floats and the launch is the k_adamw*
  // twin, which also gets the bounds of the decayed ranges; otherwise exactly the launch there has always been
  const bool wd = decay_armed(o);
  const int n_scalars = wd ? 9 : ema ? 8 : 7;
  if (o.clip_max_norm > 0.0) {
    FU_TRY(launch_grad_sqnorm(o.clip, c->G, (hipStream_t)stream));
    FU_TRY(launch_grad_clip_finalize(o.clip, sc, scalars_dev, n_scalars, o.clip_max_norm, (hipStream_t)stream));
    sc = nullptr;
    scalars_dev = o.clip.scalars;
    if (!skip) skip = &o.clip.state->skip;
  }
  const AdamEma avg = {o.ema_p, o.ema_rm, c->RM, o.ema_rv, c->RV, c->total_bn};
  const AdamDecay dec = {o.wd_bounds, o.wd_nb};
  FU_TRY(launch_adam(c->P, c->G, o.adam_m, o.adam_v, c->total_params, ema ? &avg : nullptr, sc, scalars_dev,
                     (hipStream_t)stream, skip, wd ? &dec : nullptr));
  if (c->prec == PREC_F16) FU_TRY(launch_guard_book(c->guard, (hipStream_t)stream));
  c->packed_dirty = true;
  return FU_OK;
}

// the chunk table, partials, state block and scalars of the gradient norm: made once per context, at the first use
int ensure_grad_clip(fu_ctx* c) {
  if (c->opt.clip.chunks) return FU_OK;
  std::vector<int64_t> off, numel;
  for (const ParamInfo& p : c->params) { off.push_back(p.off); numel.push_back(p.numel); }
  FU_HIP_CHECK(hipSetDevice(c->cfg.device));
  return build_grad_clip(&c->opt.clip, off.data(), numel.data(), (int)c->params.size(), &c->extra_allocs);
}

}  // namespace

extern "C" {

int fu_bind_adam_state(fu_ctx* c, float* exp_avg, float* exp_avg_sq) {
  FU_REQUIRE(c && exp_avg && exp_avg_sq, "fu_bind_adam_state: null argument");
  c->opt.adam_m = exp_avg; c->opt.adam_v = exp_avg_sq;
  return FU_OK;
}
int fu_bind_ema_state(fu_ctx* c, float* ema_params, float* ema_running_mean, float* ema_running_var) {
  FU_REQUIRE(c, "null context");
  const int given = (ema_params != nullptr) + (ema_running_mean != nullptr) + (ema_running_var != nullptr);
  FU_REQUIRE(given == 0 || given == 3, "fu_bind_ema_state: give all three buffers, or all NULL to unbind");
  c->opt.ema_p = ema_params; c->opt.ema_rm = ema_running_mean; c->opt.ema_rv = ema_running_var;
  return FU_OK;
}

int fu_adam_step(fu_ctx* c, double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                 fu_stream stream) {
  FU_REQUIRE(c && c->P && c->G, "fu_adam_step: parameter / gradient buffers not bound");
  FU_REQUIRE(step >= 1, "fu_adam_step: step is 1-based");
  float sc[9];
  step_scalars(lr, beta1, beta2, eps, step, grad_scale, 0.0, c->opt.weight_decay, sc);
  return adam_step(c, "fu_adam_step", false, sc, nullptr, stream);
}

int fu_fp16_guard_state(fu_ctx* c, int64_t* skipped_steps, int32_t* backoff_exponent) {
  FU_REQUIRE(c, "null context");
  int h[4] = {0, 0, 0, 0};
  if (c->prec == PREC_F16) FU_HIP_CHECK(hipMemcpy(h, c->guard, sizeof(h), hipMemcpyDeviceToHost));   // synchronises
  if (skipped_steps) *skipped_steps = h[1];
  if (backoff_exponent) *backoff_exponent = h[2];
  return FU_OK;
}

int fu_adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, float out[7]) {
  FU_REQUIRE(out && step >= 1, "fu_adam_scalars: bad argument");
  float sc[9];
  step_scalars(lr, beta1, beta2, eps, step, grad_scale, 0.0, 0.0, sc);
  std::copy(sc, sc + 7, out);
  return FU_OK;
}

int fu_adam_step_dev(fu_ctx* c, const float* scalars_dev, fu_stream stream) {
  FU_REQUIRE(c && c->P && c->G && scalars_dev, "fu_adam_step_dev: parameter / gradient buffers not bound, or null scalars");
  return adam_step(c, "fu_adam_step_dev", false, nullptr, scalars_dev, stream);
}

int fu_adam_ema_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                        double ema_weight, float out[8]) {
  FU_TRY(check_ema_scalars(out, step, ema_weight));
  float sc[9];
  step_scalars(lr, beta1, beta2, eps, step, grad_scale, ema_weight, 0.0, sc);
  std::copy(sc, sc + 8, out);
  return FU_OK;
}

int fu_adam_ema_step(fu_ctx* c, double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale,
                     double ema_weight, fu_stream stream) {
  FU_REQUIRE(c && c->P && c->G && c->RM && c->RV, "fu_adam_ema_step: buffers not bound (fu_bind_buffers)");
  float sc[9];
  FU_TRY(check_ema_scalars(sc, step, ema_weight));
  step_scalars(lr, beta1, beta2, eps, step, grad_scale, ema_weight, c->opt.weight_decay, sc);
  return adam_step(c, "fu_adam_ema_step", true, sc, nullptr, stream);
}

int fu_adam_ema_step_dev(fu_ctx* c, const float* scalars_dev, fu_stream stream) {
  FU_REQUIRE(c && c->P && c->G && c->RM && c->RV && scalars_dev,
             "fu_adam_ema_step_dev: buffers not bound (fu_bind_buffers), or null scalars");
  return adam_step(c, "fu_adam_ema_step_dev", true, nullptr, scalars_dev, stream);
}

int fu_set_grad_clip(fu_ctx* c, double max_norm) {
  FU_REQUIRE(c, "null context");
  FU_REQUIRE(isfinite(max_norm) && max_norm >= 0.0, "fu_set_grad_clip: max_norm %g must be finite and >= 0 (0 disarms)", max_norm);
  if (max_norm > 0.0) FU_TRY(ensure_grad_clip(c));
  c->opt.clip_max_norm = max_norm;
  return FU_OK;
}

int fu_grad_clip_state(fu_ctx* c, float* last_norm, float* last_coef, int64_t* steps, int64_t* clipped_steps,
                       int64_t* nonfinite_steps) {
  FU_REQUIRE(c, "null context");
  ClipState h = {};
  if (c->opt.clip.state) {
    FU_HIP_CHECK(hipSetDevice(c->cfg.device));
    FU_HIP_CHECK(hipDeviceSynchronize());                  // every stream: the step may run on a non-blocking one
    FU_HIP_CHECK(hipMemcpy(&h, c->opt.clip.state, sizeof(h), hipMemcpyDeviceToHost));
  }
  if (last_norm) *last_norm = h.last_norm;
  if (last_coef) *last_coef = h.last_coef;
  if (steps) *steps = h.steps;
  if (clipped_steps) *clipped_steps = h.clipped;
  if (nonfinite_steps) *nonfinite_steps = h.nonfinite;
  return FU_OK;
}

int fu_adamw_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, double ema_weight,
                     double weight_decay, float out[9]) {
  FU_REQUIRE(out && step >= 1, "fu_adamw_scalars: bad argument");
  FU_REQUIRE(isfinite(weight_decay) && weight_decay >= 0.0, "fu_adamw_scalars: weight_decay %g must be finite and >= 0",
             weight_decay);
  FU_TRY(check_ema_scalars(out, step, ema_weight));
  step_scalars(lr, beta1, beta2, eps, step, grad_scale, ema_weight, weight_decay, out);
  return FU_OK;
}

int fu_set_weight_decay(fu_ctx* c, double weight_decay, const uint8_t* decay_mask, int n_mask) {
  FU_REQUIRE(c, "null context");
  FU_REQUIRE(isfinite(weight_decay) && weight_decay >= 0.0,
             "fu_set_weight_decay: weight_decay %g must be finite and >= 0 (0 disarms)", weight_decay);
  OptimState& o = c->opt;
  const int np = (int)c->params.size();
  FU_REQUIRE(!decay_mask || n_mask == np, "fu_set_weight_decay: a mask of %d flags for %d parameter tensors", n_mask, np);
  if (weight_decay == 0.0) {
    o.weight_decay = 0.0;
    o.wd_nb = 0;
    o.wd_mask.assign(np, 0);
    return FU_OK;
  }
  // default rule: every tensor with two or more dimensions (conv, transposed-conv, fusion and head weights); biases and
  // BatchNorm weight / bias do not decay
  std::vector<uint8_t> mask(np);
  std::vector<int64_t> off(np), numel(np), bounds;
  for (int t = 0; t < np; ++t) {
    const ParamInfo& p = c->params[t];
    mask[t] = decay_mask ? (decay_mask[t] != 0) : (p.ndim >= 2);
    off[t] = p.off;
    numel[t] = p.numel;
  }
  plan_decay_bounds(off.data(), numel.data(), mask.data(), np, &bounds);
  FU_REQUIRE(bounds.size() <= (size_t)2 * WD_MAX_RANGES, "fu_set_weight_decay: the mask forms %d ranges of the flat buffer, at most %d supported",
             (int)(bounds.size() / 2), WD_MAX_RANGES);
  if (!bounds.empty()) {
    FU_HIP_CHECK(hipSetDevice(c->cfg.device));
    if (!o.wd_bounds) {                  // one table of the full size per context: a later mask is copied over it
      FU_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&o.wd_bounds), (size_t)2 * WD_MAX_RANGES * sizeof(int64_t)));
      c->extra_allocs.push_back(o.wd_bounds);
    }
    FU_HIP_CHECK(hipDeviceSynchronize());                    // no step in flight reads the table while it changes
    FU_HIP_CHECK(hipMemcpy(o.wd_bounds, bounds.data(), bounds.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  o.weight_decay = weight_decay;
  o.wd_nb = (int)bounds.size();
  o.wd_mask = mask;
  return FU_OK;
}

int fu_weight_decay_state(const fu_ctx* c, double* weight_decay, uint8_t* mask_out, int n_mask) {
  FU_REQUIRE(c, "null context");
  const OptimState& o = c->opt;
  const int np = (int)c->params.size();
  FU_REQUIRE(!mask_out || n_mask == np, "fu_weight_decay_state: room for %d flags, %d parameter tensors", n_mask, np);
  if (weight_decay) *weight_decay = o.weight_decay;
  if (mask_out)
    for (int t = 0; t < np; ++t) mask_out[t] = (o.weight_decay > 0.0 && t < (int)o.wd_mask.size()) ? o.wd_mask[t] : 0;
  return FU_OK;
}

int fu_grad_norms(fu_ctx* c, double grad_scale, float* norms_out_dev, fu_stream stream) {
  FU_REQUIRE(c && c->G && norms_out_dev, "fu_grad_norms: no gradient buffer bound, or null output");
  FU_TRY(ensure_grad_clip(c));
  FU_TRY(launch_grad_sqnorm(c->opt.clip, c->G, (hipStream_t)stream));
  return launch_grad_norms_out(c->opt.clip, grad_scale, norms_out_dev, (hipStream_t)stream);
}

int fu_adam_state(fu_ctx* c, float** exp_avg, float** exp_avg_sq) {
  FU_REQUIRE(c, "null context");
  if (exp_avg) *exp_avg = c->opt.adam_m;
  if (exp_avg_sq) *exp_avg_sq = c->opt.adam_v;
  return FU_OK;
}

int fu_zero_grads(fu_ctx* c, fu_stream stream) {
  FU_REQUIRE(c && c->G, "fu_zero_grads: no gradient buffer bound");
  FU_HIP_CHECK(hipMemsetAsync(c->G, 0, c->total_params * sizeof(float), (hipStream_t)stream));
  return FU_OK;
}

}  // extern "C"
