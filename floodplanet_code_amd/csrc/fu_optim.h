// The optimiser's host-side declarations: the launchers of fu_optim.hip and the small structs they take.  Included by
// fu_optim.hip, by fu_ctx.h (the context keeps a GradClip inside its OptimState) and by fu_optim_api.hip, the entry points.
#pragma once
#include "fu_common.h"

namespace fu {

// fp16 guard: guard[0] <- 1 if a gradient is not finite; bookkeeping after the (possibly skipped) Adam launch
int launch_grad_finite_check(const float* g, int64_t n, int* guard, hipStream_t s);
int launch_guard_book(int* guard, hipStream_t s);

void adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, float out[7]);
// the weight EMA of launch_adam: the averages of the parameters and of the BatchNorm running statistics (nbn channels)
struct AdamEma {
  float* p;
  float* rm_ema; const float* rm;
  float* rv_ema; const float* rv;
  int64_t nbn;
};
// Decoupled weight decay (AdamW) of launch_adam: which elements of the flat buffer decay, as the sorted bounds of the merged
// ranges of the decayed tensors -- element i decays when an odd number of bounds is <= i (bounds[2r] = first element of range
// r, bounds[2r + 1] = one past its last).  nb = 2 x ranges, at most 2 * WD_MAX_RANGES; device memory owned by the context.
constexpr int WD_MAX_RANGES = 512;       // a parameter table of CLIP_MAX_PARAMS tensors cannot form more
struct AdamDecay {
  const int64_t* bounds;
  int nb;
};
// the merged ranges of the flagged tensors of a parameter table (offsets ascending), host side: bounds as above
void plan_decay_bounds(const int64_t* off, const int64_t* numel, const uint8_t* flag, int nparams, std::vector<int64_t>* bounds);
// Adam in one launch; ema != null: the weight EMA (parameters, then the running statistics) in the same launch.
// sc = the host scalars (adam_scalars' seven; with ema the EMA weight as the eighth), or scalars_dev != null = the same
// floats read on the device (the captured form).  wd != null: the k_adamw* kernels -- the flagged elements are multiplied by
// the ninth scalar, the step's decay factor (step_scalars, fu_optim_api.hip), ahead of the same update (sc / scalars_dev then
// hold nine floats)
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, const AdamEma* ema, const float* sc,
                const float* scalars_dev, hipStream_t s, const int* skip = nullptr, const AdamDecay* wd = nullptr);

// Global-norm gradient clipping ahead of the Adam launch (fu_set_grad_clip) and the gradient-norm report (fu_grad_norms).
// The flat gradient buffer is cut into chunks of at most CLIP_CHUNK floats, none across two parameter tensors; one launch
// writes every chunk's sum of squares (double), a one-workgroup launch sums them per tensor and in total, in a fixed order.
constexpr int CLIP_CHUNK = 16384;
struct ClipChunk { int64_t off; int32_t len; int32_t param; };
// what the finalize launch leaves behind (fu_grad_clip_state); skip is WRITTEN every step: 1 = the norm was not finite
struct ClipState { float last_norm, last_coef; int32_t skip, pad_; int64_t steps, clipped, nonfinite; };
struct GradClip {            // device memory owned by the context, made once (build_grad_clip)
  ClipChunk* chunks = nullptr;
  int* first = nullptr;      // [nparams + 1]: tensor t owns the chunks first[t] .. first[t + 1] - 1
  double* part = nullptr;    // [nchunks] sums of squares
  ClipState* state = nullptr;
  float* scalars = nullptr;  // the nine Adam scalars with the clip coefficient folded into slot 6
  int nchunks = 0, nparams = 0;
};
// the chunk table of a parameter table (offsets and sizes in floats), host side; first gets nparams + 1 entries
void plan_clip_chunks(const int64_t* off, const int64_t* numel, int nparams, std::vector<ClipChunk>* chunks,
                      std::vector<int>* first);
int build_grad_clip(GradClip* w, const int64_t* off, const int64_t* numel, int nparams, std::vector<void*>* allocs);
int launch_grad_sqnorm(const GradClip& w, const float* g, hipStream_t s);
// the Adam scalars as the caller formed them: sc (nine host floats, the first n of them meant) or sc_dev (n device floats);
// n = 7, 8 with the EMA weight, 9 with the decay factor.  The clipped set goes to w.scalars, the report to w.state
int launch_grad_clip_finalize(const GradClip& w, const float* sc, const float* sc_dev, int n, double max_norm, hipStream_t s);
// norms_out[0 .. nparams - 1] = every tensor's L2 norm times |grad_scale|, norms_out[nparams] = the total; nothing else is written
int launch_grad_norms_out(const GradClip& w, double grad_scale, float* norms_out, hipStream_t s);

}  // namespace fu
