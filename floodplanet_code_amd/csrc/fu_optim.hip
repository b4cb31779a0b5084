// Optimiser kernels (gfx950): Adam in torch's single-tensor order, optionally with the weight EMA and with AdamW's decoupled
// weight decay in the same pass, and the fp16 guard around it (non-finite gradient check, skipped-step book-keeping); the
// global gradient norm and the clip coefficient ahead of it (two launches of their own: the Adam kernels only ever see
// another gscale).
#include "fu_optim.h"

#include <algorithm>
#include <math.h>

namespace fu {

// ------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam single-tensor update order; water_seg_model.py:200), optionally with the weight EMA in the same
// pass: ema = lerp(ema, p_new, w) on the value just written -- 9 streams of n floats where the plain step moves 7, in
// 16-byte accesses.  The lerp is torch's CPU Tensor.lerp_(end, w) on float32, which in ATen is ONE fused multiply-add in
// either branch (LerpKernel.cpp, vector and scalar loop alike):
//   w <  0.5:  fma(w,     end - self, self)
//   w >= 0.5:  fma(w - 1, end - self, end)         (w - 1 rounded to float first)
// The branch is taken from the float w, on the device in the captured form (w crosses 0.5 during the warm-up).  The EMA
// launch also averages the BatchNorm running statistics (nbn channels, two arrays) after the parameters.
// skip (optional, fp16 mode): device flag set by k_grad_finite_check when a gradient of this step is not finite -- the whole
// update is then left out (parameters, moments and averages untouched), as a GradScaler skips such a step
// ------------------------------------------------------------------------------------------------
// Decoupled weight decay (WD, torch.optim.AdamW's single-tensor path): a decayed element is first multiplied by
// decay = (float)(1 - lr * weight_decay) -- param.mul_(1 - lr * weight_decay), one fp32 multiply with its own rounding -- and
// the sequence above then runs on that value; the moments only ever see the gradient.  Which elements decay is a property
// of their tensor: the kernel gets the sorted bounds of the merged ranges of the decayed tensors (AdamDecay, a few dozen
// int64), stages them in LDS and looks each 16-byte group up there -- no further stream of memory.
// ------------------------------------------------------------------------------------------------
struct AdamScalars { float w1, beta2, omb2, bc2_sqrt, eps, neg_step, gscale, ema_w, decay; };

// The update of one element; the ONLY place the sequence is written.  Every operation rounds on its own, in ATen's order
// (no fma contraction): with identical inputs the update is the same float sequence as torch's CPU Adam[W]
// ([mul_ /] lerp_ / mul_ / addcmul_ / sqrt / div / add_ / addcdiv_).  WD == false: dec and s.decay are not looked at.
template <bool WD>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s, bool dec) {
#pragma clang fp contract(off)
  if constexpr (WD) {
    if (dec) p = p * s.decay;               // param.mul_(1 - lr * weight_decay): the only place the decay is written
  }
  const float gi = g * s.gscale;
  float mi = m, vi = v;
  const float dm = gi - mi;
  mi = fmaf(s.w1, dm, mi);                  // exp_avg.lerp_(grad, 1-beta1): the weight < 0.5 branch of ATen's vectorised lerp, fmadd(weight, end - self, self)
  const float vb = vi * s.beta2;
  const float og = s.omb2 * gi;
  vi = vb + og * gi;                        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
  const float denom = sqrtf(vi) / s.bc2_sqrt + s.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  const float num = s.neg_step * mi;
  p = p + num / denom;                      // param.addcdiv_(exp_avg, denom, value=-step_size): self + value * t1 / t2
  m = mi;
  v = vi;
}
__device__ __forceinline__ float ema_lerp(float self, float end, float wl, bool small) {
  const float d = end - self;
  return fmaf(wl, d, small ? self : end);
}
// The number of bounds <= i in the sorted bounds bnd[0 .. nb - 1] (LDS): odd = element i lies in a decayed range.  A fixed
// trip count for every lane (it depends on nb alone), one LDS read per halving.
__device__ __forceinline__ int decay_rank(const int64_t* bnd, int nb, int64_t i) {
  int base = 0;
  for (int len = nb; len > 1;) {
    const int half = len >> 1;
    if (bnd[base + half - 1] <= i) base += half;
    len -= half;
  }
  return base + ((nb > 0 && bnd[base] <= i) ? 1 : 0);
}
// The decay flags of the four elements i .. i + 3, bit k = element i + k.  One search; a group that no bound cuts -- all but
// a few dozen of the buffer's -- takes its first element's flag, one that straddles a tensor boundary decides per element.
__device__ __forceinline__ unsigned decay_flags4(const int64_t* bnd, int nb, int64_t i) {
  int k = decay_rank(bnd, nb, i);
  if (k == nb || bnd[k] >= i + 4) return (k & 1) ? 0xFu : 0u;
  unsigned flags = k & 1;
  for (int el = 1; el < 4; ++el) {
    while (k < nb && bnd[k] <= i + el) ++k;
    flags |= (unsigned)(k & 1) << el;
  }
  return flags;
}
// head: the elements in front of the first 16-byte boundary (n when the arrays are not aligned alike: all scalar).
// EMA == false: e, the running statistics and s.ema_w are not touched.  WD == false: bnd, wd_nb and s.decay are not
// looked at; WD: bnd is the workgroup's LDS room for the wd_nb bounds at wd_bounds.  The copy into it is made HERE, behind the
// first group's 16-byte loads: the table's load then travels with them, where a copy ahead of them left every workgroup of the
// first wave idle for one more memory round trip.  Every thread reaches the barrier, with or without a group of its own.
template <bool EMA, bool WD>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, float* __restrict__ e, int64_t n, int64_t head,
                                          const AdamScalars& s, float* __restrict__ erm, const float* __restrict__ rm,
                                          float* __restrict__ erv, const float* __restrict__ rv, int64_t nbn,
                                          const int64_t* __restrict__ wd_bounds, int64_t* bnd, int wd_nb) {
#pragma clang fp contract(off)
  const bool small = EMA && fabsf(s.ema_w) < 0.5f;
  const float wl = !EMA ? 0.f : small ? s.ema_w : s.ema_w - 1.0f;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = (n - head) / 4;
  float4 p4, g4, m4, v4, e4;
  auto load4 = [&](int64_t i) {
    p4 = *reinterpret_cast<const float4*>(p + i);
    g4 = *reinterpret_cast<const float4*>(g + i);
    m4 = *reinterpret_cast<const float4*>(m + i);
    v4 = *reinterpret_cast<const float4*>(v + i);
    if constexpr (EMA) e4 = *reinterpret_cast<const float4*>(e + i);
  };
  if constexpr (WD) {
    if (tid < nvec) load4(head + 4 * tid);
    for (int k = threadIdx.x; k < wd_nb; k += blockDim.x) bnd[k] = wd_bounds[k];
    __syncthreads();
  }
  for (int64_t j = tid; j < nvec; j += nthr) {
    const int64_t i = head + 4 * j;
    if (!WD || j != tid) load4(i);
    unsigned dec = 0;
    if constexpr (WD) dec = decay_flags4(bnd, wd_nb, i);       // LDS reads and compares behind the loads above
    adam_elem<WD>(p4.x, g4.x, m4.x, v4.x, s, dec & 1u);
    adam_elem<WD>(p4.y, g4.y, m4.y, v4.y, s, dec & 2u);
    adam_elem<WD>(p4.z, g4.z, m4.z, v4.z, s, dec & 4u);
    adam_elem<WD>(p4.w, g4.w, m4.w, v4.w, s, dec & 8u);
    *reinterpret_cast<float4*>(p + i) = p4;
    *reinterpret_cast<float4*>(m + i) = m4;
    *reinterpret_cast<float4*>(v + i) = v4;
    if constexpr (EMA) {
      e4.x = ema_lerp(e4.x, p4.x, wl, small);
      e4.y = ema_lerp(e4.y, p4.y, wl, small);
      e4.z = ema_lerp(e4.z, p4.z, wl, small);
      e4.w = ema_lerp(e4.w, p4.w, wl, small);
      *reinterpret_cast<float4*>(e + i) = e4;
    }
  }
  const int64_t tail0 = head + 4 * nvec, nrest = head + (n - tail0);      // misaligned head and tail: plain code
  for (int64_t k = tid; k < nrest; k += nthr) {
    const int64_t i = k < head ? k : tail0 + (k - head);
    bool dec = false;
    if constexpr (WD) dec = decay_rank(bnd, wd_nb, i) & 1;
    adam_elem<WD>(p[i], g[i], m[i], v[i], s, dec);
    if constexpr (EMA) e[i] = ema_lerp(e[i], p[i], wl, small);
  }
  if constexpr (EMA) {
    for (int64_t i = tid; i < nbn; i += nthr) {
      erm[i] = ema_lerp(erm[i], rm[i], wl, small);
      erv[i] = ema_lerp(erv[i], rv[i], wl, small);
    }
  }
}
// The scalars by value, or (fu_adam_scalars: seven; fu_adam_ema_scalars: the EMA weight as the eighth) read from DEVICE
// memory: a captured (hipGraph) step replays that launch unchanged while the step count -- and with it the bias
// corrections -- moves on; the caller refreshes the floats before each replay.
// With decay (fu_adamw_scalars) the device form reads nine: slot 7 stays the EMA weight (ignored by the plain form), slot 8
// is the decay factor.  Without it slot 8 is never read: the caller's buffer is 7 or 8 floats long.
template <bool EMA, bool WD>
__device__ __forceinline__ AdamScalars adam_scalars_of(const AdamScalars& s) { return s; }
template <bool EMA, bool WD>
__device__ __forceinline__ AdamScalars adam_scalars_of(const float* __restrict__ sc) {
  return {sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], EMA ? sc[7] : 0.f, WD ? sc[8] : 1.f};
}
// four entry kernels over the one body (their names are what a captured graph's dump and a kernel trace show)
#define FU_ADAM_KERNEL(NAME, EMA, SCALARS)                                                                              \
  __global__ __launch_bounds__(256) void NAME(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, \
                                              float* __restrict__ v, float* __restrict__ e, int64_t n, int64_t head,    \
                                              SCALARS sc, float* __restrict__ erm, const float* __restrict__ rm,        \
                                              float* __restrict__ erv, const float* __restrict__ rv, int64_t nbn,       \
                                              const int* __restrict__ skip) {                                           \
    if (skip && *skip) return;                                                                                          \
    adam_body<EMA, false>(p, g, m, v, e, n, head, adam_scalars_of<EMA, false>(sc), erm, rm, erv, rv, nbn, nullptr,      \
                          nullptr, 0);                                                                                  \
  }
FU_ADAM_KERNEL(k_adam, false, AdamScalars)
FU_ADAM_KERNEL(k_adam_ema, true, AdamScalars)
FU_ADAM_KERNEL(k_adam_dev, false, const float* __restrict__)
FU_ADAM_KERNEL(k_adam_ema_dev, true, const float* __restrict__)
#undef FU_ADAM_KERNEL
// and their four decay-aware twins: the same launch over the whole flat buffer, the bounds (wd_nb <= 2 * WD_MAX_RANGES of
// them, 8 KB at the most) copied into LDS by adam_body.  A skipped step returns before anything: it skips the decay too.
#define FU_ADAMW_KERNEL(NAME, EMA, SCALARS)                                                                             \
  __global__ __launch_bounds__(256) void NAME(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, \
                                              float* __restrict__ v, float* __restrict__ e, int64_t n, int64_t head,    \
                                              SCALARS sc, float* __restrict__ erm, const float* __restrict__ rm,        \
                                              float* __restrict__ erv, const float* __restrict__ rv, int64_t nbn,       \
                                              const int* __restrict__ skip, const int64_t* __restrict__ wd_bounds,      \
                                              int wd_nb) {                                                              \
    __shared__ int64_t bnd[2 * WD_MAX_RANGES];                                                                          \
    if (skip && *skip) return;                                                                                          \
    adam_body<EMA, true>(p, g, m, v, e, n, head, adam_scalars_of<EMA, true>(sc), erm, rm, erv, rv, nbn, wd_bounds, bnd, \
                         min(wd_nb, 2 * WD_MAX_RANGES));                                                                \
  }
FU_ADAMW_KERNEL(k_adamw, false, AdamScalars)
FU_ADAMW_KERNEL(k_adamw_ema, true, AdamScalars)
FU_ADAMW_KERNEL(k_adamw_dev, false, const float* __restrict__)
FU_ADAMW_KERNEL(k_adamw_ema_dev, true, const float* __restrict__)
#undef FU_ADAMW_KERNEL

// the seven float scalars of the update: formed in double as torch.optim.Adam forms them in Python, then rounded once to
// float (the cast ATen applies to a Python scalar operand of a float tensor op)
void adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step, double grad_scale, float out[7]) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const double step_size = lr / bc1;
  const double bc2_sqrt = sqrt(bc2);
  out[0] = (float)(1.0 - beta1); out[1] = (float)beta2; out[2] = (float)(1.0 - beta2); out[3] = (float)bc2_sqrt;
  out[4] = (float)eps; out[5] = (float)(-step_size); out[6] = (float)grad_scale;
}

static int64_t adam_head(const float* p, const float* g, const float* m, const float* v, const float* e, int64_t n) {
  const uintptr_t a = (uintptr_t)p & 15;
  if (((uintptr_t)g & 15) != a || ((uintptr_t)m & 15) != a || ((uintptr_t)v & 15) != a || (e && ((uintptr_t)e & 15) != a) ||
      (a & 3))
    return n;
  const int64_t head = (int64_t)(((16 - a) & 15) / 4);
  return head < n ? head : n;
}
void plan_decay_bounds(const int64_t* off, const int64_t* numel, const uint8_t* flag, int nparams, std::vector<int64_t>* bounds) {
  bounds->clear();
  for (int t = 0; t < nparams; ++t) {
    if (!flag[t] || numel[t] <= 0) continue;
    if (!bounds->empty() && bounds->back() == off[t]) bounds->back() = off[t] + numel[t];   // adjacent tensors: one range
    else { bounds->push_back(off[t]); bounds->push_back(off[t] + numel[t]); }
  }
}
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, const AdamEma* ema, const float* sc,
                const float* scalars_dev, hipStream_t s, const int* skip, const AdamDecay* wd) {
  static const AdamEma none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  const AdamEma& E = ema ? *ema : none;
  const int64_t head = adam_head(p, g, m, v, E.p, n);
  const dim3 grid(grid_for(ceil_div64(n, 4), 256, 4096));
#define FU_ADAM(K, SC)                                                                                            \
  hipLaunchKernelGGL(K, grid, dim3(256), 0, s, p, g, m, v, E.p, n, head, SC, E.rm_ema, E.rm, E.rv_ema, E.rv, E.nbn, skip)
#define FU_ADAMW(K, SC)                                                                                            \
  hipLaunchKernelGGL(K, grid, dim3(256), 0, s, p, g, m, v, E.p, n, head, SC, E.rm_ema, E.rm, E.rv_ema, E.rv, E.nbn, skip, \
                     wd->bounds, wd->nb)
  if (wd) {
    FU_REQUIRE(wd->bounds && wd->nb >= 2 && wd->nb <= 2 * WD_MAX_RANGES && wd->nb % 2 == 0,
               "weight decay: %d range bounds, 2 to %d in pairs supported", wd->nb, 2 * WD_MAX_RANGES);
    if (scalars_dev) {
      if (ema) FU_ADAMW(k_adamw_ema_dev, scalars_dev);
      else FU_ADAMW(k_adamw_dev, scalars_dev);
    } else {
      const AdamScalars as = {sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], ema ? sc[7] : 0.f, sc[8]};
      if (ema) FU_ADAMW(k_adamw_ema, as);
      else FU_ADAMW(k_adamw, as);
    }
  } else if (scalars_dev) {
    if (ema) FU_ADAM(k_adam_ema_dev, scalars_dev);
    else FU_ADAM(k_adam_dev, scalars_dev);
  } else {
    const AdamScalars as = {sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], ema ? sc[7] : 0.f, 1.f};
    if (ema) FU_ADAM(k_adam_ema, as);
    else FU_ADAM(k_adam, as);
  }
#undef FU_ADAM
#undef FU_ADAMW
  FU_LAUNCH_CHECK();
  return 0;
}

// fp16 guard.  The loss scale is chosen once per backward from max|dL/dlogits|; what the chain multiplies on top (a
// BatchNorm with a tiny variance: gamma * invstd in the hundreds) can still push an fp16 gradient map past 65504.  The inf /
// NaN then reaches the flat gradient buffer; guard[0] flags it, the Adam launch of that step does nothing, and the next
// backward's scale is halved once more (guard[2] = back-off exponent, taken back by one every 64 clean steps).
//   guard[0] non-finite flag of the running step, [1] steps skipped so far, [2] back-off exponent, [3] clean steps since
// Every element is examined once: a scalar head up to the first 16-byte boundary (the gradient buffer is bound at any 4-byte
// alignment, as for adam_body and k_grad_sqnorm_chunks), 16-byte loads over the body, a scalar tail -- head and tail, at
// most 3 + 3 elements, by the first lanes of workgroup 0.
__global__ __launch_bounds__(256) void k_grad_finite_check(const float* __restrict__ g, int64_t n, int* __restrict__ guard) {
  int64_t head = (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t nvec = (n - head) >> 2;
  const float4* __restrict__ body = reinterpret_cast<const float4*>(g + head);
  bool bad = false;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nvec; j += (int64_t)gridDim.x * 256) {
    const float4 v = body[j];
    bad = bad || !(fabsf(v.x) <= 3.0e38f) || !(fabsf(v.y) <= 3.0e38f) || !(fabsf(v.z) <= 3.0e38f) || !(fabsf(v.w) <= 3.0e38f);
  }
  const int64_t tail0 = head + 4 * nvec, nrest = head + (n - tail0);
  if (blockIdx.x == 0 && threadIdx.x < nrest)
    bad = bad || !(fabsf(g[threadIdx.x < head ? (int64_t)threadIdx.x : tail0 + (threadIdx.x - head)]) <= 3.0e38f);
  if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(guard, 1);
}
__global__ void k_guard_book(int* __restrict__ guard) {
  if (guard[0]) { guard[1] += 1; guard[2] = min(guard[2] + 1, 14); guard[3] = 0; guard[0] = 0; }
  else if (++guard[3] >= 64) { guard[3] = 0; guard[2] = max(guard[2] - 1, 0); }
}
int launch_grad_finite_check(const float* g, int64_t n, int* guard, hipStream_t s) {
  hipLaunchKernelGGL(k_grad_finite_check, dim3(grid_for(n, 1024 * 4, 2048)), dim3(256), 0, s, g, n, guard);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_guard_book(int* guard, hipStream_t s) {
  hipLaunchKernelGGL(k_guard_book, dim3(1), dim3(1), 0, s, guard);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) ahead of the Adam launch, and the gradient-norm report.
// The Adam kernels above are not involved: clipping only replaces the one scalar they multiply every gradient by (gscale,
// slot 6), computed on the device by two launches: k_grad_sqnorm_chunks streams the gradient buffer once and WRITES one
// double per chunk (no atomics; the result does not depend on the grid), k_grad_norm_finalize (one workgroup) sums the
// chunks of each tensor in chunk order, the tensors in parameter order, and forms the coefficient.  Every element is
// squared in double -- exact for an fp32 value -- so gradients of 1e30 or 1e-30 neither overflow nor vanish.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq4_acc(double a, const float4 x) {
  const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
  a = fma(x0, x0, a);
  a = fma(x1, x1, a);
  a = fma(x2, x2, a);
  return fma(x3, x3, a);
}
// One chunk per workgroup turn: scalar head up to the first 16-byte boundary (a chunk starts at any float offset and the
// buffer is bound at any 4-byte alignment), 16-byte loads four in flight per lane, scalar tail; lane sums in a fixed order,
// wave butterfly, then the four waves through LDS in wave order.
__global__ __launch_bounds__(256) void k_grad_sqnorm_chunks(const float* __restrict__ g, const ClipChunk* __restrict__ chunks,
                                                            int nchunks, double* __restrict__ part) {
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const ClipChunk ck = chunks[c];
    const float* __restrict__ p = g + ck.off;
    const int len = ck.len;
    int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const float4* __restrict__ v = reinterpret_cast<const float4*>(p + head);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = tid;
    for (; j + 768 < nvec; j += 1024) {
      const float4 x0 = v[j], x1 = v[j + 256], x2 = v[j + 512], x3 = v[j + 768];
      a0 = sq4_acc(a0, x0);
      a1 = sq4_acc(a1, x1);
      a2 = sq4_acc(a2, x2);
      a3 = sq4_acc(a3, x3);
    }
    for (; j < nvec; j += 256) a0 = sq4_acc(a0, v[j]);
    const int tail0 = head + 4 * nvec, nrest = head + (len - tail0);      // at most 3 + 3 elements
    if (tid < nrest) {
      const double x = (double)p[tid < head ? tid : tail0 + (tid - head)];
      a1 = fma(x, x, a1);
    }
    double a = (a0 + a1) + (a2 + a3);
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) part[c] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();                                                       // wsum is free for the next chunk
  }
}

struct ClipScalars { float v[9]; };
// src[lo] + src[lo + 1] + ... in that order; the loads of eight terms are issued ahead of their adds, so that the chain
// costs an add per term, not a memory round trip
__device__ __forceinline__ double ordered_sum(const double* src, int lo, int hi) {
  double s = 0.0;
  int i = lo;
  for (; i + 8 <= hi; i += 8) {
    const double x0 = src[i], x1 = src[i + 1], x2 = src[i + 2], x3 = src[i + 3], x4 = src[i + 4], x5 = src[i + 5],
                 x6 = src[i + 6], x7 = src[i + 7];
    s += x0; s += x1; s += x2; s += x3; s += x4; s += x5; s += x6; s += x7;
  }
  for (; i < hi; ++i) s += src[i];
  return s;
}
constexpr int CLIP_FIN_CHUNKS = 4096;    // partials staged in LDS up to this many chunks (32 KB); more are read in place
constexpr int CLIP_MAX_PARAMS = 1024;    // per-tensor sums live in LDS (build_grad_clip refuses a longer parameter table)
// sc_dev == null: the caller's scalars are scv (by value); else nsc floats (7, 8 with the EMA weight, 9 with the decay factor)
// are read from sc_dev.
// out_sc == null: no scalar part, no state (fu_grad_norms); norms_out == null: no per-tensor report (the optimiser step).
__global__ __launch_bounds__(256) void k_grad_norm_finalize(const double* __restrict__ part, const int* __restrict__ first,
                                                            int nparams, int nchunks, ClipScalars scv,
                                                            const float* __restrict__ sc_dev, int nsc, double max_norm,
                                                            float* __restrict__ out_sc, ClipState* __restrict__ st,
                                                            float* __restrict__ norms_out, double report_scale) {
#pragma clang fp contract(off)
  __shared__ double lpart[CLIP_FIN_CHUNKS];
  __shared__ double tsq[CLIP_MAX_PARAMS];
  const int tid = threadIdx.x;
  const bool staged = nchunks <= CLIP_FIN_CHUNKS;
  float in[9];                                        // read ahead of the sums: nothing below waits for these loads
  for (int k = 0; k < 9; ++k) in[k] = !out_sc ? 0.f : sc_dev ? (k < nsc ? sc_dev[k] : 0.f) : scv.v[k];
  if (staged) {
    for (int i = tid; i < nchunks; i += 256) lpart[i] = part[i];
    __syncthreads();
  }
  for (int t = tid; t < nparams; t += 256) {
    const int lo = first[t], hi = first[t + 1];
    tsq[t] = staged ? ordered_sum(lpart, lo, hi) : ordered_sum(part, lo, hi);
  }
  __syncthreads();
  if (norms_out)
    for (int t = tid; t < nparams; t += 256) norms_out[t] = (float)(sqrt(tsq[t]) * fabs(report_scale));
  if (tid != 0) return;
  const double total = ordered_sum(tsq, 0, nparams);
  if (norms_out) norms_out[nparams] = (float)(sqrt(total) * fabs(report_scale));
  if (!out_sc) return;
  const float gscale_in = in[6];
  const double N = sqrt(total) * fabs((double)gscale_in);
  const bool finite = isfinite(N);
  const double r = max_norm / (N + 1e-6);
  const float coef = (max_norm > 0.0 && finite && r < 1.0) ? (float)r : 1.0f;
  for (int k = 0; k < 9; ++k) out_sc[k] = in[k];
  out_sc[6] = gscale_in * coef;
  st->last_norm = (float)N;
  st->last_coef = coef;
  st->skip = finite ? 0 : 1;
  st->steps += 1;
  if (coef < 1.0f) st->clipped += 1;
  if (!finite) st->nonfinite += 1;
}

void plan_clip_chunks(const int64_t* off, const int64_t* numel, int nparams, std::vector<ClipChunk>* chunks,
                      std::vector<int>* first) {
  chunks->clear();
  first->assign(1, 0);
  for (int t = 0; t < nparams; ++t) {
    for (int64_t o = 0; o < numel[t]; o += CLIP_CHUNK)
      chunks->push_back({off[t] + o, (int32_t)std::min<int64_t>(CLIP_CHUNK, numel[t] - o), t});
    first->push_back((int)chunks->size());
  }
}
int build_grad_clip(GradClip* w, const int64_t* off, const int64_t* numel, int nparams, std::vector<void*>* allocs) {
  if (w->chunks) return 0;
  FU_REQUIRE(nparams >= 1 && nparams <= CLIP_MAX_PARAMS, "gradient norm: %d parameter tensors, at most %d supported", nparams,
             CLIP_MAX_PARAMS);
  std::vector<ClipChunk> chunks;
  std::vector<int> first;
  plan_clip_chunks(off, numel, nparams, &chunks, &first);
  const size_t nch = chunks.size();
  // one allocation: chunks | first | partials | state | scalars, each on a 256-byte boundary
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_first = up(nch * sizeof(ClipChunk)), o_part = o_first + up(first.size() * sizeof(int)),
               o_state = o_part + up(nch * sizeof(double)), o_scal = o_state + up(sizeof(ClipState)),
               total = o_scal + up(9 * sizeof(float));
  char* base = nullptr;
  FU_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&base), total));
  allocs->push_back(base);
  FU_HIP_CHECK(hipMemset(base, 0, total));
  if (nch) FU_HIP_CHECK(hipMemcpy(base, chunks.data(), nch * sizeof(ClipChunk), hipMemcpyHostToDevice));
  FU_HIP_CHECK(hipMemcpy(base + o_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice));
  w->first = reinterpret_cast<int*>(base + o_first);
  w->part = reinterpret_cast<double*>(base + o_part);
  w->state = reinterpret_cast<ClipState*>(base + o_state);
  w->scalars = reinterpret_cast<float*>(base + o_scal);
  w->nchunks = (int)nch;
  w->nparams = nparams;
  w->chunks = reinterpret_cast<ClipChunk*>(base);
  return 0;
}
int launch_grad_sqnorm(const GradClip& w, const float* g, hipStream_t s) {
  if (w.nchunks == 0) return 0;
  hipLaunchKernelGGL(k_grad_sqnorm_chunks, dim3(std::min(w.nchunks, 2048)), dim3(256), 0, s, g, w.chunks, w.nchunks, w.part);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_grad_clip_finalize(const GradClip& w, const float* sc, const float* sc_dev, int n, double max_norm, hipStream_t s) {
  ClipScalars scv = {};
  if (!sc_dev) for (int k = 0; k < n; ++k) scv.v[k] = sc[k];
  hipLaunchKernelGGL(k_grad_norm_finalize, dim3(1), dim3(256), 0, s, w.part, w.first, w.nparams, w.nchunks, scv, sc_dev,
                     n, max_norm, w.scalars, w.state, (float*)nullptr, 0.0);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_grad_norms_out(const GradClip& w, double grad_scale, float* norms_out, hipStream_t s) {
  hipLaunchKernelGGL(k_grad_norm_finalize, dim3(1), dim3(256), 0, s, w.part, w.first, w.nparams, w.nchunks, ClipScalars{},
                     (const float*)nullptr, 0, 0.0, (float*)nullptr, (ClipState*)nullptr, norms_out, grad_scale);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
