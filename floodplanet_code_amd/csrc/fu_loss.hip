// Loss kernels of the training step (gfx950): softmax cross entropy (plain, class-weighted / label-smoothed, focal), the soft
// Tversky region term that goes with it, and BCE + soft Dice over the resident logits, with their deterministic reductions; the NCHW -> NHWC copy of an external
// logits gradient; the gradient the head backward consumes (upstream factor, fp16 loss scale).
#include "fu_common.h"

namespace fu {

// ------------------------------------------------------------------------------------------------
// The reduction the loss kernels share: per-thread fp32 sums -> one row of N partials per block -> N fp64 sums.  Every
// order is fixed (the lanes of a wave by wave_sum, the waves of a block in index order, the rows by thread index and a
// 256-wide tree), so a loss is the same bits on every run; sync_sum_over_ranks goes between the two helpers.
// ------------------------------------------------------------------------------------------------
static constexpr int CE_BLOCK = 256;
// rows of partials per launch: the partial buffer (LOSS_PART_FLOATS, fu_common.h) holds CE_MAX_BLOCKS rows of the widest
// CE form (four sums).  Both CE forms use this one cap: their grids, and with them their bits for w = 1, eps = 0, agree.
static constexpr int CE_MAX_BLOCKS = LOSS_PART_FLOATS / 4;
// BCE + Dice keeps the 400 rows of five sums its loss values were recorded with (the cap sets the summation order)
static constexpr int BD_MAX_BLOCKS = 400;
static_assert(4 * CE_MAX_BLOCKS <= LOSS_PART_FLOATS && 5 * BD_MAX_BLOCKS <= LOSS_PART_FLOATS, "loss partial rows");

// acc[N] of every thread of a CE_BLOCK-wide block -> row[N]: wave sums, LDS, the first N threads add the waves in order
template <int N>
__device__ __forceinline__ void block_partial_row(const float (&acc)[N], float* __restrict__ row) {
  __shared__ float wsum[CE_BLOCK / 64][N];
  float v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = wave_sum(acc[j]);
  if ((threadIdx.x & 63) == 0) {            // (one predicated region: the N stores merge into wide LDS writes)
#pragma unroll
    for (int j = 0; j < N; ++j) wsum[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    float t = 0.f;
    for (int wv = 0; wv < CE_BLOCK / 64; ++wv) t += wsum[wv][threadIdx.x];
    row[threadIdx.x] = t;
  }
}

// partials[nblk][N] -> out[N] in every thread of one 256-wide block: fp64, fixed tree (deterministic)
template <int N>
__device__ __forceinline__ void partial_rows_sum(const float* __restrict__ partials, int nblk, double (&out)[N]) {
  __shared__ double sm[N][256];
  double a[N];
#pragma unroll
  for (int j = 0; j < N; ++j) a[j] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] += (double)partials[i * N + j];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) sm[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int j = 0; j < N; ++j) sm[j][threadIdx.x] += sm[j][threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < N; ++j) out[j] = sm[j][0];
}

// ------------------------------------------------------------------------------------------------
// softmax cross entropy with ignore_index (water_seg_model.py:40,103-107), argmax, confusion counts -- and its
// class-weighted, label-smoothed extension (fu_loss_ce_weighted; the reference has no such loss, the specification is
// torch.nn.functional.cross_entropy(weight, ignore_index, label_smoothing)).  Over the valid pixels, with p = softmax(z),
// W = sum_c w[c]:
//   WEIGHTED == false:  loss = sum_i (lse - z[t]) / n_valid,      dz_k = (p_k - [k == t]) / n_valid
//   WEIGHTED == true:   loss = [c_nll * sum_i w[t] (lse - z[t]) + c_smooth * sum_i sum_c w[c] (lse - z[c])] / D
//                       dz_k = [c_nll * w[t] (p_k - [k == t]) + c_smooth * (p_k W - w[k])] / D
//                       D = sum_i w[t_i],  c_nll = 1 - eps,  c_smooth = eps / C
// WEIGHTED is a compile-time flag: the plain instantiation has no weight loads, no smoothing sum, no D, and two partials
// per block where the weighted one has four.  Grid, per-thread order, lse and softmax expressions and the reduction are
// shared, so w = 1, eps = 0 reproduces the plain bits (every extra factor is then an exact 1 or 0).  NC as in k_head_fwd:
// compile-time class count, 0 = any count up to HEAD_MAX_CLS; the weights are uniform values loaded once per thread.
// D == 0 gives loss 0 and a zero gradient (the rule of the all-ignored batch).
//   FOCAL (a WEIGHTED form, gamma > 0; fu_loss_ce_focal), with q = p[t], u = 1 - q:
//                       loss = sum_i w[t] u^gamma (-log q) / D
//                       dz_k = w[t] (p_k - [k == t]) mf / D,   mf = u^gamma - gamma q u^(gamma-1) log q
// FOCAL is a third compile-time flag: the other instantiations hold none of its code (gamma is an argument they ignore).
// It fills the weighted row of four
// sums (the smoothing sum stays 0), so k_ce_finalize<true> with c_nll = 1, c_smooth = 0 and the exact-mode sum over the
// ranks serve it unchanged.  gamma == 0 never gets here: the launchers send it to the WEIGHTED instantiation.
// ------------------------------------------------------------------------------------------------
// The focal terms of one pixel, free of cancellation.  e[k] = exp(z[k] - m); u is the OTHER classes' share of the sum (not
// 1 - q: that is 0 for every q within 2^-24 of 1); -log q is log(se) - (z[t] - m), and log1p(so) where the target holds
// the maximum (its exponential is then exactly 1, se = 1 + so).  A target outside 0..ncls-1 (an ignored pixel) gives
// finite values the callers discard.
template <int KMAX>
__device__ __forceinline__ void focal_terms(const float (&z)[KMAX], float m, int ncls, int t, float (&e)[KMAX], float& se,
                                            float& u, float& q, float& nlq) {
  float et = 0.f, so = 0.f, zt = m;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < ncls) {
      e[k] = expf(z[k] - m);
      if (k == t) { et = e[k]; zt = z[k]; } else so += e[k];
    }
  }
  se = et + so;
  u = so / se;
  q = et / se;
  nlq = (zt == m) ? log1pf(so) : logf(se) - (zt - m);
}
// u^gamma for gamma > 0; u == 0 (the other classes' exponentials underflowed): exactly 0, the pixel drops out
__device__ __forceinline__ float focal_pow(float u, float gamma) { return u > 0.f ? powf(u, gamma) : 0.f; }

template <int NC, bool WEIGHTED, bool FOCAL>
__global__ __launch_bounds__(CE_BLOCK) void k_ce_loss(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                      int ncls_rt, int ignore_index, int64_t npix,
                                                      const float* __restrict__ class_weight,
                                                      float* __restrict__ partials,
                                                      unsigned long long* __restrict__ conf_tmp, float gamma) {
  static_assert(WEIGHTED || !FOCAL, "the focal form is a weighted form");
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  constexpr int NS = WEIGHTED ? 4 : 2;   // plain: nll sum, valid count; weighted: w[t] nll, smoothing term, w[t], count
  const int ncls = NC ? NC : ncls_rt;
  __shared__ unsigned int hist[HEAD_MAX_CLS * HEAD_MAX_CLS];
  for (int i = threadIdx.x; i < ncls * ncls; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  float w[WEIGHTED ? KMAX : 1];
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) w[k] = (k < ncls) ? (class_weight ? class_weight[k] : 1.f) : 0.f;
  }
  float acc[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j] = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    float z[KMAX];
    float m = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < ncls) {
        z[k] = logits[p * ncls + k];
        if (z[k] > m) { m = z[k]; am = k; }
      }
    }
    if (t != (int64_t)ignore_index && t >= 0 && t < ncls) {
      if constexpr (FOCAL) {
        float e[KMAX], se, u, q, nlq, wt = 0.f;
        focal_terms<KMAX>(z, m, ncls, (int)t, e, se, u, q, nlq);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < ncls && k == (int)t) wt = w[k];
        acc[0] += wt * (focal_pow(u, gamma) * nlq);
        acc[2] += wt;
      } else {
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < ncls) se += expf(z[k] - m);
        const float lse = m + logf(se);
        float zt = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < ncls && k == (int)t) zt = z[k];
        if constexpr (WEIGHTED) {
          float wt = 0.f, sm = 0.f;
#pragma unroll
          for (int k = 0; k < KMAX; ++k) {
            if (k < ncls) {
              if (k == (int)t) wt = w[k];
              sm += w[k] * (lse - z[k]);
            }
          }
          acc[0] += wt * (lse - zt);
          acc[1] += sm;
          acc[2] += wt;
        } else {
          acc[0] += lse - zt;
        }
      }
      acc[NS - 1] += 1.f;
      atomicAdd(&hist[(int)t * ncls + am], 1u);
    }
  }
  block_partial_row<NS>(acc, partials + blockIdx.x * NS);
  for (int i = threadIdx.x; i < ncls * ncls; i += blockDim.x)
    if (hist[i]) atomicAdd(&conf_tmp[i], (unsigned long long)hist[i]);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_ce_finalize(const float* __restrict__ partials, int nblk, int ncls, float c_nll,
                                                     float c_smooth, float* __restrict__ loss_out,
                                                     int64_t* __restrict__ n_valid_dev, float* __restrict__ weight_sum_dev,
                                                     unsigned long long* __restrict__ conf_tmp,
                                                     int64_t* __restrict__ conf_accum, int64_t* __restrict__ n_valid_out,
                                                     float* __restrict__ weight_sum_out) {
  constexpr int NS = WEIGHTED ? 4 : 2;
  double a[NS];
  partial_rows_sum<NS>(partials, nblk, a);
  if (threadIdx.x == 0) {
    const double c = a[NS - 1];
    float loss;
    if constexpr (WEIGHTED) {
      const double nll = a[0], smooth = a[1], D = a[2];
      double num = (double)c_nll * nll;
      if (c_smooth != 0.f) num += (double)c_smooth * smooth;
      // mean over the weights of the valid pixels; D == 0: torch's NaN -> 0, the rule of the all-ignored batch
      loss = D > 0.0 ? (float)(num / D) : 0.f;
      *weight_sum_dev = (float)D;
      if (weight_sum_out) *weight_sum_out = (float)D;
    } else {
      // CrossEntropyLoss mean over non-ignored pixels; 0/0 = NaN -> nan_to_num -> 0  (water_seg_model.py:104-106)
      loss = c > 0.0 ? (float)(a[0] / c) : 0.f;
    }
    if (loss_out) *loss_out = loss;
    *n_valid_dev = (int64_t)(c + 0.5);
    if (n_valid_out) *n_valid_out = (int64_t)(c + 0.5);
  }
  for (int i = threadIdx.x; i < ncls * ncls; i += blockDim.x) {
    if (conf_accum) conf_accum[i] += (int64_t)conf_tmp[i];
    conf_tmp[i] = 0ull;
  }
}

#define FU_NC_SWITCH(ncls, LAUNCH) \
  switch (ncls) {                  \
    case 1: LAUNCH(1); break;      \
    case 2: LAUNCH(2); break;      \
    case 3: LAUNCH(3); break;      \
    case 4: LAUNCH(4); break;      \
    default: LAUNCH(0); break;     \
  }

int launch_ce_loss(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                   const CeWeighting* cw, float* partials, float* loss_out, int64_t* n_valid_dev,
                   int64_t* confusion_accum, int64_t* n_valid_out, unsigned long long* conf_tmp, const SyncDesc* sync,
                   hipStream_t s) {
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "CE: n_classes must be 1..%d", HEAD_MAX_CLS);
  const int nblk = grid_for(npix, CE_BLOCK, CE_MAX_BLOCKS);
  const bool focal = cw && cw->focal_gamma > 0.f;     // gamma == 0 is the weighted loss itself: its instantiation, its bits
#define FU_CE_LOSS_AS(NC, WEIGHTED, FOCAL, CLASS_WEIGHT, GAMMA)                                                    \
  hipLaunchKernelGGL((k_ce_loss<NC, WEIGHTED, FOCAL>), dim3(nblk), dim3(CE_BLOCK), 0, s, logits_nhwc, target, ncls, \
                     ignore_index, npix, CLASS_WEIGHT, partials, conf_tmp, GAMMA)
#define FU_CE_LOSS(NC)                                                  \
  do {                                                                  \
    if (focal)                                                          \
      FU_CE_LOSS_AS(NC, true, true, cw->class_weight, cw->focal_gamma); \
    else if (cw)                                                        \
      FU_CE_LOSS_AS(NC, true, false, cw->class_weight, 0.f);            \
    else                                                                \
      FU_CE_LOSS_AS(NC, false, false, nullptr, 0.f);                    \
  } while (0)
  FU_NC_SWITCH(ncls, FU_CE_LOSS);
#undef FU_CE_LOSS
#undef FU_CE_LOSS_AS
  FU_LAUNCH_CHECK();
  // exact DP: the global sums (loss, N_valid; weighted: D too) before the division
  FU_TRY(sync_sum_over_ranks(sync, partials, (int64_t)nblk * (cw ? 4 : 2), false, s));
  if (cw)
    hipLaunchKernelGGL(k_ce_finalize<true>, dim3(1), dim3(256), 0, s, partials, nblk, ncls, cw->c_nll, cw->c_smooth,
                       loss_out, n_valid_dev, cw->weight_sum_dev, conf_tmp, confusion_accum, n_valid_out,
                       cw->weight_sum_out);
  else
    hipLaunchKernelGGL(k_ce_finalize<false>, dim3(1), dim3(256), 0, s, partials, nblk, ncls, 1.f, 0.f, loss_out,
                       n_valid_dev, nullptr, conf_tmp, confusion_accum, n_valid_out, nullptr);
  FU_LAUNCH_CHECK();
  return 0;
}

template <int NC, bool WEIGHTED, bool FOCAL>
__global__ __launch_bounds__(256) void k_ce_grad(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                 int ncls_rt, int ignore_index, int64_t npix,
                                                 const float* __restrict__ class_weight, float c_nll, float c_smooth,
                                                 const int64_t* __restrict__ n_valid, const float* __restrict__ weight_sum,
                                                 float* __restrict__ dl, float gamma) {
  static_assert(WEIGHTED || !FOCAL, "the focal form is a weighted form");
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  bool live;
  float inv;
  if constexpr (WEIGHTED) {
    const float D = *weight_sum;
    live = D > 0.f;
    inv = live ? 1.f / D : 0.f;
  } else {
    const int64_t nv = *n_valid;
    live = nv > 0;
    inv = live ? 1.f / (float)nv : 0.f;
  }
  float w[WEIGHTED ? KMAX : 1];
  float W = 0.f;
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      w[k] = (k < ncls) ? (class_weight ? class_weight[k] : 1.f) : 0.f;
      W += w[k];
    }
  }
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    const bool valid = (t != (int64_t)ignore_index && t >= 0 && t < ncls) && live;
    float z[KMAX];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < ncls) { z[k] = logits[p * ncls + k]; m = fmaxf(m, z[k]); }
    if constexpr (FOCAL) {
      float e[KMAX], se, u, q, nlq, wt = 0.f;
      focal_terms<KMAX>(z, m, ncls, (int)t, e, se, u, q, nlq);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < ncls && (int)t == k) wt = w[k];
      // mf = u^gamma (1 + gamma q (-log q) / u): -log q / u stays within [1, -log q], where u^(gamma-1) alone overflows
      // for a denormal u and gamma < 1; u == 0 drops the pixel (no 0^(gamma-1) * 0)
      const float mf = u > 0.f ? powf(u, gamma) * (1.f + gamma * q * (nlq / u)) : 0.f;
      const float a = wt * mf * inv, r = 1.f / se;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)                        // (p_t - 1 is -u, without the cancellation)
        if (k < ncls) dl[p * ncls + k] = valid ? a * ((int)t == k ? -u : e[k] * r) : 0.f;
      continue;
    }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < ncls) { z[k] = expf(z[k] - m); se += z[k]; }
    const float r = 1.f / se;
    if constexpr (WEIGHTED) {
      float wt = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < ncls && (int)t == k) wt = w[k];
      const float a = c_nll * wt, rW = r * W;   // (p_k W as e_k (r W): p_k - [k == t] keeps the plain expression)
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < ncls) {
          const float g = a * (z[k] * r - ((int)t == k ? 1.f : 0.f)) + c_smooth * (z[k] * rW - w[k]);
          dl[p * ncls + k] = valid ? g * inv : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < ncls) dl[p * ncls + k] = valid ? (z[k] * r - ((int)t == k ? 1.f : 0.f)) * inv : 0.f;
    }
  }
}

int launch_ce_grad(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                   const CeWeighting* cw, const int64_t* n_valid_dev, float* dlogits_nhwc, hipStream_t s) {
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "CE: n_classes must be 1..%d", HEAD_MAX_CLS);
  const int g = grid_for(npix, 256, 4096);
  const bool focal = cw && cw->focal_gamma > 0.f;
#define FU_CE_GRAD_AS(NC, WEIGHTED, FOCAL, CLASS_WEIGHT, C_NLL, C_SMOOTH, WEIGHT_SUM, GAMMA)                        \
  hipLaunchKernelGGL((k_ce_grad<NC, WEIGHTED, FOCAL>), dim3(g), dim3(256), 0, s, logits_nhwc, target, ncls,         \
                     ignore_index, npix, CLASS_WEIGHT, C_NLL, C_SMOOTH, n_valid_dev, WEIGHT_SUM, dlogits_nhwc, GAMMA)
#define FU_CE_GRAD(NC)                                                                                    \
  do {                                                                                                    \
    if (focal)                                                                                            \
      FU_CE_GRAD_AS(NC, true, true, cw->class_weight, 1.f, 0.f, cw->weight_sum_dev, cw->focal_gamma);     \
    else if (cw)                                                                                          \
      FU_CE_GRAD_AS(NC, true, false, cw->class_weight, cw->c_nll, cw->c_smooth, cw->weight_sum_dev, 0.f); \
    else                                                                                                  \
      FU_CE_GRAD_AS(NC, false, false, nullptr, 1.f, 0.f, nullptr, 0.f);                                   \
  } while (0)
  FU_NC_SWITCH(ncls, FU_CE_GRAD);
#undef FU_CE_GRAD
#undef FU_CE_GRAD_AS
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The soft Tversky region term added to a cross entropy (fu_loss_ce_region; the reference has no such loss, the
// specification is tests/tools/region_ref.py).  Over the valid pixels of the CE, p = softmax(z), y_ik = [t_i == k]:
//   I_k = sum_i p_ik y_ik,  P_k = sum_i p_ik,  T_k = sum_i y_ik,  Num_k = I_k + s,
//   Den_k = I_k + alpha (P_k - I_k) + beta (T_k - I_k) + s,  TI_k = Num_k / Den_k,
//   R = sum_{k in K} (1 - TI_k) / |K|,  K = the classes but ignore_index;  loss = CE + lambda R
//   d(lambda R)/dz_ij = lambda p_ij (g_ij - sum_k g_ik p_ik),  g_ik = y_ik ? A_k : B_k,
//   A_k = -(alpha (P_k - I_k) + beta (T_k + s)) / (|K| Den_k^2),  B_k = alpha Num_k / (|K| Den_k^2)   (0 outside K)
// Passes of their own after the CE's, which stay as they are: k_region_sums -> (exact DP: the sum over the ranks) ->
// k_region_finalize (fp64: R added to the loss the CE finalize wrote, A / B / lambda left on the device) ->
// k_region_grad_add (training forwards: added to the stored CE gradient, valid pixels only).  The term follows pixel
// validity, not the CE's summed weight D: valid pixels of zero-weight classes keep it alive.  No valid pixel: every sum is
// 0, TI_k = s / s, R = 0 exactly, and the gradient pass touches nothing.
// ------------------------------------------------------------------------------------------------
// rows of partials per launch: a row is 3 sums for each of KMAX classes (KMAX = the class count up to 4, else HEAD_MAX_CLS),
// and as many rows as fit the partial buffer are used: 682 / 455 / 341 blocks for 2 / 3 / 4 classes, 170 beyond.  The cap
// sets the summation order (tests/tools/region_ref.py: region_cap).
static constexpr int region_max_blocks(int kmax) { return LOSS_PART_FLOATS / (3 * kmax); }
static_assert(3 * HEAD_MAX_CLS * region_max_blocks(HEAD_MAX_CLS) <= LOSS_PART_FLOATS && region_max_blocks(HEAD_MAX_CLS) >= 1,
              "region partial rows");
static_assert(3 * HEAD_MAX_CLS * 256 * sizeof(double) <= 64 * 1024, "partial_rows_sum of a region row: static LDS");
static constexpr int REGION_COEF_FLOATS = 2 * HEAD_MAX_CLS + 1;   // A[HEAD_MAX_CLS], B[HEAD_MAX_CLS], lambda
static_assert(REGION_COEF_FLOATS * sizeof(float) <= REGION_COEF_BYTES, "region coefficient buffer");

// row of a block: I[KMAX], P[KMAX], T[KMAX] (T: counts, exact in fp32 -- a block adds fewer than 2^24 pixels)
template <int NC>
__global__ __launch_bounds__(CE_BLOCK) void k_region_sums(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ target, int ncls_rt,
                                                          int ignore_index, int64_t npix, float* __restrict__ partials) {
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  float acc[3 * KMAX];
#pragma unroll
  for (int j = 0; j < 3 * KMAX; ++j) acc[j] = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    if (t != (int64_t)ignore_index && t >= 0 && t < ncls) {
      float e[KMAX];
      float m = -INFINITY, se = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < ncls) { e[k] = logits[p * ncls + k]; m = fmaxf(m, e[k]); }
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < ncls) { e[k] = expf(e[k] - m); se += e[k]; }
      const float r = 1.f / se;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < ncls) {
          const float pk = e[k] * r;
          const bool hit = (int)t == k;
          acc[k] += hit ? pk : 0.f;
          acc[KMAX + k] += pk;
          acc[2 * KMAX + k] += hit ? 1.f : 0.f;
        }
      }
    }
  }
  block_partial_row<3 * KMAX>(acc, partials + blockIdx.x * (3 * KMAX));
}

// one block.  coef: A[HEAD_MAX_CLS], B[HEAD_MAX_CLS], lambda; loss_io: the scalar the CE finalize wrote; region_out: optional
// [1 + ncls] = R, TI_k (1 for the ignored class).  P_k - I_k and T_k - I_k are >= 0 in exact arithmetic; their fp32 partials
// are rounded separately, so they are held at 0 from below.
template <int KMAX>
__global__ __launch_bounds__(256) void k_region_finalize(const float* __restrict__ partials, int nblk, int ncls,
                                                         int ignore_index, float lambda, float alpha, float beta,
                                                         float smooth, float* __restrict__ loss_io,
                                                         float* __restrict__ coef, float* __restrict__ region_out) {
  double a[3 * KMAX];
  partial_rows_sum<3 * KMAX>(partials, nblk, a);
  if (threadIdx.x != 0) return;
  int nk = 0;
  for (int k = 0; k < ncls; ++k) nk += (k != ignore_index);
  const double al = alpha, be = beta, s = smooth;
  double R = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const bool in = k < ncls && k != ignore_index;
    const double I = a[k], T = a[2 * KMAX + k];
    const double fp = fmax(a[KMAX + k] - I, 0.0), fn = fmax(T - I, 0.0);
    const double num = I + s, den = I + al * fp + be * fn + s;
    const double ti = num / den, q = in ? 1.0 / ((double)nk * den * den) : 0.0;
    if (in) R += 1.0 - ti;
    coef[k] = (float)(-(al * fp + be * (T + s)) * q);
    coef[HEAD_MAX_CLS + k] = (float)(al * num * q);
    if (region_out && k < ncls) region_out[1 + k] = in ? (float)ti : 1.f;
  }
  for (int k = KMAX; k < HEAD_MAX_CLS; ++k) coef[k] = coef[HEAD_MAX_CLS + k] = 0.f;
  R = nk > 0 ? R / nk : 0.0;
  coef[2 * HEAD_MAX_CLS] = lambda;
  *loss_io += (float)((double)lambda * R);
  if (region_out) region_out[0] = (float)R;
}

// dl += lambda p_j (g_j - sum_k g_k p_k) on the valid pixels; the others are not read, not written
template <int NC>
__global__ __launch_bounds__(256) void k_region_grad_add(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int ncls_rt,
                                                         int ignore_index, int64_t npix, const float* __restrict__ coef,
                                                         float* __restrict__ dl) {
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  float A[KMAX], B[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { A[k] = coef[k]; B[k] = coef[HEAD_MAX_CLS + k]; }
  const float lambda = coef[2 * HEAD_MAX_CLS];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = target[p];
    if (!(t != (int64_t)ignore_index && t >= 0 && t < ncls)) continue;
    float e[KMAX], g[KMAX];
    float m = -INFINITY, se = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < ncls) { e[k] = logits[p * ncls + k]; m = fmaxf(m, e[k]); }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < ncls) { e[k] = expf(e[k] - m); se += e[k]; }
    const float r = 1.f / se;
    float gp = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < ncls) {
        e[k] *= r;
        g[k] = (int)t == k ? A[k] : B[k];
        gp += g[k] * e[k];
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < ncls) dl[p * ncls + k] += lambda * e[k] * (g[k] - gp);
  }
}

int launch_region_term(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                       const RegionTerm& rg, float* partials, float* loss_io, float* dlogits_nhwc, const SyncDesc* sync,
                       hipStream_t s) {
  FU_REQUIRE(ncls >= 2 && ncls <= HEAD_MAX_CLS, "region term: n_classes must be 2..%d", HEAD_MAX_CLS);
  const int kmax = ncls <= 4 ? ncls : HEAD_MAX_CLS;               // the KMAX of FU_NC_SWITCH's instantiation
  const int nblk = grid_for(npix, CE_BLOCK, region_max_blocks(kmax));
#define FU_REGION_SUMS(NC)                                                                                    \
  hipLaunchKernelGGL((k_region_sums<NC>), dim3(nblk), dim3(CE_BLOCK), 0, s, logits_nhwc, target, ncls, ignore_index, \
                     npix, partials)
#define FU_REGION_FINALIZE(NC)                                                                                      \
  hipLaunchKernelGGL((k_region_finalize<(NC ? NC : HEAD_MAX_CLS)>), dim3(1), dim3(256), 0, s, partials, nblk, ncls, \
                     ignore_index, rg.weight, rg.alpha, rg.beta, rg.smooth, loss_io, rg.coef, rg.region_out)
#define FU_REGION_GRAD(NC)                                                                                         \
  hipLaunchKernelGGL((k_region_grad_add<NC>), dim3(grid_for(npix, 256, 4096)), dim3(256), 0, s, logits_nhwc, target, \
                     ncls, ignore_index, npix, rg.coef, dlogits_nhwc)
  FU_NC_SWITCH(ncls, FU_REGION_SUMS);
  FU_LAUNCH_CHECK();
  // exact DP: I, P and T of the whole batch, so that every rank forms the same R and the same coefficients
  FU_TRY(sync_sum_over_ranks(sync, partials, (int64_t)nblk * 3 * kmax, false, s));
  FU_NC_SWITCH(ncls, FU_REGION_FINALIZE);
  FU_LAUNCH_CHECK();
  if (dlogits_nhwc) {
    FU_NC_SWITCH(ncls, FU_REGION_GRAD);
    FU_LAUNCH_CHECK();
  }
#undef FU_REGION_SUMS
#undef FU_REGION_FINALIZE
#undef FU_REGION_GRAD
  return 0;
}
#undef FU_NC_SWITCH

// ------------------------------------------------------------------------------------------------
// BCE + soft Dice on p = softmax(z)[1] (north-star extension; the reference has no such loss -> parity is pinned
// only by oracle/unet_oracle.py:bce_dice_loss).  All spatial reductions in fp32 registers + wave shuffles, fp64 finalize.
//   BCE  = -(1/N) sum_valid [ t log p + (1-t) log(1-p) ],  Dice = 1 - (2 sum p t + 1) / (sum p + sum t + 1)
// ------------------------------------------------------------------------------------------------
// One pixel's terms: s = softmax(z), p = s[1], log p, log(1-p), and s1 = the softmax over the classes other than 1 (the
// derivative of their logsumexp; s1[1] = 0).  The other classes get their OWN maximum m1, as the oracle's logsumexp over
// them does: log(1-p) = (m1 - m) + log(sum_{k != 1} exp(z[k] - m1)) - log(sum_k exp(z[k] - m)), and -log1p(e[1] / that sum)
// where they hold the overall maximum (m1 == m: no difference of two nearly equal logs for a small p).  Until this form,
// both sums shared the maximum m over all classes: once class 1 led every other class by more than ~87.3 their
// exponentials were denormal (log(1-p) off by 0.02 at a margin of 100) and beyond ~104 they were 0 -- log(1-p) = -inf,
// the loss of a batch with one such background pixel inf, and s1 = 0, a gradient row that no longer sums to zero.
__device__ __forceinline__ void bd_pixel(const float* z, int ncls, float& p, float& logp, float& log1mp, float* s,
                                         float* s1) {
  float m = -INFINITY, m1 = -INFINITY;
#pragma unroll
  for (int k = 0; k < HEAD_MAX_CLS; ++k) {
    if (k < ncls) {
      m = fmaxf(m, z[k]);
      if (k != 1) m1 = fmaxf(m1, z[k]);
    }
  }
  float se = 0.f, sf = 0.f;
  float e[HEAD_MAX_CLS], f[HEAD_MAX_CLS];
#pragma unroll
  for (int k = 0; k < HEAD_MAX_CLS; ++k) {
    e[k] = k < ncls ? expf(z[k] - m) : 0.f;
    f[k] = (k < ncls && k != 1) ? expf(z[k] - m1) : 0.f;
    se += e[k];
    sf += f[k];
  }
  const float inv = 1.f / se, inv1 = 1.f / sf;        // (ncls >= 2: sf holds an exact 1, the class at m1)
#pragma unroll
  for (int k = 0; k < HEAD_MAX_CLS; ++k) { s[k] = e[k] * inv; s1[k] = f[k] * inv1; }
  p = s[1];
  const float lse = logf(se);
  logp = (z[1] - m) - lse;
  log1mp = (m1 == m) ? -log1pf(e[1] * inv1) : (m1 - m) + logf(sf) - lse;
}

__global__ void k_bd_loss(const float* __restrict__ logits, const int64_t* __restrict__ target, int ncls,
                          int ignore_index, int64_t npix, float* __restrict__ partials) {
  float acc[5] = {0, 0, 0, 0, 0};  // bce, p*t, p, t, n
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tg = target[px];
    if (tg != (int64_t)ignore_index && tg >= 0 && tg < ncls) {
      float z[HEAD_MAX_CLS], s[HEAD_MAX_CLS], s1[HEAD_MAX_CLS];
#pragma unroll
      for (int k = 0; k < HEAD_MAX_CLS; ++k) z[k] = k < ncls ? logits[px * ncls + k] : -INFINITY;
      float p, lp, l1p;
      bd_pixel(z, ncls, p, lp, l1p, s, s1);
      const float t = tg == 1 ? 1.f : 0.f;
      acc[0] -= t > 0.f ? lp : l1p;
      acc[1] += p * t; acc[2] += p; acc[3] += t; acc[4] += 1.f;
    }
  }
  block_partial_row<5>(acc, partials + blockIdx.x * 5);
}

// coef: [0] = 1/N (0 if N == 0), [1] = D, [2] = 2I+1, [3] = dice weight
__global__ __launch_bounds__(256) void k_bd_finalize(const float* __restrict__ partials, int nblk, float dice_w,
                                                     float* __restrict__ loss_out, float* __restrict__ coef,
                                                     int64_t* __restrict__ n_valid_dev) {
  double a[5];
  partial_rows_sum<5>(partials, nblk, a);
  if (threadIdx.x == 0) {
    const double bce = a[0], I = a[1], Sp = a[2], St = a[3], N = a[4];
    const double D = Sp + St + 1.0, Nn = 2.0 * I + 1.0;
    const double loss = N > 0.0 ? bce / N + (double)dice_w * (1.0 - Nn / D) : 0.0;
    if (loss_out) *loss_out = (float)loss;
    coef[0] = N > 0.0 ? (float)(1.0 / N) : 0.f;
    coef[1] = (float)D; coef[2] = (float)Nn; coef[3] = N > 0.0 ? dice_w : 0.f;
    *n_valid_dev = (int64_t)(N + 0.5);
  }
}

__global__ void k_bd_grad(const float* __restrict__ logits, const int64_t* __restrict__ target, int ncls,
                          int ignore_index, int64_t npix, const float* __restrict__ coef, float* __restrict__ dl) {
  const float invN = coef[0], D = coef[1], Nn = coef[2], w = coef[3];
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tg = target[px];
    const bool valid = tg != (int64_t)ignore_index && tg >= 0 && tg < ncls && invN > 0.f;
    float z[HEAD_MAX_CLS], s[HEAD_MAX_CLS], s1[HEAD_MAX_CLS];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) z[k] = k < ncls ? logits[px * ncls + k] : -INFINITY;
    float p, lp, l1p;
    bd_pixel(z, ncls, p, lp, l1p, s, s1);
    const float t = tg == 1 ? 1.f : 0.f;
    const float ddice = -(2.f * t * D - Nn) / (D * D);   // d Dice / d p
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) {
      if (k < ncls) {
        const float d1 = k == 1 ? 1.f : 0.f;
        const float gb = (s[k] - t * d1 - (1.f - t) * s1[k]) * invN;
        const float gd = w * ddice * p * (d1 - s[k]);
        dl[px * ncls + k] = valid ? gb + gd : 0.f;
      }
    }
  }
}

int launch_bce_dice(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                    float dice_w, float* partials, float* coef, float* loss_out, int64_t* n_valid_dev,
                    float* dlogits_nhwc, hipStream_t s) {
  FU_REQUIRE(ncls >= 2, "bce_dice needs n_classes >= 2 (class 1 = flood)");
  const int nblk = grid_for(npix, CE_BLOCK, BD_MAX_BLOCKS);
  hipLaunchKernelGGL(k_bd_loss, dim3(nblk), dim3(CE_BLOCK), 0, s, logits_nhwc, target, ncls, ignore_index, npix,
                     partials);
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bd_finalize, dim3(1), dim3(256), 0, s, partials, nblk, dice_w, loss_out, coef, n_valid_dev);
  FU_LAUNCH_CHECK();
  if (dlogits_nhwc) {
    hipLaunchKernelGGL(k_bd_grad, dim3(grid_for(npix, 256, 4096)), dim3(256), 0, s, logits_nhwc, target, ncls,
                       ignore_index, npix, coef, dlogits_nhwc);
    FU_LAUNCH_CHECK();
  }
  return 0;
}

__global__ void k_dlogits_from_nchw(const float* __restrict__ src, float* __restrict__ dst, int ncls, int HW,
                                    int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(idx % ncls);
    const int64_t p = idx / ncls;
    const int64_t bb = p / HW;
    const int pp = (int)(p % HW);
    dst[idx] = src[(bb * ncls + k) * HW + pp];
  }
}

int launch_dlogits_from_nchw(const float* dlogits_nchw, float* dlogits_nhwc, int ncls, int B, int H, int W,
                             hipStream_t s) {
  const int64_t total = (int64_t)B * H * W * ncls;
  hipLaunchKernelGGL(k_dlogits_from_nchw, dim3(grid_for(total, 256)), dim3(256), 0, s, dlogits_nchw, dlogits_nhwc, ncls,
                     H * W, total);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The gradient the head backward consumes: eff = dlogits * up * S, written OUT OF PLACE (the stored loss gradient stays as
// fu_loss_* left it, so a second backward of the same loss -- retain_graph, fu_backward_block(0) twice -- sees the same
// input; in place, the second call would have found max|dl| already in [32, 64), chosen S = 1 and unscaled by 1).
//   up: optional device scalar, the upstream gradient autograd hands to loss.backward() (fu_scale_loss_grad);
//   S:  fp16 mode only (scale != null): 2^k with max|dl * up| * S in [2^5, 2^6) -- three decades of headroom to fp16's
//       65504 for what the backward chain multiplies on top, while the bulk of the gradient maps stays in fp16's normal
//       range; chosen from the data on the device (no host read, any loss, any upstream scale).  scale[0] = S,
//       scale[1] = 1/S (fu_common.h: what the gradient-writing launches get as `unscale`).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_absmax_partial(const float* __restrict__ x, int64_t n, float* __restrict__ partials) {
  __shared__ float sm[4];
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = fabsf(x[i]);
    m = (v <= 3.0e38f && v > m) ? v : m;        // (non-finite entries do not define the scale)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}
__global__ __launch_bounds__(256) void k_loss_grad_eff(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                                       const float* __restrict__ partials, int nPart,
                                                       const float* __restrict__ up, float* __restrict__ scale,
                                                       const int* __restrict__ guard) {
  __shared__ float sm[4];
  const float upv = up ? *up : 1.f;
  float f = upv;
  if (scale) {                                                        // uniform
    float m = threadIdx.x < nPart ? partials[threadIdx.x] : 0.f;      // nPart <= 256
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])) * fabsf(upv);
    int e = 0;
    if (m > 0.f && m <= 3.0e38f) { (void)frexpf(m, &e); e = 6 - e; }  // m = f * 2^e', f in [0.5, 1)  ->  m * 2^(6 - e') in [32, 64)
    if (guard) e -= guard[2];                                        // back-off after overflowed steps (k_guard_book)
    e = min(max(e, -60), 60);
    const float S = ldexpf(1.f, e);
    if (blockIdx.x == 0 && threadIdx.x == 0) { scale[0] = S; scale[1] = ldexpf(1.f, -e); }
    f = upv * S;                                                      // a power of two: no extra rounding
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = x[i] * f;
}
int launch_loss_grad_eff(const float* dlogits, float* out, int64_t n, const float* up_scale_dev, float* partials,
                         float* scale, hipStream_t s, const int* guard) {
  int g = 0;
  if (scale) {
    g = grid_for(n, 256 * 16, 256);
    hipLaunchKernelGGL(k_absmax_partial, dim3(g), dim3(256), 0, s, dlogits, n, partials);
    FU_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_loss_grad_eff, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, s, dlogits, out, n, partials, g,
                     up_scale_dev, scale, guard);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
