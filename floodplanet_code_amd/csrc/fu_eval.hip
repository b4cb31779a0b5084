// Evaluation-side kernels (gfx950): what turns the resident logits of a forward pass into scene outputs and metrics --
// overlap-averaging stitching (one crop or a table of crops), per-sample confusion counts, the test-time-augmentation
// merge.  None of them runs inside a training step.
#include "../../include/floodunet.h"
#include "fu_common.h"

#include <algorithm>
#include <vector>

namespace fu {

// exp(z[k] - max z) for k < ncls (0 above) and 1 / their sum: the softmax of a pixel's logits is e[k] * inv.  The callers
// write that product inside their own accumulate statement (it contracts to one fma there), and all of them go through
// this one expression, which is what keeps fu_stitch_add, fu_stitch_add_batch and fu_merge_views bit-identical.
__device__ __forceinline__ void softmax_terms(const float* z, int ncls, float (&e)[HEAD_MAX_CLS], float& inv) {
  float m = -INFINITY, se = 0.f;
#pragma unroll
  for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) m = fmaxf(m, z[k]);
#pragma unroll
  for (int k = 0; k < HEAD_MAX_CLS; ++k) { e[k] = k < ncls ? expf(z[k] - m) : 0.f; se += e[k]; }
  inv = 1.f / se;
}

// A block's confusion histogram in LDS (bins[t * ncls + p], atomicAdd by the block's threads between zero and flush);
// flush adds the non-zero bins to the caller's counts with 64-bit integer atomics: exact and order-free, so there is no
// finalisation pass.
struct ConfusionBins {
  unsigned int bins[HEAD_MAX_CLS * HEAD_MAX_CLS];
  __device__ __forceinline__ void zero(int ncls) {
    for (int i = threadIdx.x; i < ncls * ncls; i += blockDim.x) bins[i] = 0;
    __syncthreads();
  }
  __device__ __forceinline__ void flush(int ncls, unsigned long long* out) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncls * ncls; i += blockDim.x)
      if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
  }
};

// ------------------------------------------------------------------------------------------------
// Inference stitching (utils/utils_image.py:410-494, predict.py:329-347): softmax of a crop's logits is added into an
// overlap-averaging canvas, canvas[h0:hE, w0:wE, :] += p[:dh, :dw, :], weight += 1; finalisation divides by
// (weight + 1e-5) and emits the argmax map.
// ------------------------------------------------------------------------------------------------
__global__ void k_stitch_add(const float* __restrict__ logits_nhwc, int ncls, int cropW, float* __restrict__ canvas,
                             float* __restrict__ weight, int canvasW, int h0, int w0, int dh, int dw) {
  const int64_t total = (int64_t)dh * dw;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % dw), y = (int)(idx / dw);
    const float* z = logits_nhwc + ((int64_t)y * cropW + x) * ncls;
    float e[HEAD_MAX_CLS], inv;
    softmax_terms(z, ncls, e, inv);
    const int64_t o = (int64_t)(h0 + y) * canvasW + (w0 + x);
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) canvas[o * ncls + k] += e[k] * inv;
    weight[o] += 1.f;
  }
}

__global__ void k_stitch_finalize(float* __restrict__ canvas, const float* __restrict__ weight, int ncls,
                                  int64_t npix, int64_t* __restrict__ argmax_out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float inv = 1.f / (weight[p] + 1e-5f);
    float best = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) {
      if (k < ncls) {
        const float v = canvas[p * ncls + k] * inv;
        canvas[p * ncls + k] = v;
        if (v > best) { best = v; am = k; }
      }
    }
    if (argmax_out) argmax_out[p] = am;
  }
}

int launch_stitch_add(const float* logits_nhwc, int ncls, int cropW, float* canvas, float* weight, int canvasW, int h0,
                      int w0, int dh, int dw, hipStream_t s) {
  hipLaunchKernelGGL(k_stitch_add, dim3(grid_for((int64_t)dh * dw, 256, 2048)), dim3(256), 0, s, logits_nhwc, ncls,
                     cropW, canvas, weight, canvasW, h0, w0, dh, dw);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_stitch_finalize(float* canvas, const float* weight, int ncls, int64_t npix, int64_t* argmax_out,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_stitch_finalize, dim3(grid_for(npix, 256, 2048)), dim3(256), 0, s, canvas, weight, ncls, npix,
                     argmax_out);
  FU_LAUNCH_CHECK();
  return 0;
}

// Batched stitching: jobs[0..n-1] in one launch, bit-identical to k_stitch_add for each job in table order.  A canvas
// pixel belongs to the first job that covers it; that thread reads the canvas once, adds the softmax of every covering
// job in table order with the very expression of k_stitch_add (same rounding sequence), and writes once -- overlapping
// crops of one batch (stride < crop) never race and need no float atomics.  blockIdx.y walks the jobs, blockIdx.x the
// pixels of the job's box; the ownership scan over earlier jobs is uniform across the block (scalar loads of the table).
struct StitchJob {         // one crop of the table (device copy of a validated fu_stitch_entry)
  const float* logits;     // NHWC fp32 logits of the crop's sample (the tile's [0, 0] pixel), or its probabilities
  float* canvas;
  float* weight;
  int canvasW, h0, w0, dh, dw, pad;
};

__device__ __forceinline__ bool stitch_covers(const StitchJob& J, const float* canvas, int cy, int cx) {
  return J.canvas == canvas && cy >= J.h0 && cy < J.h0 + J.dh && cx >= J.w0 && cx < J.w0 + J.dw;
}

// PROBS (fu_stitch_add_batch_probs): Q.logits points at the job's [H, W, k] fp32 probabilities, which are added as they
// are instead of a softmax of logits.
template <bool PROBS>
__global__ void k_stitch_add_batch(const StitchJob* __restrict__ jobs, int n, int ncls, int cropW) {
  for (int e = blockIdx.y; e < n; e += gridDim.y) {
    const StitchJob J = jobs[e];
    const int64_t total = (int64_t)J.dh * J.dw;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
      const int cy = J.h0 + (int)(idx / J.dw), cx = J.w0 + (int)(idx % J.dw);
      bool owner = true;
      for (int j = 0; j < e && owner; ++j) owner = !stitch_covers(jobs[j], J.canvas, cy, cx);
      if (!owner) continue;
      const int64_t o = (int64_t)cy * J.canvasW + cx;
      float acc[HEAD_MAX_CLS], wacc = J.weight[o];
#pragma unroll
      for (int k = 0; k < HEAD_MAX_CLS; ++k) acc[k] = k < ncls ? J.canvas[o * ncls + k] : 0.f;
      for (int j = e; j < n; ++j) {
        const StitchJob Q = jobs[j];
        if (!stitch_covers(Q, J.canvas, cy, cx)) continue;
        const float* z = Q.logits + ((int64_t)(cy - Q.h0) * cropW + (cx - Q.w0)) * ncls;
        if constexpr (PROBS) {
#pragma unroll
          for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) acc[k] += z[k];
        } else {
          float ex[HEAD_MAX_CLS], inv;
          softmax_terms(z, ncls, ex, inv);
#pragma unroll
          for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) acc[k] += ex[k] * inv;
        }
        wacc += 1.f;
      }
#pragma unroll
      for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) J.canvas[o * ncls + k] = acc[k];
      J.weight[o] = wacc;
    }
  }
}

// Every check comes before the copy and the launch: a rejected call leaves the stream untouched.
int launch_stitch_add_batch(DeviceTable& table, const char* fn, const char* batch_name, int n, const fu_stitch_entry* entries,
                            const float* src, int n_samples, bool probs, int H, int W, int ncls, hipStream_t s) {
  std::vector<StitchJob> jobs((size_t)n);
  int max_area = 0;
  for (int i = 0; i < n; ++i) {
    const fu_stitch_entry& E = entries[i];
    const int dh = E.hE - E.h0, dw = E.wE - E.w0;
    FU_REQUIRE(E.canvas && E.weight, "%s: entry %d: null canvas / weight", fn, i);
    FU_REQUIRE(E.sample >= 0 && E.sample < n_samples, "%s: entry %d: sample %d not in the %s (%d)", fn, i, E.sample,
               batch_name, n_samples);
    FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && dh > 0 && dw > 0 && E.hE <= E.canvas_h && E.wE <= E.canvas_w && dh <= H && dw <= W,
               "%s: entry %d: crop [%d:%d, %d:%d] is empty or does not fit canvas %dx%d / tile %dx%d", fn, i,
               E.h0, E.hE, E.w0, E.wE, E.canvas_h, E.canvas_w, H, W);
    for (int j = 0; j < i; ++j) {   // one thread owns a canvas pixel: canvases must not share a weight or disagree in size
      const fu_stitch_entry& P = entries[j];
      FU_REQUIRE((P.canvas == E.canvas) == (P.weight == E.weight) &&
                 (P.canvas != E.canvas || (P.canvas_h == E.canvas_h && P.canvas_w == E.canvas_w)),
                 "%s: entries %d and %d share a canvas or a weight but not both (or differ in size)", fn, j, i);
    }
    jobs[i] = StitchJob{src + (int64_t)E.sample * H * W * ncls, E.canvas, E.weight, E.canvas_w, E.h0, E.w0, dh, dw, 0};
    max_area = std::max(max_area, dh * dw);
  }
  FU_TRY(table.upload(jobs.data(), (size_t)n * sizeof(StitchJob), sizeof(StitchJob), s));
  const StitchJob* jobs_dev = static_cast<const StitchJob*>(table.dev);
  const dim3 grid(grid_for(max_area, 256, 1024), n < 65535 ? n : 65535);
  if (probs) hipLaunchKernelGGL(k_stitch_add_batch<true>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W);
  else hipLaunchKernelGGL(k_stitch_add_batch<false>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Per-sample confusion counts of the resident logits (prediction metrics, predict.py:236-250): the argmax and pixel rule
// of k_ce_loss without the loss.  blockIdx.y = sample; a block histograms its pixels in LDS, then adds the non-zero bins
// to counts[b][t * k + p] with 64-bit integer atomics (exact, order-free), so there is no finalisation pass.
// ------------------------------------------------------------------------------------------------
__global__ void k_eval_confusion(const float* __restrict__ logits, const int64_t* __restrict__ target, int ncls,
                                 int ignore_index, int64_t hw, unsigned long long* __restrict__ counts) {
  __shared__ ConfusionBins hist;
  hist.zero(ncls);
  const int64_t base = (int64_t)blockIdx.y * hw;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < hw; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = base + q;
    const int64_t t = target[p];
    if (t == (int64_t)ignore_index || t < 0 || t >= ncls) continue;
    float m = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) {
      if (k < ncls) {
        const float z = logits[p * ncls + k];
        if (z > m) { m = z; am = k; }
      }
    }
    atomicAdd(&hist.bins[(int)t * ncls + am], 1u);
  }
  hist.flush(ncls, counts + (int64_t)blockIdx.y * ncls * ncls);
}

int launch_eval_confusion(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int B, int64_t hw,
                          int64_t* counts, hipStream_t s) {
  const dim3 grid(grid_for(hw, 256, 64), B);
  hipLaunchKernelGGL(k_eval_confusion, grid, dim3(256), 0, s, logits_nhwc, target, ncls, ignore_index, hw,
                     reinterpret_cast<unsigned long long*>(counts));
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Test-time augmentation merge (fu_merge_views): P_b = (sum over views v, in view order, of inverse view codes[v] of
// softmax(logits of sample v * B + b)) / T, fp32 NHWC [B, H, W, k].  One thread per (crop, pixel): it reads the k logits
// at the pixel's place in each view (view_dst_pixel), takes the softmax with the expression of k_stitch_add_batch and
// keeps the sum in registers.  Blocks cover 16 x 16 pixel tiles, so a transposing view reads a 16 x 16 tile of its
// logits too (whole 16-pixel row segments per block, not one pixel per row).  With counts, argmax P (first maximum wins)
// is histogrammed against the target as in k_eval_confusion: LDS bins, then 64-bit integer atomics.
// ------------------------------------------------------------------------------------------------
static constexpr int MERGE_TILE = 16;

__global__ __launch_bounds__(MERGE_TILE * MERGE_TILE) void k_merge_views(
    const float* __restrict__ logits, int H, int W, int ncls, int B, int T, unsigned codes, float* __restrict__ probs,
    const int64_t* __restrict__ target, int ignore_index, unsigned long long* __restrict__ counts) {
  __shared__ ConfusionBins hist;
  if (counts) hist.zero(ncls);
  const int b = blockIdx.z;
  const int x = blockIdx.x * MERGE_TILE + (int)(threadIdx.x % MERGE_TILE);
  const int y = blockIdx.y * MERGE_TILE + (int)(threadIdx.x / MERGE_TILE);
  const int64_t hw = (int64_t)H * W;
  if (y < H && x < W) {
    float acc[HEAD_MAX_CLS];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) acc[k] = 0.f;
    for (int v = 0; v < T; ++v) {
      const int q = view_dst_pixel((codes >> (3 * v)) & 7, y, x, H, W);
      const float* z = logits + (((int64_t)v * B + b) * hw + q) * ncls;
      float ex[HEAD_MAX_CLS], inv;
      softmax_terms(z, ncls, ex, inv);
#pragma unroll
      for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) acc[k] += ex[k] * inv;
    }
    const int64_t p = (int64_t)b * hw + (int64_t)y * W + x;
    const float fT = (float)T;
    float pm = -INFINITY;
    int am = 0;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) {
      if (k < ncls) {
        const float pk = acc[k] / fT;
        if (probs) probs[p * ncls + k] = pk;
        if (pk > pm) { pm = pk; am = k; }
      }
    }
    if (counts) {
      const int64_t t = target[p];
      if (t != (int64_t)ignore_index && t >= 0 && t < ncls) atomicAdd(&hist.bins[(int)t * ncls + am], 1u);
    }
  }
  if (counts) hist.flush(ncls, counts + (int64_t)b * ncls * ncls);
}

int launch_merge_views(const float* logits_nhwc, int H, int W, int ncls, int B, int n_views, unsigned codes, float* probs,
                       const int64_t* target, int ignore_index, int64_t* counts, hipStream_t s) {
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS && B >= 1 && B <= 65535 && n_views >= 1 && n_views <= 8,
             "merge_views: bad geometry (classes %d, batch %d, views %d)", ncls, B, n_views);
  const dim3 grid((unsigned)ceil_div(W, MERGE_TILE), (unsigned)ceil_div(H, MERGE_TILE), (unsigned)B);
  hipLaunchKernelGGL(k_merge_views, grid, dim3(MERGE_TILE * MERGE_TILE), 0, s, logits_nhwc, H, W, ncls, B, n_views, codes,
                     probs, target, ignore_index, reinterpret_cast<unsigned long long*>(counts));
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
