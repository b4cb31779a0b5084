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

// The windowed form (fu_stitch_add_batch_windowed): the ownership scheme of k_stitch_add_batch, and every covering job
// counts with w = win_y[ly] * win_x[lx] at its tile-local pixel (ly, lx) -- also in an edge-clipped box -- instead of 1.
// A kernel of its own: nothing here contracts (each product and each add rounds once, which is what a sequence of
// elementwise fp32 tensor ops gives), whereas k_stitch_add_batch<false> keeps its fma.  The logits source rounds
// e[k] * inv first, so it adds exactly what the probs source adds of fu_merge_views' single-view probabilities.
template <bool PROBS>
__global__ void k_stitch_add_batch_windowed(const StitchJob* __restrict__ jobs, int n, int ncls, int cropW,
                                            const float* __restrict__ win_y, const float* __restrict__ win_x) {
#pragma clang fp contract(off)
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
        const int ly = cy - Q.h0, lx = cx - Q.w0;
        const float w = win_y[ly] * win_x[lx];
        const float* z = Q.logits + ((int64_t)ly * cropW + lx) * ncls;
        float p[HEAD_MAX_CLS];
        if constexpr (PROBS) {
#pragma unroll
          for (int k = 0; k < HEAD_MAX_CLS; ++k) p[k] = k < ncls ? z[k] : 0.f;
        } else {
          float ex[HEAD_MAX_CLS], inv;
          softmax_terms(z, ncls, ex, inv);
#pragma unroll
          for (int k = 0; k < HEAD_MAX_CLS; ++k) p[k] = ex[k] * inv;
        }
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) {
          const float wp = w * p[k];
          acc[k] = acc[k] + wp;
        }
        wacc = wacc + w;
      }
#pragma unroll
      for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) J.canvas[o * ncls + k] = acc[k];
      J.weight[o] = wacc;
    }
  }
}

// Every check comes before the copy and the launch: a rejected call leaves the stream untouched.  win_y / win_x: null for
// the plain kernels; both given for the windowed one (H and W elements, the caller's).
int launch_stitch_add_batch(DeviceTable& table, const char* fn, const char* batch_name, int n, const fu_stitch_entry* entries,
                            const float* src, int n_samples, bool probs, int H, int W, int ncls, hipStream_t s,
                            const float* win_y, const float* win_x) {
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
  if (win_y) {
    if (probs) hipLaunchKernelGGL(k_stitch_add_batch_windowed<true>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W, win_y, win_x);
    else hipLaunchKernelGGL(k_stitch_add_batch_windowed<false>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W, win_y, win_x);
  } else if (probs) hipLaunchKernelGGL(k_stitch_add_batch<true>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W);
  else hipLaunchKernelGGL(k_stitch_add_batch<false>, grid, dim3(256), 0, s, jobs_dev, n, ncls, W);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Fused finalisation (fu_stitch_finalize_maps): one pass over a canvas gives the normalised canvas (k_stitch_finalize's
// expression, with the caller's eps), the uint8 class map, the uint8 probability bands, the uint8 top-2 margin and the
// pixels per argmax class.  Memory bound: a thread takes 4 consecutive pixels -- one float4 of weights, K float4 of
// canvas, one 4-byte store per uint8 map -- between a misaligned head and a tail that run one pixel at a time; an array
// that is not aligned alike (vec bit clear) is read or written one element at a time inside the groups too.
// MASKED (fu_stitch_finalize_maps_masked with a mask): one more byte per pixel, read 4 at a time where aligned; a pixel whose
// byte is 0 goes the uncovered pixel's way, except that its class byte is nodata_value.  The unmasked instantiations are
// the kernels they were.
// ------------------------------------------------------------------------------------------------
enum : unsigned { MAPS_VEC_CANVAS = 1, MAPS_VEC_CLASS = 2, MAPS_VEC_PROB = 4, MAPS_VEC_MARGIN = 8, MAPS_VEC_VALID = 16 };

struct FinalizeMaps {
  float* canvas;                   // [npix, K] raw sums
  const float* weight;             // [npix]
  unsigned char* class_out;        // [npix] or null
  unsigned char* prob_out;         // [K, npix] or null
  unsigned char* margin_out;       // [npix] or null
  unsigned long long* counts;      // [K] or null, added to
  int64_t npix, head;              // head: the pixels in front of weight's first 16-byte boundary
  unsigned long long class_values; // byte k = the class map's value for argmax k
  float eps;
  int normalize;                   // write the normalised canvas back
  unsigned vec;                    // MAPS_VEC_*: the array is aligned for the group's wide access
  int thr_cls;                     // fu_stitch_finalize_maps_ex: the thresholded class, -1 = the plain argmax
  float thr;
  const unsigned char* valid;      // MASKED: [npix], 0 = no data
  unsigned nodata_value;           // MASKED: the class map's byte of such a pixel
};

__device__ __forceinline__ unsigned char quantize_unit(float x) {
  return (unsigned char)rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.f);
}

// v: raw sums in, normalised values out.  am: argmax (first maximum wins), margin: v[top1] - v[top2] (v[0] for K == 1).
template <int K>
__device__ __forceinline__ bool finalize_pixel(float (&v)[K], float wgt, float eps, int& am, float& margin) {
#pragma clang fp contract(off)
  const float s = wgt + eps;
  const bool covered = s > 0.f;
  am = 0;
  margin = 0.f;
  if (!covered) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.f;
    return false;
  }
  const float inv = 1.f / s;
  float best = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = v[k] * inv;
    if (v[k] > best) { best = v[k]; am = k; }
  }
  if constexpr (K == 1) {
    margin = v[0];
  } else {
    float second = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) if (k != am) second = fmaxf(second, v[k]);
    margin = v[am] - second;
  }
  return true;
}

// The decided class of a covered pixel (fu_stitch_finalize_maps_ex): cls when v[cls] >= thr, otherwise the first maximum
// over the other classes; cls < 0: the argmax as it is.  K >= 2 whenever cls >= 0.
template <int K>
__device__ __forceinline__ int decide_class(const float (&v)[K], int am, int cls, float thr) {
  if (cls < 0) return am;
  float vc = 0.f, best = -INFINITY;
  int other = cls == 0 ? 1 : 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k == cls) vc = v[k];
    else if (v[k] > best) { best = v[k]; other = k; }
  }
  return vc >= thr ? cls : other;
}

// MASKED: a pixel without data -> the uncovered pixel's values; false: it is no pixel to count or to classify
template <int K>
__device__ __forceinline__ bool mask_pixel(bool has_data, bool covered, float (&v)[K], float& margin) {
  if (has_data) return covered;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.f;
  margin = 0.f;
  return false;
}

template <int K, bool MASKED>
__global__ __launch_bounds__(256) void k_stitch_finalize_maps(const FinalizeMaps a) {
  __shared__ unsigned int bins[HEAD_MAX_CLS];
  if (a.counts) {
    if (threadIdx.x < K) bins[threadIdx.x] = 0;
    __syncthreads();
  }
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = (a.npix - a.head) / 4;
  for (int64_t j = tid; j < nvec; j += nthr) {
    const int64_t p = a.head + 4 * j;
    const float4 w4 = *reinterpret_cast<const float4*>(a.weight + p);
    const float wq[4] = {w4.x, w4.y, w4.z, w4.w};
    float c[4 * K];
    if (a.vec & MAPS_VEC_CANVAS) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float4 t = reinterpret_cast<const float4*>(a.canvas + p * K)[i];
        c[4 * i] = t.x, c[4 * i + 1] = t.y, c[4 * i + 2] = t.z, c[4 * i + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4 * K; ++i) c[i] = a.canvas[p * K + i];
    }
    unsigned cls = 0, mg = 0, pq[K], vm = 0x01010101u;
    if constexpr (MASKED) {
      if (a.vec & MAPS_VEC_VALID) {
        vm = *reinterpret_cast<const unsigned*>(a.valid + p);
      } else {
        vm = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) vm |= (unsigned)a.valid[p + q] << (8 * q);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) pq[k] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[K], margin;
      int am;
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = c[q * K + k];
      bool covered = finalize_pixel<K>(v, wq[q], a.eps, am, margin);
      bool has_data = true;
      if constexpr (MASKED) {
        has_data = ((vm >> (8 * q)) & 0xffu) != 0u;
        covered = mask_pixel<K>(has_data, covered, v, margin);
      }
      if (covered) am = decide_class<K>(v, am, a.thr_cls, a.thr);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        c[q * K + k] = v[k];
        pq[k] |= (unsigned)quantize_unit(v[k]) << (8 * q);
      }
      cls |= (has_data ? (unsigned)(unsigned char)(a.class_values >> (8 * am)) : a.nodata_value) << (8 * q);
      mg |= (unsigned)quantize_unit(margin) << (8 * q);
      if (a.counts && covered) atomicAdd(&bins[am], 1u);
    }
    if (a.normalize) {
      if (a.vec & MAPS_VEC_CANVAS) {
#pragma unroll
        for (int i = 0; i < K; ++i)
          reinterpret_cast<float4*>(a.canvas + p * K)[i] = make_float4(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4 * K; ++i) a.canvas[p * K + i] = c[i];
      }
    }
    if (a.class_out) {
      if (a.vec & MAPS_VEC_CLASS) {
        *reinterpret_cast<unsigned*>(a.class_out + p) = cls;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.class_out[p + q] = (unsigned char)(cls >> (8 * q));
      }
    }
    if (a.margin_out) {
      if (a.vec & MAPS_VEC_MARGIN) {
        *reinterpret_cast<unsigned*>(a.margin_out + p) = mg;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.margin_out[p + q] = (unsigned char)(mg >> (8 * q));
      }
    }
    if (a.prob_out) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        unsigned char* dst = a.prob_out + (int64_t)k * a.npix + p;
        if (a.vec & MAPS_VEC_PROB) {
          *reinterpret_cast<unsigned*>(dst) = pq[k];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) dst[q] = (unsigned char)(pq[k] >> (8 * q));
        }
      }
    }
  }
  const int64_t tail0 = a.head + 4 * nvec, nrest = a.head + (a.npix - tail0);   // misaligned head and tail: plain code
  for (int64_t r = tid; r < nrest; r += nthr) {
    const int64_t p = r < a.head ? r : tail0 + (r - a.head);
    float v[K], margin;
    int am;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = a.canvas[p * K + k];
    bool covered = finalize_pixel<K>(v, a.weight[p], a.eps, am, margin);
    bool has_data = true;
    if constexpr (MASKED) {
      has_data = a.valid[p] != 0;
      covered = mask_pixel<K>(has_data, covered, v, margin);
    }
    if (covered) am = decide_class<K>(v, am, a.thr_cls, a.thr);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (a.normalize) a.canvas[p * K + k] = v[k];
      if (a.prob_out) a.prob_out[(int64_t)k * a.npix + p] = quantize_unit(v[k]);
    }
    if (a.class_out) a.class_out[p] = has_data ? (unsigned char)(a.class_values >> (8 * am)) : (unsigned char)a.nodata_value;
    if (a.margin_out) a.margin_out[p] = quantize_unit(margin);
    if (a.counts && covered) atomicAdd(&bins[am], 1u);
  }
  if (a.counts) {
    __syncthreads();
    if (threadIdx.x < K && bins[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
  }
}

int launch_stitch_finalize_maps(float* canvas, const float* weight, int ncls, int64_t npix, float eps, bool normalize,
                                const unsigned char* class_values, unsigned char* class_out, unsigned char* prob_out,
                                unsigned char* margin_out, int64_t* counts, const fu_class_threshold* thr, hipStream_t s,
                                const unsigned char* valid, int nodata_value) {
  if (npix <= 0) return 0;
  FinalizeMaps a{};
  a.valid = valid, a.nodata_value = valid ? (unsigned)nodata_value : 0u;
  a.thr_cls = thr ? thr->cls : -1, a.thr = thr ? thr->threshold : 0.f;
  a.canvas = canvas, a.weight = weight, a.class_out = class_out, a.prob_out = prob_out, a.margin_out = margin_out;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.npix = npix, a.eps = eps, a.normalize = normalize ? 1 : 0;
  for (int k = 0; k < HEAD_MAX_CLS; ++k)
    a.class_values |= (unsigned long long)(class_values && k < ncls ? class_values[k] : (unsigned char)k) << (8 * k);
  const uintptr_t wa = reinterpret_cast<uintptr_t>(weight);
  a.head = wa % 4 ? npix : std::min<int64_t>(npix, (int64_t)((16 - wa % 16) % 16) / 4);
  const auto aligned = [&](const void* base, int64_t elem_bytes, int64_t per_pixel, unsigned to) {
    return base && (reinterpret_cast<uintptr_t>(base) + (uintptr_t)(a.head * per_pixel * elem_bytes)) % to == 0;
  };
  if (aligned(canvas, 4, ncls, 16)) a.vec |= MAPS_VEC_CANVAS;
  if (aligned(class_out, 1, 1, 4)) a.vec |= MAPS_VEC_CLASS;
  if (aligned(margin_out, 1, 1, 4)) a.vec |= MAPS_VEC_MARGIN;
  if (aligned(valid, 1, 1, 4)) a.vec |= MAPS_VEC_VALID;
  if (aligned(prob_out, 1, 1, 4) && (ncls == 1 || npix % 4 == 0)) a.vec |= MAPS_VEC_PROB;   // every band alike
  const dim3 grid(grid_for(ceil_div64(npix, 4), 256, 2048));
  switch (ncls) {
#define FU_MAPS_CASE(K)                                                                               \
  case K:                                                                                             \
    if (valid) hipLaunchKernelGGL((k_stitch_finalize_maps<K, true>), grid, dim3(256), 0, s, a);       \
    else hipLaunchKernelGGL((k_stitch_finalize_maps<K, false>), grid, dim3(256), 0, s, a);            \
    break;
    FU_MAPS_CASE(1) FU_MAPS_CASE(2) FU_MAPS_CASE(3) FU_MAPS_CASE(4) FU_MAPS_CASE(5) FU_MAPS_CASE(6) FU_MAPS_CASE(7)
    FU_MAPS_CASE(8)
#undef FU_MAPS_CASE
    default: FU_REQUIRE(false, "stitch_finalize_maps: %d classes", ncls);
  }
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
// Probability histogram (fu_eval_prob_hist / fu_prob_hist): hist[c][t][bin(p[c])] and top[argmax == t][bin(p[argmax])] over
// the pixels k_eval_confusion counts, p = the softmax of the resident logits (e[c] * inv, the product rounded on its own:
// what fu_merge_views writes for one view of code 0) or the caller's probabilities.  Memory bound -- K floats and one
// int64 per pixel; a thread takes 4 consecutive pixels with K 16-byte loads between a misaligned head and a tail that go
// one pixel at a time (as k_stitch_finalize_maps) -- so what has to be kept off the critical path is LDS-atomic
// contention: flood scenes are saturated, whole waves of pixels fall into one (class, target, bin).  Two measures:
//   * the block keeps up to 4 histogram copies while they fit PROB_HIST_COPIES_BYTES (4 copies of 11 KB at K = 3, 256
//     bins) and wave w adds into copy w % copies, so at most 4 of the block's 16 waves ever meet on an address;
//   * inside a wave, wave_add elects a leader per round: the first pending lane broadcasts its key, the lanes that hold the
//     same key are found with one ballot, and the leader adds their number in ONE atomic.  Up to PROB_HIST_ROUNDS rounds,
//     stopping at the first group below PROB_HIST_GROUP_MIN lanes (diffuse data: one wasted single-lane atomic per
//     class); the lanes still pending then add 1 each, to mostly distinct addresses.
// Bins are unsigned int in LDS (the grid keeps a block's share of pixels below 2^32); the flush sums the copies and adds
// the non-zero bins with 64-bit integer atomics, as ConfusionBins::flush: exact, order-free, no finalisation pass.
// ------------------------------------------------------------------------------------------------
// 16 waves per block: the grid is capped at one block per CU (the flush below costs a block up to (K * K + 2) * n_bins
// global atomics, so blocks are few), and a CU needs that many waves to keep its share of the loads in flight
static constexpr int PROB_HIST_BLOCK = 1024, PROB_HIST_ROUNDS = 4, PROB_HIST_GROUP_MIN = 4;
static constexpr int PROB_HIST_COPIES_BYTES = 64 * 1024;   // more than one copy only while they fit this much LDS

struct ProbHist {
  const float* src;               // [npix, K] logits (LOGITS) or probabilities
  const int64_t* target;          // [npix]
  unsigned long long* hist;       // [K][K][n_bins] or null, added to
  unsigned long long* top;        // [2][n_bins] or null, added to
  int64_t npix, head;             // head: the pixels in front of src's first 16-byte boundary (npix: no wide loads at all)
  int ignore_index, n_bins, copies;
};

// the bin rule of include/floodunet.h: s = p * n_bins is exact for a power of two; NaN and p < 1 / n_bins go to bin 0
__device__ __forceinline__ int prob_bin(float p, int n_bins) {
  const float s = p * (float)n_bins;
  return s >= 1.f ? (s >= (float)n_bins ? n_bins - 1 : (int)s) : 0;
}

// row[key] += 1 for every lane with `valid`, lanes of one key pre-aggregated (see above).  Called by whole waves: the
// loops around it have wave-uniform trip counts.
__device__ __forceinline__ void wave_add(unsigned int* row, int key, bool valid) {
  unsigned long long todo = __ballot(valid);
  const int lane = (int)(threadIdx.x & 63);
  for (int r = 0; r < PROB_HIST_ROUNDS && todo; ++r) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int lk = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long same = __ballot(valid && key == lk) & todo;
    const int n = __popcll(same);
    if (lane == leader) atomicAdd(&row[lk], (unsigned int)n);
    todo &= ~same;
    if (n < PROB_HIST_GROUP_MIN) break;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&row[key], 1u);
}

// one pixel per lane: z = its K logits or probabilities, t = its target (anything invalid for a lane without a pixel)
template <int K, bool LOGITS>
__device__ __forceinline__ void prob_hist_pixel(unsigned int* bins, const float (&z)[K], int64_t t, const ProbHist& a) {
#pragma clang fp contract(off)
  const bool valid = t != (int64_t)a.ignore_index && t >= 0 && t < K;
  float p[K];
  if constexpr (LOGITS) {
    float e[HEAD_MAX_CLS], inv;
    softmax_terms(z, K, e, inv);
#pragma unroll
    for (int c = 0; c < K; ++c) p[c] = e[c] * inv;
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c) p[c] = z[c];
  }
  const int nb = a.n_bins, tt = valid ? (int)t : 0;
  if (a.hist) {
#pragma unroll
    for (int c = 0; c < K; ++c) wave_add(bins + c * K * nb, tt * nb + prob_bin(p[c], nb), valid);
  }
  if (a.top) {
    float pm = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) if (p[c] > pm) { pm = p[c]; am = c; }
    wave_add(bins + K * K * nb, (am == tt ? nb : 0) + prob_bin(pm, nb), valid);
  }
}

template <int K, bool LOGITS>
__global__ __launch_bounds__(PROB_HIST_BLOCK) void k_prob_hist(const ProbHist a) {
  extern __shared__ unsigned int prob_hist_lds[];
  const int per = (K * K + 2) * a.n_bins;
  for (int i = threadIdx.x; i < per * a.copies; i += PROB_HIST_BLOCK) prob_hist_lds[i] = 0;
  __syncthreads();
  unsigned int* bins = prob_hist_lds + (int)((threadIdx.x >> 6) % (unsigned)a.copies) * per;
  const int64_t nthr = (int64_t)gridDim.x * PROB_HIST_BLOCK;
  const int64_t nvec = (a.npix - a.head) / 4;
  for (int64_t j0 = (int64_t)blockIdx.x * PROB_HIST_BLOCK; j0 < nvec; j0 += nthr) {   // uniform trips: wave_add ballots
    const int64_t j = j0 + threadIdx.x;
    const bool in = j < nvec;
    float c[4 * K];
    int64_t t[4];
    if (in) {
      const int64_t p = a.head + 4 * j;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float4 v = reinterpret_cast<const float4*>(a.src + p * K)[i];
        c[4 * i] = v.x, c[4 * i + 1] = v.y, c[4 * i + 2] = v.z, c[4 * i + 3] = v.w;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = a.target[p + q];
    } else {
#pragma unroll
      for (int i = 0; i < 4 * K; ++i) c[i] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = -1;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float z[K];
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = c[q * K + k];
      prob_hist_pixel<K, LOGITS>(bins, z, t[q], a);
    }
  }
  const int64_t tail0 = a.head + 4 * nvec, nrest = a.head + (a.npix - tail0);   // misaligned head and tail: plain code
  for (int64_t r0 = (int64_t)blockIdx.x * PROB_HIST_BLOCK; r0 < nrest; r0 += nthr) {
    const int64_t r = r0 + threadIdx.x;
    float z[K];
    int64_t t = -1;
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = 0.f;
    if (r < nrest) {
      const int64_t p = r < a.head ? r : tail0 + (r - a.head);
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = a.src[p * K + k];
      t = a.target[p];
    }
    prob_hist_pixel<K, LOGITS>(bins, z, t, a);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < per; i += PROB_HIST_BLOCK) {
    unsigned long long n = 0;
    for (int cp = 0; cp < a.copies; ++cp) n += prob_hist_lds[cp * per + i];
    if (!n) continue;
    const int ih = K * K * a.n_bins;
    if (i < ih) {
      if (a.hist) atomicAdd(&a.hist[i], n);
    } else if (a.top) {
      atomicAdd(&a.top[i - ih], n);
    }
  }
}

// fu_eval_prob_hist (logits == true: src = the resident NHWC logits) and fu_prob_hist: every check comes before anything
// is launched, so a rejected call leaves the outputs untouched
int launch_prob_hist(const char* fn, const float* src, bool logits, const int64_t* target, int64_t npix, int ncls,
                     int ignore_index, int n_bins, int64_t* hist, int64_t* top, hipStream_t s) {
  FU_REQUIRE(src && target, "%s: null %s / target", fn, logits ? "logits" : "probs");
  FU_REQUIRE(hist || top, "%s: nothing to write (hist_out and top_out are both null)", fn);
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "%s: n_classes %d not in 1..%d", fn, ncls, HEAD_MAX_CLS);
  FU_REQUIRE(n_bins >= 2 && n_bins <= 1024 && (n_bins & (n_bins - 1)) == 0, "%s: n_bins %d is not a power of two in 2..1024",
             fn, n_bins);
  FU_REQUIRE(npix >= 1, "%s: n_pixels %lld < 1", fn, (long long)npix);
  const int64_t copy_bytes = (int64_t)(ncls * ncls + 2) * n_bins * 4;
  FU_REQUIRE(copy_bytes <= FU_PROB_HIST_LDS_BYTES, "%s: %d classes x %d bins need %lld bytes of LDS, more than the %d reserved",
             fn, ncls, n_bins, (long long)copy_bytes, FU_PROB_HIST_LDS_BYTES);
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src);
  FU_REQUIRE(sa % 4 == 0 && reinterpret_cast<uintptr_t>(target) % 8 == 0, "%s: misaligned %s / target", fn,
             logits ? "logits" : "probs");
  ProbHist a{};
  a.src = src, a.target = target, a.npix = npix, a.ignore_index = ignore_index, a.n_bins = n_bins;
  a.hist = reinterpret_cast<unsigned long long*>(hist), a.top = reinterpret_cast<unsigned long long*>(top);
  a.head = npix;   // the first pixel at a 16-byte boundary, if the stride of ncls floats ever reaches one
  for (int h = 0; h < 4; ++h)
    if ((sa + (uintptr_t)h * ncls * 4) % 16 == 0) { a.head = std::min<int64_t>(npix, h); break; }
  a.copies = 4 * copy_bytes <= PROB_HIST_COPIES_BYTES ? 4 : 2 * copy_bytes <= PROB_HIST_COPIES_BYTES ? 2 : 1;
  const size_t lds = (size_t)(a.copies * copy_bytes);
  // one block per CU at most (the flush costs a block up to (k * k + 2) * n_bins global atomics), and enough blocks
  // that a block's share of pixels -- the most one unsigned int bin can receive -- stays below 2^32
  const int grid = (int)std::max<int64_t>(grid_for(ceil_div64(npix, 4), PROB_HIST_BLOCK, 256), ceil_div64(npix, (int64_t)1 << 31));
  const void* fn_ptr = nullptr;
  switch (ncls) {
#define FU_HIST_CASE(K) case K: fn_ptr = logits ? (const void*)k_prob_hist<K, true> : (const void*)k_prob_hist<K, false>; break;
    FU_HIST_CASE(1) FU_HIST_CASE(2) FU_HIST_CASE(3) FU_HIST_CASE(4) FU_HIST_CASE(5) FU_HIST_CASE(6) FU_HIST_CASE(7)
    FU_HIST_CASE(8)
#undef FU_HIST_CASE
  }
  if (lds > 64 * 1024) {   // one copy above the default dynamic-LDS window: the device must have it, and the kernel opts in
    int dev = 0, have = 0;
    FU_REQUIRE(hipGetDevice(&dev) == hipSuccess &&
               hipDeviceGetAttribute(&have, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && (size_t)have >= lds,
               "%s: %d classes x %d bins need %zu bytes of LDS, the device offers %d per block", fn, ncls, n_bins, lds, have);
    FU_REQUIRE(hipFuncSetAttribute(fn_ptr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
               "%s: the device refuses %zu bytes of dynamic LDS", fn, lds);
  }
  switch (ncls) {
#define FU_HIST_CASE(K)                                                                                              \
  case K:                                                                                                            \
    if (logits) hipLaunchKernelGGL((k_prob_hist<K, true>), dim3(grid), dim3(PROB_HIST_BLOCK), lds, s, a);            \
    else hipLaunchKernelGGL((k_prob_hist<K, false>), dim3(grid), dim3(PROB_HIST_BLOCK), lds, s, a);                  \
    break;
    FU_HIST_CASE(1) FU_HIST_CASE(2) FU_HIST_CASE(3) FU_HIST_CASE(4) FU_HIST_CASE(5) FU_HIST_CASE(6) FU_HIST_CASE(7)
    FU_HIST_CASE(8)
#undef FU_HIST_CASE
  }
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
