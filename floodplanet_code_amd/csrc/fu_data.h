// What more than one of the data-preparation files (fu_data.hip, fu_scene_train.hip, fu_band_stats.hip) needs: the rotation's
// index arithmetic, how a (sample, channel) plane is addressed, the per-tile statistics and the normalisation they feed, and
// the argument checks the assembling entry points share; private to csrc.
#pragma once
#include "../../include/floodunet.h"
#include "fu_common.h"

#include <math.h>

namespace fu {

// torchvision F.rotate -> affine_grid + grid_sample(nearest, align_corners=False).  Index arithmetic: bit-exact with
// oracle/unet_oracle.py:augment -- the same fp32 operations in the same order, each rounded on its own (no fma
// contraction), cos / sin evaluated in double and rounded once to float, round-half-even.
__device__ __forceinline__ void rotation_of(float angle_deg, float& cs, float& sn) {
#pragma clang fp contract(off)
  const float th = angle_deg * 0.017453292519943295f;
  cs = (float)cos((double)th);
  sn = (float)sin((double)th);
}
// the source pixel of output (ox, oy) under that rotation; false: it lies outside the tile
__device__ __forceinline__ bool rotate_source(int ox, int oy, float cs, float sn, int H, int W, int& sx, int& sy) {
#pragma clang fp contract(off)
  const float xc = ((float)ox + 0.5f) - 0.5f * (float)W, yc = ((float)oy + 0.5f) - 0.5f * (float)H;
  const float px = cs * xc, qx = sn * yc, py = sn * xc, qy = cs * yc;
  const float xs = ((px - qx) + 0.5f * (float)W) - 0.5f;
  const float ys = ((py + qy) + 0.5f * (float)H) - 0.5f;
  sx = (int)nearbyintf(xs);
  sy = (int)nearbyintf(ys);
  return sx >= 0 && sx < W && sy >= 0 && sy < H;
}

// How k_tile_stats / k_assemble_tiles address the (sample, channel) planes they read: the plane's first valid pixel, its
// row stride and the sample's valid crop size.  Both kernels are instantiated once per form, so fu_scene_crops runs the
// very arithmetic of fu_assemble_tiles (same values, same order) and equals cut-then-assemble bit for bit.
struct BatchPlanes {        // fu_assemble_tiles: sample b of the SrcList batch, crop in the top-left corner of the tile
  SrcList S;
  int H, W;
  const int* vh;
  const int* vw;
  __device__ __forceinline__ const float* plane(int b, int c) const {
    int si = 0;
    for (int k = 1; k < S.n; ++k) si = c >= S.coff[k] ? k : si;
    return S.p[si] + ((int64_t)b * S.c[si] + (c - S.coff[si])) * H * W;
  }
  __device__ __forceinline__ int64_t stride(int) const { return W; }
  // (the crop sizes come from device memory: clamp, an oversized or negative entry must not read past the plane)
  __device__ __forceinline__ int valid_h(int b) const { return vh ? min(max(vh[b], 0), H) : H; }
  __device__ __forceinline__ int valid_w(int b) const { return vw ? min(max(vw[b], 0), W) : W; }
};

struct SceneCropJob {       // one box of the table (device copy of a validated fu_scene_crop / fu_scene_train_entry)
  const float* scene;       // fp32 [C, scene_h, scene_w]
  int scene_h, scene_w, h0, w0, dh, dw;
};

struct ScenePlanes {        // fu_scene_crops: box b of a resident scene [C, scene_h, scene_w] (boxes validated on the host)
  const SceneCropJob* __restrict__ jobs;
  __device__ __forceinline__ const float* plane(int b, int c) const {
    const SceneCropJob& J = jobs[b];
    return J.scene + ((int64_t)c * J.scene_h + J.h0) * J.scene_w + J.w0;
  }
  __device__ __forceinline__ int64_t stride(int b) const { return jobs[b].scene_w; }
  __device__ __forceinline__ int valid_h(int b) const { return jobs[b].dh; }
  __device__ __forceinline__ int valid_w(int b) const { return jobs[b].dw; }
};

// one block per (sample, channel): mean and POPULATION std (numpy .mean / .std, ddof = 0) over the valid crop, two passes
// (the plane stays in L2), fp64 accumulation, fixed-order block reduction
template <class Planes>
__global__ __launch_bounds__(256) void k_tile_stats(Planes P, int Ctot, float* __restrict__ mean_o,
                                                    float* __restrict__ std_o) {
  __shared__ double sm[256];
  const int b = blockIdx.x / Ctot, c = blockIdx.x - b * Ctot;
  const float* plane = P.plane(b, c);
  const int64_t st = P.stride(b);
  const int h = P.valid_h(b), w = P.valid_w(b);
  const int n = h * w;
  auto block_sum = [&](double v) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
      __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
  };
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)plane[(i / w) * st + (i % w)];
  const double mean = n > 0 ? block_sum(a) / n : 0.0;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { const double dlt = (double)plane[(i / w) * st + (i % w)] - mean; q += dlt * dlt; }
  const double var = n > 0 ? block_sum(q) / n : 1.0;
  if (threadIdx.x == 0) { mean_o[blockIdx.x] = (float)mean; std_o[blockIdx.x] = (float)sqrt(var); }
}

// What the assembling kernels normalise with: null = not at all, else (x - mean[i]) / stdv[i], i per (sample, channel)
// or per channel.
struct NormParams { const float* mean = nullptr; const float* stdv = nullptr; int per_sample = 0; };

// norm_mode -> NormParams: 1 ('local') launches k_tile_stats into mean_out / std_out and normalises with those, 2
// ('global') takes the caller's per-channel parameters, 0 none.  The callers have checked the arguments (check_norm_mode).
template <class Planes>
int resolve_norm(const Planes& P, int B, int Ctot, int norm_mode, const float* gmean, const float* gstd, float* mean_out,
                 float* std_out, hipStream_t s, NormParams& N) {
  N = NormParams{};
  if (norm_mode == 1) {
    hipLaunchKernelGGL(k_tile_stats<Planes>, dim3(B * Ctot), dim3(256), 0, s, P, Ctot, mean_out, std_out);
    FU_LAUNCH_CHECK();
    N = NormParams{mean_out, std_out, 1};
  } else if (norm_mode == 2) {
    N = NormParams{gmean, gstd, 0};
  }
  return 0;
}

// The argument checks the three assembling entry points share.  fn: the prefix of the messages; stats_shape: the shape
// of mean_out / std_out as that entry point names it.
static int check_norm_mode(const char* fn, const char* stats_shape, int norm_mode, const float* gmean, const float* gstd,
                           const float* mean_out, const float* std_out) {
  FU_REQUIRE(norm_mode >= 0 && norm_mode <= 2, "%s: norm_mode must be 0 (None), 1 ('local') or 2 ('global'), got %d", fn,
             norm_mode);
  FU_REQUIRE(norm_mode != 1 || (mean_out && std_out), "%s: norm_mode 'local' needs mean_out / std_out %s", fn, stats_shape);
  FU_REQUIRE(norm_mode != 2 || (gmean && gstd), "%s: norm_mode 'global' needs the per-channel parameters", fn);
  return 0;
}

// The checks fu_scene_crops and fu_scene_train_tiles[_ex] share for entry i (E: fu_scene_crop or fu_scene_train_entry) -> its
// job.  zoom (fu_scene_train_tiles_ex with out sizes): the box is resampled onto out_h x out_w of the tile, so the box may
// exceed the tile and the out size may not.
template <class Entry>
static int check_scene_box(const char* fn, int i, const Entry& E, int tile_h, int tile_w, SceneCropJob& job,
                           bool zoom = false, int out_h = 0, int out_w = 0) {
  const int dh = E.hE - E.h0, dw = E.wE - E.w0;
  FU_REQUIRE(E.scene, "%s: entry %d: null scene", fn, i);
  FU_REQUIRE(E.scene_h >= 1 && E.scene_w >= 1, "%s: entry %d: bad scene size %dx%d", fn, i, E.scene_h, E.scene_w);
  FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && E.hE <= E.scene_h && E.wE <= E.scene_w,
             "%s: entry %d: box [%d:%d, %d:%d] lies outside its scene %dx%d", fn, i, E.h0, E.hE, E.w0, E.wE, E.scene_h,
             E.scene_w);
  FU_REQUIRE(dh >= 1 && dw >= 1, "%s: entry %d: box [%d:%d, %d:%d] is empty", fn, i, E.h0, E.hE, E.w0, E.wE);
  FU_REQUIRE(zoom || (dh <= tile_h && dw <= tile_w), "%s: entry %d: box %dx%d is larger than the tile %dx%d", fn, i, dh, dw,
             tile_h, tile_w);
  FU_REQUIRE(!zoom || (int64_t)dh * dw <= INT32_MAX, "%s: entry %d: box %dx%d is too large", fn, i, dh, dw);
  FU_REQUIRE(!zoom || (out_h >= 1 && out_h <= tile_h && out_w >= 1 && out_w <= tile_w),
             "%s: entry %d: out size %dx%d must lie within 1x1 and the tile %dx%d", fn, i, out_h, out_w, tile_h, tile_w);
  job = SceneCropJob{E.scene, E.scene_h, E.scene_w, E.h0, E.w0, dh, dw};
  return 0;
}

}  // namespace fu
