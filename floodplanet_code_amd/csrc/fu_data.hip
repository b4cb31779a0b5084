// Data-preparation kernels (gfx950): what turns rasters that are already in HBM into batches, tile by tile -- tile
// augmentation, tile assembly and scene crops, Lanczos-4 resampling.  None of them runs inside a training step.  fu_scene_crops,
// which takes a table of host entries, is validated here, next to the kernels that trust the table.  Training tiles from
// resident scenes and the label counts are in fu_scene_train.hip, the band statistics in fu_band_stats.hip; fu_data.h holds
// what they share with this file.
#include "fu_data.h"

#include <vector>

namespace fu {

// ------------------------------------------------------------------------------------------------
// On-GPU tile augmentation (datasets/base_dataset.py:494-555): per sample hflip -> vflip -> rotate(angle) with
// torchvision's tensor semantics (nearest, expand=False, centre = image centre, zero fill), applied identically to
// the image [B,C,H,W] fp32 and the target [B,H,W] int64.  One gather pass: the three transforms are composed into a
// single source coordinate per output pixel.
// ------------------------------------------------------------------------------------------------
__global__ void k_augment(const float* __restrict__ img, const int64_t* __restrict__ tgt, float* __restrict__ img_o,
                          int64_t* __restrict__ tgt_o, const int* __restrict__ flags, const float* __restrict__ angle,
                          int C, int H, int W, int64_t target_fill, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(idx % W);
    const int64_t r = idx / W;
    const int oy = (int)(r % H);
    const int b = (int)(r / H);
    const int f = flags[b];
    int sx = ox, sy = oy;
    bool inside = true;
    if (f & 4) {
      float cs, sn;
      rotation_of(angle[b], cs, sn);
      inside = rotate_source(ox, oy, cs, sn, H, W, sx, sy);
    }
    if (f & 2) sy = H - 1 - sy;   // the rotate input is the v-flipped, h-flipped tile
    if (f & 1) sx = W - 1 - sx;
    if (tgt_o) tgt_o[idx] = inside ? tgt[((int64_t)b * H + sy) * W + sx] : target_fill;
    for (int c = 0; c < C; ++c) {
      const int64_t o = (((int64_t)b * C + c) * H + oy) * W + ox;
      img_o[o] = inside ? img[(((int64_t)b * C + c) * H + sy) * W + sx] : 0.f;
    }
  }
}

int launch_augment(const float* img, const int64_t* tgt, float* img_o, int64_t* tgt_o, const int* flags,
                   const float* angle, int B, int C, int H, int W, int64_t target_fill, hipStream_t s) {
  const int64_t total = (int64_t)B * H * W;
  hipLaunchKernelGGL(k_augment, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, img, tgt, img_o, tgt_o, flags, angle,
                     C, H, W, target_fill, total);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Tile assembly: per-tile normalisation (base_dataset.py:77-113), edge-crop buffer
// (base_dataset.py:271-325) and multi-sensor channel concatenation (ef_model.py:28-44 / stacked sensors) of a whole batch
// that is already in HBM, instead of per item in DataLoader workers.
// ------------------------------------------------------------------------------------------------

// out[b][c][y][x] = inside the valid crop ? (src - mean[b][c]) / std[b][c] : pad_value
template <class Planes>
__global__ void k_assemble_tiles(Planes P, int Ctot, int H, int W, const float* __restrict__ mean,
                                 const float* __restrict__ stdv, int per_sample, float pad_value, float* __restrict__ out,
                                 int64_t total) {
#pragma clang fp contract(off)      // image -= mean; image /= std: two roundings, as numpy does them
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % W);
    int64_t r = idx / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % Ctot);
    const int b = (int)(r / Ctot);
    const bool inside = y < P.valid_h(b) && x < P.valid_w(b);
    float v = pad_value;
    if (inside) {
      v = P.plane(b, c)[y * P.stride(b) + x];
      if (mean) {
        const int mi = per_sample ? b * Ctot + c : c;
        const float d = v - mean[mi];
        v = d / stdv[mi];
      }
    }
    out[idx] = v;
  }
}

template <class Planes>
int launch_tiles(const Planes& P, int B, int Ctot, int H, int W, int norm_mode, const float* gmean, const float* gstd,
                 float pad_value, float* out, float* mean_out, float* std_out, hipStream_t s) {
  NormParams N;
  FU_TRY(resolve_norm(P, B, Ctot, norm_mode, gmean, gstd, mean_out, std_out, s, N));
  const int64_t total = (int64_t)B * Ctot * H * W;
  hipLaunchKernelGGL(k_assemble_tiles<Planes>, dim3(grid_for(total, 256)), dim3(256), 0, s, P, Ctot, H, W, N.mean, N.stdv,
                     N.per_sample, pad_value, out, total);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// Lanczos-4 resampling of a batch of tiles (round 4).  The reference resamples the WHOLE raster to the
// label raster's size for every item it loads (floodplanet.py:338-340 -> utils_image.py:11-54, cv2.INTER_LANCZOS4) and then cuts
// the tile out.  Lanczos is local: tile rows [Y0, Y0 + TH) of the resampled raster depend on a window of ~TH * scale + 8 source
// rows, so the host ships that window and two 8-tap tables per tile axis (index into the window, weight) and the device computes
//     out[b][c][y][x] = sum_kx wx[b][x][kx] * ( sum_ky wy[b][y][ky] * win[b][c][iy[b][y][ky]][ix[b][x][kx]] )
// in fp32 with the taps accumulated in order and multiply / add rounded separately -- the arithmetic of the numpy restatement
// (datasets/resize.py: rows first, then columns), so the tile equals the crop of the host's whole-raster result bit for bit.
// scale_mode = the sensor scaling that follows the crop in the reference (floodplanet.py:347 / :406 / :467 / :525).
// One thread per output pixel; the window (a few KB per tile and band) is served from L2.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_resize_lanczos4_tiles(const float* __restrict__ win, int C, int win_h, int win_w,
                                                               const int* __restrict__ iy, const float* __restrict__ wy,
                                                               const int* __restrict__ ix, const float* __restrict__ wx,
                                                               int TH, int TW, int scale_mode, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int bc = blockIdx.z, b = bc / C;
  if (x >= TW || y >= TH) return;
  const float* w = win + (size_t)bc * win_h * win_w;
  const int* iyb = iy + ((size_t)b * TH + y) * 8;
  const float* wyb = wy + ((size_t)b * TH + y) * 8;
  const int* ixb = ix + ((size_t)b * TW + x) * 8;
  const float* wxb = wx + ((size_t)b * TW + x) * 8;
  int ry[8], cx[8];
  float fy[8], fx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { ry[k] = iyb[k] * win_w; fy[k] = wyb[k]; cx[k] = ixb[k]; fx[k] = wxb[k]; }
  float o = 0.f;
#pragma unroll
  for (int kx = 0; kx < 8; ++kx) {
    float t = 0.f;
#pragma unroll
    for (int ky = 0; ky < 8; ++ky) {
      const float p = fy[ky] * w[ry[ky] + cx[kx]];      // (two roundings: numpy multiplies, then adds)
      t = t + p;
    }
    const float q = fx[kx] * t;
    o = o + q;
  }
  if (scale_mode == 1) o = fminf(fmaxf((o + 50.f) / 100.f, 0.f), 1.f);            // S1 (dB): clip((x + 50) / 100, 0, 1), NaN -> 0
  else if (scale_mode == 2) o = fminf(fmaxf(o / 4096.f, 0.f), 1.f);                // S2: clip(x / 2^12, 0, 1)
  else if (scale_mode == 3) o = fminf(fmaxf(o, 0.f), 18607.72f) / 18607.72f;       // L8: clip(x, 0, 18607.72) / 18607.72
  else if (scale_mode == 4) o = o / 65536.f;                                       // PS stored as uint16: x / 2^16
  out[((size_t)bc * TH + y) * TW + x] = o;
}

int launch_resize_lanczos4_tiles(const float* win, int B, int C, int win_h, int win_w, const int* iy, const float* wy,
                                 const int* ix, const float* wx, int TH, int TW, int scale_mode, float* out, hipStream_t s) {
  FU_REQUIRE((int64_t)B * C <= 65535 && TH >= 1 && TW >= 1 && win_h >= 1 && win_w >= 1, "resize_lanczos4_tiles: bad shape");
  // grid.y walks the output rows 4 at a time, and the kernel indexes a window plane with 32-bit offsets
  FU_REQUIRE(ceil_div(TH, 4) <= 65535 && (int64_t)win_h * win_w <= INT32_MAX,
             "resize_lanczos4_tiles: tile of %d rows or window %dx%d too large for one launch", TH, win_h, win_w);
  FU_REQUIRE(scale_mode >= 0 && scale_mode <= 4, "resize_lanczos4_tiles: scale_mode %d", scale_mode);
  hipLaunchKernelGGL(k_resize_lanczos4_tiles, dim3(ceil_div(TW, 64), ceil_div(TH, 4), B * C), dim3(256), 0, s, win, C, win_h,
                     win_w, iy, wy, ix, wx, TH, TW, scale_mode, out);
  FU_LAUNCH_CHECK();
  return 0;
}

int launch_assemble_tiles(const float* const* srcs, const int* src_channels, int n_src, int B, int H, int W, const int* vh,
                          const int* vw, int norm_mode, const float* gmean, const float* gstd, float pad_value, float* out,
                          float* mean_out, float* std_out, hipStream_t s) {
  FU_REQUIRE(n_src >= 1 && n_src <= 8, "assemble: 1..8 sources (got %d)", n_src);
  BatchPlanes P;
  P.S.n = n_src;
  int off = 0;
  for (int k = 0; k < n_src; ++k) {
    FU_REQUIRE(srcs[k] && src_channels[k] >= 1, "assemble: bad source %d", k);
    P.S.p[k] = srcs[k]; P.S.c[k] = src_channels[k]; P.S.coff[k] = off; off += src_channels[k];
  }
  P.S.coff[n_src] = off;
  P.H = H; P.W = W; P.vh = vh; P.vw = vw;
  FU_TRY(check_norm_mode("assemble", "[B, sum C]", norm_mode, gmean, gstd, mean_out, std_out));
  return launch_tiles(P, B, off, H, W, norm_mode, gmean, gstd, pad_value, out, mean_out, std_out, s);
}

// every check before anything is launched or copied: a rejected call leaves the stream untouched
int launch_scene_crops(DeviceTable& table, int n, const fu_scene_crop* entries, int C, int H, int W, int norm_mode,
                       const float* gmean, const float* gstd, float pad_value, float* out, float* mean_out, float* std_out,
                       hipStream_t s) {
  FU_REQUIRE(n >= 1 && C >= 1 && H >= 1 && W >= 1, "fu_scene_crops: n = %d, C = %d, tile %dx%d (all must be >= 1)", n, C, H, W);
  FU_TRY(check_norm_mode("fu_scene_crops", "[n, C]", norm_mode, gmean, gstd, mean_out, std_out));
  FU_REQUIRE((int64_t)n * C <= INT32_MAX && (int64_t)n * C * H * W <= ((int64_t)1 << 40),
             "fu_scene_crops: %d boxes of %d channels are too many for one call", n, C);
  std::vector<SceneCropJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i) FU_TRY(check_scene_box("fu_scene_crops", i, entries[i], H, W, jobs[i]));
  FU_TRY(table.upload(jobs.data(), (size_t)n * sizeof(SceneCropJob), sizeof(SceneCropJob), s));
  ScenePlanes P;
  P.jobs = static_cast<const SceneCropJob*>(table.dev);
  return launch_tiles(P, n, C, H, W, norm_mode, gmean, gstd, pad_value, out, mean_out, std_out, s);
}

}  // namespace fu
