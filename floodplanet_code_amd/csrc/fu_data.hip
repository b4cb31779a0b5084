// Data-preparation kernels (gfx950): what turns rasters that are already in HBM into training and inference batches --
// tile augmentation, tile assembly and scene crops, Lanczos-4 resampling, training tiles straight from resident scenes,
// label class counts, streaming band statistics.  None of them runs inside a training step.  The entry points that take a
// table of host entries (fu_scene_crops, fu_scene_train_tiles[_ex], fu_label_class_counts, fu_label_box_counts) are validated
// here, next to the kernels that trust the table.
#include "../../include/floodunet.h"
#include "fu_common.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace fu {

// ------------------------------------------------------------------------------------------------
// On-GPU tile augmentation (datasets/base_dataset.py:494-555): per sample hflip -> vflip -> rotate(angle) with
// torchvision's tensor semantics (nearest, expand=False, centre = image centre, zero fill), applied identically to
// the image [B,C,H,W] fp32 and the target [B,H,W] int64.  One gather pass: the three transforms are composed into a
// single source coordinate per output pixel.
// ------------------------------------------------------------------------------------------------
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

// The checks fu_scene_crops and fu_scene_train_tiles share for entry i (E: fu_scene_crop or fu_scene_train_entry) -> its job.
template <class Entry>
static int check_scene_box(const char* fn, int i, const Entry& E, int tile_h, int tile_w, SceneCropJob& job) {
  const int dh = E.hE - E.h0, dw = E.wE - E.w0;
  FU_REQUIRE(E.scene, "%s: entry %d: null scene", fn, i);
  FU_REQUIRE(E.scene_h >= 1 && E.scene_w >= 1, "%s: entry %d: bad scene size %dx%d", fn, i, E.scene_h, E.scene_w);
  FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && E.hE <= E.scene_h && E.wE <= E.scene_w,
             "%s: entry %d: box [%d:%d, %d:%d] lies outside its scene %dx%d", fn, i, E.h0, E.hE, E.w0, E.wE, E.scene_h,
             E.scene_w);
  FU_REQUIRE(dh >= 1 && dw >= 1, "%s: entry %d: box [%d:%d, %d:%d] is empty", fn, i, E.h0, E.hE, E.w0, E.wE);
  FU_REQUIRE(dh <= tile_h && dw <= tile_w, "%s: entry %d: box %dx%d is larger than the tile %dx%d", fn, i, dh, dw, tile_h,
             tile_w);
  job = SceneCropJob{E.scene, E.scene_h, E.scene_w, E.h0, E.w0, dh, dw};
  return 0;
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

// ------------------------------------------------------------------------------------------------
// Training batches straight from resident scenes (fu_scene_train_tiles): k_assemble_tiles<ScenePlanes> composed with
// k_augment, and the label decode of FloodplanetTiles._load_label_image, in one pass -- no crop batch is written to HBM
// and read back.  A block owns one plane (sample b, channel c -- or the sample's target plane) and a run of its pixels;
// a thread owns PX consecutive pixels of a row at a time and walks the plane, so its stores and those of its wave are
// contiguous along x (PX = 4: one 16-byte store per image quad, two per int64 target quad; PX = 1 when tile_w % 4 != 0).
// The flags are uniform per block: samples without the rotate flag take the row copy / reversal loop (16-byte loads too
// where the source quad is aligned), the others the gather loop with sin / cos evaluated once per thread.  Same fp32
// operations in the same order as the two kernels it replaces, so the outputs are the same bits.
// ------------------------------------------------------------------------------------------------
struct SceneTrainAug {     // what box b of the table carries besides its SceneCropJob
  const uint8_t* label;    // the scene's raw label raster, uint8 [scene_h, scene_w], or nullptr (no target)
  int flags;               // FU_AUG_*
  float angle;             // degrees
};

// (x - mean) / std as k_assemble_tiles rounds it: two operations, two roundings
__device__ __forceinline__ float normalise(float v, bool norm, float m, float sd) {
#pragma clang fp contract(off)
  if (norm) {
    const float d = v - m;
    v = d / sd;
  }
  return v;
}

// raw label value -> class (floodplanet.py:586-596): 2 flood -> 1, 0 no data -> nodata_value, anything else -> 0
// The one statement of "raw label byte -> category": 0 = neither 0 nor 2 (decodes to class 0), 1 = raw 2 (decodes to class
// 1), 2 = raw 0 (no data).  decode_label and both label-count kernels go through it.
__device__ __forceinline__ int label_category(uint8_t raw) { return raw == 2 ? 1 : (raw == 0 ? 2 : 0); }
__device__ __forceinline__ int64_t decode_label(uint8_t raw, int64_t nodata_value) {
  const int k = label_category(raw);
  return k == 2 ? nodata_value : (int64_t)k;
}

template <int PX>
__device__ __forceinline__ void store_px(float* __restrict__ o, const float (&v)[PX]) {
  if constexpr (PX == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  else o[0] = v[0];
}
template <int PX>
__device__ __forceinline__ void store_px(int64_t* __restrict__ o, const int64_t (&v)[PX]) {
  if constexpr (PX == 4) {
    reinterpret_cast<longlong2*>(o)[0] = make_longlong2(v[0], v[1]);
    reinterpret_cast<longlong2*>(o)[1] = make_longlong2(v[2], v[3]);
  } else {
    o[0] = v[0];
  }
}

static constexpr int STT_RUNS = 4;     // pixel runs of PX per thread: a block covers 256 * STT_RUNS * PX pixels of its plane

template <int PX>
__global__ __launch_bounds__(256) void k_scene_train_tiles(const SceneCropJob* __restrict__ jobs,
                                                           const SceneTrainAug* __restrict__ augs, int C, int H, int W,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           int per_sample, float pad_value, int64_t nodata_value,
                                                           int64_t target_fill, float* __restrict__ img_o,
                                                           int64_t* __restrict__ tgt_o) {
  const int planes = C + (tgt_o ? 1 : 0);
  const int b = blockIdx.x / planes, p = blockIdx.x - b * planes;
  const SceneCropJob J = jobs[b];
  const SceneTrainAug A = augs[b];
  const int QW = W / PX, nq = H * QW;        // PX = 4 only where W % 4 == 0
  const int q0 = blockIdx.y * (256 * STT_RUNS);
  const int q1 = min(q0 + 256 * STT_RUNS, nq);
  const bool is_target = p == C;
  const bool hf = A.flags & 1, vf = A.flags & 2;
  // the plane this block reads, from the box's first pixel, and the plane it writes
  const int64_t box = (int64_t)J.h0 * J.scene_w + J.w0;
  const float* __restrict__ src = J.scene + (int64_t)(is_target ? 0 : p) * J.scene_h * J.scene_w + box;
  const uint8_t* __restrict__ lab = A.label ? A.label + box : nullptr;
  float* __restrict__ io = img_o + ((int64_t)b * C + (is_target ? 0 : p)) * H * W;
  int64_t* __restrict__ to = tgt_o ? tgt_o + (int64_t)b * H * W : nullptr;
  const bool norm = mean != nullptr;
  float m = 0.f, sd = 1.f;
  if (norm && !is_target) {
    const int mi = per_sample ? b * C + p : p;
    m = mean[mi];
    sd = stdv[mi];
  }

  if (A.flags & 4) {                          // gather: every pixel has its own source
    float cs, sn;
    rotation_of(A.angle, cs, sn);
    for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
      const int oy = q / QW, x0 = (q - oy * QW) * PX;
      int sx[PX], sy[PX];
      bool in_tile[PX], in_box[PX];
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        in_tile[j] = rotate_source(x0 + j, oy, cs, sn, H, W, sx[j], sy[j]);
        if (vf) sy[j] = H - 1 - sy[j];        // the rotate input is the v-flipped, h-flipped tile
        if (hf) sx[j] = W - 1 - sx[j];
        in_box[j] = in_tile[j] && sy[j] < J.dh && sx[j] < J.dw;
      }
      if (is_target) {
        int64_t v[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j)
          v[j] = in_box[j] ? decode_label(lab[(int64_t)sy[j] * J.scene_w + sx[j]], nodata_value) : target_fill;
        store_px<PX>(to + (int64_t)oy * W + x0, v);
      } else {
        float v[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j)
          v[j] = in_box[j] ? normalise(src[(int64_t)sy[j] * J.scene_w + sx[j]], norm, m, sd)
                           : (in_tile[j] ? pad_value : 0.f);
        store_px<PX>(io + (int64_t)oy * W + x0, v);
      }
    }
    return;
  }

  // no rotation: output row oy is source row oy (or its mirror), copied or reversed
  for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
    const int oy = q / QW, x0 = (q - oy * QW) * PX;
    const int sy = vf ? H - 1 - oy : oy;
    const int lo = hf ? W - PX - x0 : x0;     // source x of the run's lowest address; output j reads lo + (PX - 1 - j) if hf
    const bool row_in = sy < J.dh;
    const int64_t off = (int64_t)sy * J.scene_w + lo;
    if (is_target) {
      int64_t s[PX], v[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) s[k] = row_in && lo + k < J.dw ? decode_label(lab[off + k], nodata_value) : target_fill;
#pragma unroll
      for (int j = 0; j < PX; ++j) v[j] = hf ? s[PX - 1 - j] : s[j];
      store_px<PX>(to + (int64_t)oy * W + x0, v);
    } else {
      float s[PX], v[PX];
      bool wide = false;
      if constexpr (PX == 4) {
        wide = row_in && lo + 3 < J.dw && (reinterpret_cast<uintptr_t>(src + off) & 15) == 0;
        if (wide) {
          const float4 t = *reinterpret_cast<const float4*>(src + off);
          s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
#pragma unroll
          for (int k = 0; k < 4; ++k) s[k] = normalise(s[k], norm, m, sd);
        }
      }
      if (!wide) {
#pragma unroll
        for (int k = 0; k < PX; ++k) s[k] = row_in && lo + k < J.dw ? normalise(src[off + k], norm, m, sd) : pad_value;
      }
#pragma unroll
      for (int j = 0; j < PX; ++j) v[j] = hf ? s[PX - 1 - j] : s[j];
      store_px<PX>(io + (int64_t)oy * W + x0, v);
    }
  }
}

// every check before anything is launched or copied: a rejected call leaves the stream untouched
int launch_scene_train_tiles(DeviceTable& table, int n, const fu_scene_train_entry* entries, int C, int H, int W,
                             int norm_mode, const float* gmean, const float* gstd, float pad_value, int64_t nodata_value,
                             int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out, float* std_out,
                             hipStream_t s) {
  const char* fn = "fu_scene_train_tiles";
  FU_REQUIRE(n >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: n = %d, C = %d, tile %dx%d (all must be >= 1)", fn, n, C, H, W);
  FU_TRY(check_norm_mode(fn, "[n, C]", norm_mode, gmean, gstd, mean_out, std_out));
  // fu_scene_crops' bounds, with the target plane counted; the kernel's grid.y walks a plane 1024 pixel runs at a time, so
  // 2^25 pixels (32768 rows of blocks with one pixel per run) stay inside the 65535 a launch accepts
  FU_REQUIRE((int64_t)n * (C + 1) <= INT32_MAX && (int64_t)n * C * H * W <= ((int64_t)1 << 40) &&
             (int64_t)H * W <= ((int64_t)1 << 25),
             "%s: %d boxes of %d channels, tile %dx%d, are too many for one call", fn, n, C, H, W);
  // one table: the boxes, then the transforms
  const size_t crop_bytes = (size_t)n * sizeof(SceneCropJob);
  std::vector<unsigned char> host(crop_bytes + (size_t)n * sizeof(SceneTrainAug));
  SceneCropJob* jobs = reinterpret_cast<SceneCropJob*>(host.data());
  SceneTrainAug* augs = reinterpret_cast<SceneTrainAug*>(host.data() + crop_bytes);
  for (int i = 0; i < n; ++i) {
    const fu_scene_train_entry& E = entries[i];
    FU_TRY(check_scene_box(fn, i, E, H, W, jobs[i]));
    FU_REQUIRE(!target_out || E.label, "%s: entry %d: target_out given but the entry has no label", fn, i);
    FU_REQUIRE((E.flags & ~(FU_AUG_HFLIP | FU_AUG_VFLIP | FU_AUG_ROTATE)) == 0, "%s: entry %d: unknown flag bits 0x%x", fn, i,
               (unsigned)E.flags);
    FU_REQUIRE(std::isfinite(E.angle_deg), "%s: entry %d: the angle is not finite", fn, i);
    augs[i] = SceneTrainAug{E.label, E.flags, E.angle_deg};
  }
  FU_TRY(table.upload(host.data(), host.size(), sizeof(SceneCropJob) + sizeof(SceneTrainAug), s));
  const SceneCropJob* jobs_dev = static_cast<const SceneCropJob*>(table.dev);
  const SceneTrainAug* augs_dev = reinterpret_cast<const SceneTrainAug*>(static_cast<const unsigned char*>(table.dev) + crop_bytes);
  ScenePlanes P;
  P.jobs = jobs_dev;
  NormParams N;                               // 'local': the statistics of the un-augmented crop, fu_scene_crops' own kernel
  FU_TRY(resolve_norm(P, n, C, norm_mode, gmean, gstd, mean_out, std_out, s, N));
  const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(image_out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(target_out) & 15) == 0;
  const int64_t nq = (int64_t)H * (vec ? W / 4 : W);
  const dim3 grid((unsigned)(n * (C + (target_out ? 1 : 0))), (unsigned)ceil_div64(nq, (int64_t)256 * STT_RUNS));
  if (vec)
    hipLaunchKernelGGL(k_scene_train_tiles<4>, grid, dim3(256), 0, s, jobs_dev, augs_dev, C, H, W, N.mean, N.stdv,
                       N.per_sample, pad_value, nodata_value, target_fill, image_out, target_out);
  else
    hipLaunchKernelGGL(k_scene_train_tiles<1>, grid, dim3(256), 0, s, jobs_dev, augs_dev, C, H, W, N.mean, N.stdv,
                       N.per_sample, pad_value, nodata_value, target_fill, image_out, target_out);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The same pass with radiometric and zoom augmentation (fu_scene_train_tiles_ex; include/floodunet.h states the arithmetic).
// A sibling of k_scene_train_tiles, which stays as it is: with zoom every pixel has its own source in any case, so this
// kernel has one loop -- per output pixel the flips and the rotation yield an integer pixel of the un-augmented tile, ZOOM
// maps it into the box (four taps served from L2, x first, then y; labels nearest-exact), the value is normalised, and
// PHOTO applies gain, bias and sigma * z.  The same plane / run decomposition, so the stores are the same 16-byte stores.
// z comes from Philox4x32-10 keyed by the OUTPUT pixel, the channel and the sample's stream: 40 32-bit integer multiplies
// per value, independent of every load, and no transcendental.  Without ZOOM and PHOTO this kernel is not instantiated.
// ------------------------------------------------------------------------------------------------
struct SceneAugEx {        // what box b carries for this kernel besides its SceneCropJob and SceneTrainAug
  int out_h, out_w;        // ZOOM: the region of the tile the box is resampled onto (else unused)
  uint32_t stream_lo, stream_hi;
};

struct ScenePhoto {        // device [n * C] each, null = that term is skipped
  const float* gain;
  const float* bias;
  const float* sigma;
  uint32_t key_lo, key_hi;
  float k;                 // (float)(1 / sqrt(32 * (65536^2 - 1) / 12)): 2 * S - 524280 has that variance's inverse
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// the unit-variance draw of (output pixel, channel, stream): |2 * S - 524280| < 2^24, so the convert is exact
__device__ __forceinline__ float unit_noise(uint32_t pixel, uint32_t channel, uint32_t stream_lo, uint32_t stream_hi,
                                            const ScenePhoto& T) {
  uint32_t o[4];
  philox4x32_10(pixel, channel, stream_lo, stream_hi, T.key_lo, T.key_hi, o);
  int S = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) S += (int)(o[i] & 0xffffu) + (int)(o[i] >> 16);
  return (float)(2 * S - 524280) * T.k;
}

// one axis of the zoom: pixel i of `out` -> the two taps and the weight of the bilinear image, the index of the label
__device__ __forceinline__ void zoom_axis(int i, int src, int out, int& i0, int& i1, float& w, int& nearest) {
#pragma clang fp contract(off)
  const float scale = (float)src / (float)out;
  const float c = ((float)i + 0.5f) * scale;
  const float f = fmaxf(c - 0.5f, 0.f);
  i0 = min((int)floorf(f), src - 1);
  i1 = min(i0 + 1, src - 1);
  w = f - (float)i0;
  nearest = min((int)floorf(c), src - 1);
}

__device__ __forceinline__ float lerp_sep(float p, float q, float w) {
#pragma clang fp contract(off)
  const float d = q - p;
  const float e = w * d;
  return p + e;
}

template <int PX, bool ZOOM, bool PHOTO>
__global__ __launch_bounds__(256) void k_scene_train_tiles_aug(const SceneCropJob* __restrict__ jobs,
                                                               const SceneTrainAug* __restrict__ augs,
                                                               const SceneAugEx* __restrict__ exs, ScenePhoto T, int C, int H,
                                                               int W, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, int per_sample,
                                                               float pad_value, int64_t nodata_value, int64_t target_fill,
                                                               float* __restrict__ img_o, int64_t* __restrict__ tgt_o) {
#pragma clang fp contract(off)
  const int planes = C + (tgt_o ? 1 : 0);
  const int b = blockIdx.x / planes, p = blockIdx.x - b * planes;
  const SceneCropJob J = jobs[b];
  const SceneTrainAug A = augs[b];
  const SceneAugEx X = exs[b];
  const int QW = W / PX, nq = H * QW;        // PX = 4 only where W % 4 == 0
  const int q0 = blockIdx.y * (256 * STT_RUNS);
  const int q1 = min(q0 + 256 * STT_RUNS, nq);
  const bool is_target = p == C;
  const bool hf = A.flags & 1, vf = A.flags & 2, rot = A.flags & 4;
  const int64_t box = (int64_t)J.h0 * J.scene_w + J.w0;
  const float* __restrict__ src = J.scene + (int64_t)(is_target ? 0 : p) * J.scene_h * J.scene_w + box;
  const uint8_t* __restrict__ lab = A.label ? A.label + box : nullptr;
  float* __restrict__ io = img_o + ((int64_t)b * C + (is_target ? 0 : p)) * H * W;
  int64_t* __restrict__ to = tgt_o ? tgt_o + (int64_t)b * H * W : nullptr;
  const int vh = ZOOM ? X.out_h : J.dh, vw = ZOOM ? X.out_w : J.dw;      // the valid region of the un-augmented tile
  const bool norm = mean != nullptr;
  float m = 0.f, sd = 1.f, gain = 1.f, bias = 0.f, sigma = 0.f;
  if (!is_target) {
    if (norm) {
      const int mi = per_sample ? b * C + p : p;
      m = mean[mi];
      sd = stdv[mi];
    }
    if (PHOTO) {
      const int gi = b * C + p;
      if (T.gain) gain = T.gain[gi];
      if (T.bias) bias = T.bias[gi];
      if (T.sigma) sigma = T.sigma[gi];
    }
  }
  float cs = 1.f, sn = 0.f;
  if (rot) rotation_of(A.angle, cs, sn);

  for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
    const int oy = q / QW, x0 = (q - oy * QW) * PX;
    float fv[PX];
    int64_t tv[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int ox = x0 + j;
      int sx = ox, sy = oy;
      bool in_tile = true;
      if (rot) in_tile = rotate_source(ox, oy, cs, sn, H, W, sx, sy);
      if (vf) sy = H - 1 - sy;                // the rotate input is the v-flipped, h-flipped tile
      if (hf) sx = W - 1 - sx;
      const bool in_box = in_tile && sy < vh && sx < vw;
      if (is_target) {
        int64_t v = target_fill;
        if (in_box) {
          int ly = sy, lx = sx;
          if (ZOOM) {
            int a0, a1; float w;
            zoom_axis(sy, J.dh, X.out_h, a0, a1, w, ly);
            zoom_axis(sx, J.dw, X.out_w, a0, a1, w, lx);
          }
          v = decode_label(lab[(int64_t)ly * J.scene_w + lx], nodata_value);
        }
        tv[j] = v;
      } else {
        float v = in_tile ? pad_value : 0.f;
        if (in_box) {
          if (ZOOM) {
            int y0, y1, x0s, x1s, nn;
            float wy, wx;
            zoom_axis(sy, J.dh, X.out_h, y0, y1, wy, nn);
            zoom_axis(sx, J.dw, X.out_w, x0s, x1s, wx, nn);
            const float* __restrict__ r0 = src + (int64_t)y0 * J.scene_w;
            const float* __restrict__ r1 = src + (int64_t)y1 * J.scene_w;
            const float top = lerp_sep(r0[x0s], r0[x1s], wx);
            const float bot = lerp_sep(r1[x0s], r1[x1s], wx);
            v = lerp_sep(top, bot, wy);
          } else {
            v = src[(int64_t)sy * J.scene_w + sx];
          }
          v = normalise(v, norm, m, sd);
          if (PHOTO) {
            if (T.gain) v = v * gain;
            if (T.bias) v = v + bias;
            if (T.sigma) {
              const float z = unit_noise((uint32_t)(oy * W + ox), (uint32_t)p, X.stream_lo, X.stream_hi, T);
              const float e = sigma * z;
              v = v + e;
            }
          }
        }
        fv[j] = v;
      }
    }
    if (is_target) store_px<PX>(to + (int64_t)oy * W + x0, tv);
    else store_px<PX>(io + (int64_t)oy * W + x0, fv);
  }
}

// every check before anything is launched or copied: a rejected call leaves the stream untouched
int launch_scene_train_tiles_ex(DeviceTable& table, int n, const fu_scene_train_entry* entries, int C, int H, int W,
                                int norm_mode, const float* gmean, const float* gstd, float pad_value, int64_t nodata_value,
                                int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out, float* std_out,
                                const fu_scene_aug* aug, hipStream_t s) {
  const char* fn = "fu_scene_train_tiles_ex";
  const bool photo = aug && (aug->gain || aug->bias || aug->sigma);
  const bool zoom = aug && (aug->out_h || aug->out_w);
  if (!photo && !zoom)                        // nothing switched on: the plain call, its kernel and its bits
    return launch_scene_train_tiles(table, n, entries, C, H, W, norm_mode, gmean, gstd, pad_value, nodata_value,
                                    target_fill, image_out, target_out, mean_out, std_out, s);
  FU_REQUIRE(n >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: n = %d, C = %d, tile %dx%d (all must be >= 1)", fn, n, C, H, W);
  FU_TRY(check_norm_mode(fn, "[n, C]", norm_mode, gmean, gstd, mean_out, std_out));
  FU_REQUIRE((int64_t)n * (C + 1) <= INT32_MAX && (int64_t)n * C * H * W <= ((int64_t)1 << 40) &&
             (int64_t)H * W <= ((int64_t)1 << 25),
             "%s: %d boxes of %d channels, tile %dx%d, are too many for one call", fn, n, C, H, W);
  FU_REQUIRE(!zoom || (aug->out_h && aug->out_w), "%s: out_h and out_w go together", fn);
  FU_REQUIRE(!(aug->sigma) || aug->noise_stream, "%s: sigma needs noise_stream", fn);
  const size_t nc = (size_t)n * (size_t)C;
  for (size_t i = 0; i < nc; ++i) {
    FU_REQUIRE(!aug->gain || std::isfinite(aug->gain[i]), "%s: gain[%zu] is not finite", fn, i);
    FU_REQUIRE(!aug->bias || std::isfinite(aug->bias[i]), "%s: bias[%zu] is not finite", fn, i);
    FU_REQUIRE(!aug->sigma || (std::isfinite(aug->sigma[i]) && aug->sigma[i] >= 0.f),
               "%s: sigma[%zu] = %g must be finite and >= 0", fn, i, aug->sigma ? (double)aug->sigma[i] : 0.0);
  }
  // one table: the boxes, the transforms, the per-sample extras, then the per-(sample, channel) terms that are given
  const size_t crop_bytes = (size_t)n * sizeof(SceneCropJob), aug_bytes = (size_t)n * sizeof(SceneTrainAug);
  const size_t ex_bytes = (size_t)n * sizeof(SceneAugEx), term_bytes = nc * sizeof(float);
  const int n_terms = (aug->gain ? 1 : 0) + (aug->bias ? 1 : 0) + (aug->sigma ? 1 : 0);
  std::vector<unsigned char> host(crop_bytes + aug_bytes + ex_bytes + (size_t)n_terms * term_bytes);
  SceneCropJob* jobs = reinterpret_cast<SceneCropJob*>(host.data());
  SceneTrainAug* augs = reinterpret_cast<SceneTrainAug*>(host.data() + crop_bytes);
  SceneAugEx* exs = reinterpret_cast<SceneAugEx*>(host.data() + crop_bytes + aug_bytes);
  for (int i = 0; i < n; ++i) {
    const fu_scene_train_entry& E = entries[i];
    if (zoom) {                               // a check of its own: the box may exceed the tile, the out size may not
      const int dh = E.hE - E.h0, dw = E.wE - E.w0;
      FU_REQUIRE(E.scene, "%s: entry %d: null scene", fn, i);
      FU_REQUIRE(E.scene_h >= 1 && E.scene_w >= 1, "%s: entry %d: bad scene size %dx%d", fn, i, E.scene_h, E.scene_w);
      FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && E.hE <= E.scene_h && E.wE <= E.scene_w,
                 "%s: entry %d: box [%d:%d, %d:%d] lies outside its scene %dx%d", fn, i, E.h0, E.hE, E.w0, E.wE, E.scene_h,
                 E.scene_w);
      FU_REQUIRE(dh >= 1 && dw >= 1, "%s: entry %d: box [%d:%d, %d:%d] is empty", fn, i, E.h0, E.hE, E.w0, E.wE);
      FU_REQUIRE((int64_t)dh * dw <= INT32_MAX, "%s: entry %d: box %dx%d is too large", fn, i, dh, dw);
      FU_REQUIRE(aug->out_h[i] >= 1 && aug->out_h[i] <= H && aug->out_w[i] >= 1 && aug->out_w[i] <= W,
                 "%s: entry %d: out size %dx%d must lie within 1x1 and the tile %dx%d", fn, i, aug->out_h[i], aug->out_w[i],
                 H, W);
      jobs[i] = SceneCropJob{E.scene, E.scene_h, E.scene_w, E.h0, E.w0, dh, dw};
    } else {
      FU_TRY(check_scene_box(fn, i, E, H, W, jobs[i]));
    }
    FU_REQUIRE(!target_out || E.label, "%s: entry %d: target_out given but the entry has no label", fn, i);
    FU_REQUIRE((E.flags & ~(FU_AUG_HFLIP | FU_AUG_VFLIP | FU_AUG_ROTATE)) == 0, "%s: entry %d: unknown flag bits 0x%x", fn, i,
               (unsigned)E.flags);
    FU_REQUIRE(std::isfinite(E.angle_deg), "%s: entry %d: the angle is not finite", fn, i);
    augs[i] = SceneTrainAug{E.label, E.flags, E.angle_deg};
    const uint64_t st = aug->noise_stream ? aug->noise_stream[i] : 0;
    exs[i] = SceneAugEx{zoom ? aug->out_h[i] : 0, zoom ? aug->out_w[i] : 0, (uint32_t)st, (uint32_t)(st >> 32)};
  }
  size_t term_off[3] = {0, 0, 0};
  {
    size_t off = crop_bytes + aug_bytes + ex_bytes;
    const float* terms[3] = {aug->gain, aug->bias, aug->sigma};
    for (int k = 0; k < 3; ++k) {
      if (!terms[k]) continue;
      std::copy(terms[k], terms[k] + nc, reinterpret_cast<float*>(host.data() + off));
      term_off[k] = off;
      off += term_bytes;
    }
  }
  FU_TRY(table.upload(host.data(), host.size(),
                      sizeof(SceneCropJob) + sizeof(SceneTrainAug) + sizeof(SceneAugEx) + 3 * (size_t)C * sizeof(float), s));
  const unsigned char* dev = static_cast<const unsigned char*>(table.dev);
  const SceneCropJob* jobs_dev = reinterpret_cast<const SceneCropJob*>(dev);
  const SceneTrainAug* augs_dev = reinterpret_cast<const SceneTrainAug*>(dev + crop_bytes);
  const SceneAugEx* exs_dev = reinterpret_cast<const SceneAugEx*>(dev + crop_bytes + aug_bytes);
  ScenePhoto T;
  T.gain = aug->gain ? reinterpret_cast<const float*>(dev + term_off[0]) : nullptr;
  T.bias = aug->bias ? reinterpret_cast<const float*>(dev + term_off[1]) : nullptr;
  T.sigma = aug->sigma ? reinterpret_cast<const float*>(dev + term_off[2]) : nullptr;
  T.key_lo = (uint32_t)aug->noise_key;
  T.key_hi = (uint32_t)(aug->noise_key >> 32);
  T.k = (float)(1.0 / sqrt(32.0 * (65536.0 * 65536.0 - 1.0) / 12.0));
  ScenePlanes P;
  P.jobs = jobs_dev;
  NormParams N;                               // 'local': the statistics of the source box's own pixels
  FU_TRY(resolve_norm(P, n, C, norm_mode, gmean, gstd, mean_out, std_out, s, N));
  const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(image_out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(target_out) & 15) == 0;
  const int64_t nq = (int64_t)H * (vec ? W / 4 : W);
  const dim3 grid((unsigned)(n * (C + (target_out ? 1 : 0))), (unsigned)ceil_div64(nq, (int64_t)256 * STT_RUNS));
#define FU_STT_AUG(PX, Z, PH)                                                                                           \
  hipLaunchKernelGGL((k_scene_train_tiles_aug<PX, Z, PH>), grid, dim3(256), 0, s, jobs_dev, augs_dev, exs_dev, T, C, H, W, \
                     N.mean, N.stdv, N.per_sample, pad_value, nodata_value, target_fill, image_out, target_out)
  if (vec) {
    if (zoom && photo) FU_STT_AUG(4, true, true);
    else if (zoom) FU_STT_AUG(4, true, false);
    else FU_STT_AUG(4, false, true);
  } else {
    if (zoom && photo) FU_STT_AUG(1, true, true);
    else if (zoom) FU_STT_AUG(1, true, false);
    else FU_STT_AUG(1, false, true);
  }
#undef FU_STT_AUG
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Class frequencies of resident label rasters (fu_label_class_counts), for "balanced" class weights: every pixel of every
// box of the table, decoded as k_scene_train_tiles decodes it.  A decoded label is 0, 1 or nodata_value, so a thread counts
// its pixels in three registers; a block folds them into a three-bin LDS histogram with integer atomics and adds the bins
// whose class lies in [0, n_classes) to the caller's counts with 64-bit integer atomics (the scheme of k_eval_confusion):
// exact, whatever the order.  blockIdx.x = box, blockIdx.y = a share of its pixels.
// ------------------------------------------------------------------------------------------------
struct LabelBox {          // device copy of a validated fu_scene_train_entry, as far as the counts need it
  const uint8_t* label;    // first pixel of the box
  int scene_w, dh, dw;
};

__global__ __launch_bounds__(256) void k_label_class_counts(const LabelBox* __restrict__ boxes, int64_t nodata_value,
                                                            int n_classes, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int bins[3];         // decoded 0, decoded 1, no data
  if (threadIdx.x < 3) bins[threadIdx.x] = 0u;
  __syncthreads();
  const LabelBox J = boxes[blockIdx.x];
  const unsigned npx = (unsigned)J.dh * (unsigned)J.dw;      // < 2^31 (launch_label_class_counts checks)
  unsigned c0 = 0, c1 = 0, cn = 0;
  for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < npx; i += gridDim.y * 256u) {
    const unsigned y = i / (unsigned)J.dw, x = i - y * (unsigned)J.dw;
    const int k = label_category(J.label[(int64_t)y * J.scene_w + x]);
    c0 += k == 0 ? 1u : 0u;
    c1 += k == 1 ? 1u : 0u;
    cn += k == 2 ? 1u : 0u;
  }
  if (c0) atomicAdd(&bins[0], c0);
  if (c1) atomicAdd(&bins[1], c1);
  if (cn) atomicAdd(&bins[2], cn);
  __syncthreads();
  if (threadIdx.x < 3 && bins[threadIdx.x]) {
    const int64_t d = threadIdx.x == 2 ? nodata_value : (int64_t)threadIdx.x;     // decode_label's three values
    if (d >= 0 && d < n_classes) atomicAdd(&counts[d], (unsigned long long)bins[threadIdx.x]);
  }
}

// The entry check of both label-count calls (fn goes into the messages): label, raster size and box of every entry, and
// the device form of each; *max_px, when given, receives the largest box area.  Nothing is copied or launched here.
static int check_label_boxes(const char* fn, int n, const fu_scene_train_entry* entries, std::vector<LabelBox>& boxes,
                             int64_t* max_px) {
  boxes.resize((size_t)n);
  int64_t mx = 0;
  for (int i = 0; i < n; ++i) {
    const fu_scene_train_entry& E = entries[i];
    const int dh = E.hE - E.h0, dw = E.wE - E.w0;
    FU_REQUIRE(E.label, "%s: entry %d: null label raster", fn, i);
    FU_REQUIRE(E.scene_h >= 1 && E.scene_w >= 1 && (int64_t)E.scene_h * E.scene_w <= INT32_MAX,
               "%s: entry %d: bad raster size %dx%d", fn, i, E.scene_h, E.scene_w);
    FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && E.hE <= E.scene_h && E.wE <= E.scene_w,
               "%s: entry %d: box [%d:%d, %d:%d] lies outside its raster %dx%d", fn, i, E.h0, E.hE, E.w0, E.wE, E.scene_h,
               E.scene_w);
    FU_REQUIRE(dh >= 1 && dw >= 1, "%s: entry %d: box [%d:%d, %d:%d] is empty", fn, i, E.h0, E.hE, E.w0, E.wE);
    boxes[i] = LabelBox{E.label + (int64_t)E.h0 * E.scene_w + E.w0, E.scene_w, dh, dw};
    mx = std::max<int64_t>(mx, (int64_t)dh * dw);
  }
  if (max_px) *max_px = mx;
  return 0;
}

// every check before anything is launched or copied: a rejected call leaves the stream and the counts untouched
int launch_label_class_counts(DeviceTable& table, int n, const fu_scene_train_entry* entries, int64_t nodata_value,
                              int n_classes, int64_t* counts, hipStream_t s) {
  const char* fn = "fu_label_class_counts";
  FU_REQUIRE(n >= 1 && n_classes >= 1, "%s: n = %d, n_classes = %d (both must be >= 1)", fn, n, n_classes);
  std::vector<LabelBox> boxes;
  int64_t max_px = 0;
  FU_TRY(check_label_boxes(fn, n, entries, boxes, &max_px));
  FU_TRY(table.upload(boxes.data(), (size_t)n * sizeof(LabelBox), sizeof(LabelBox), s));
  // 16 pixels per thread where the largest box allows it, at most 64 blocks per box
  const dim3 grid((unsigned)n, (unsigned)grid_for(max_px, 256 * 16, 64));
  hipLaunchKernelGGL(k_label_class_counts, grid, dim3(256), 0, s, static_cast<const LabelBox*>(table.dev), nodata_value,
                     n_classes, reinterpret_cast<unsigned long long*>(counts));
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The label content of every box of a table, separately (fu_label_box_counts), for content-aware tile sampling: row i of
// the output = the pixels of box i by label_category.  One workgroup per box, which owns its row of the output: no global
// atomic, no pre-zeroing, no dependence on launch order.  A row of the box is seen as the 16-byte aligned chunks of memory
// it touches, at most cpr = (dw + 30) / 16 of them (15 bytes of head, then whole chunks); the block's threads stride
// over the dh * cpr (row, chunk) pairs.  A chunk that lies wholly inside the row is one 16-byte load, the partial chunk at
// either end is read byte by byte, and a pair past the row's last chunk is skipped.  Counters: three registers per
// thread, a xor tree over the wave, a three-bin LDS fold over the four waves, three 64-bit stores by thread 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_label_box_counts(const LabelBox* __restrict__ boxes, int64_t* __restrict__ counts) {
  __shared__ unsigned int bins[3];
  if (threadIdx.x < 3) bins[threadIdx.x] = 0u;
  __syncthreads();
  const LabelBox J = boxes[blockIdx.x];
  const unsigned cpr = ((unsigned)J.dw + 30u) / 16u;
  // dh * dw < 2^31 (check_label_boxes), so dh * cpr <= dh * dw * 31 / 16 < 2^32
  const unsigned n_items = (unsigned)J.dh * cpr;
  unsigned c[3] = {0u, 0u, 0u};
  for (unsigned i = threadIdx.x; i < n_items; i += 256u) {
    const unsigned y = i / cpr, k = i - y * cpr;
    const uint8_t* __restrict__ row = J.label + (int64_t)y * J.scene_w;
    const int head = (int)(reinterpret_cast<uintptr_t>(row) & 15);   // bytes of the first chunk that precede the row
    const int x0 = (int)k * 16 - head;                               // the chunk is row[x0, x0 + 16)
    if (x0 >= J.dw) continue;
    if (x0 >= 0 && x0 + 16 <= J.dw) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int cat = label_category((uint8_t)(w[q] >> (8 * b)));
          c[0] += cat == 0 ? 1u : 0u;
          c[1] += cat == 1 ? 1u : 0u;
          c[2] += cat == 2 ? 1u : 0u;
        }
      }
    } else {
      for (int x = max(x0, 0); x < min(x0 + 16, J.dw); ++x) {
        const int cat = label_category(row[x]);
        c[0] += cat == 0 ? 1u : 0u;
        c[1] += cat == 1 ? 1u : 0u;
        c[2] += cat == 2 ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_xor(c[j], o, 64);
    if ((threadIdx.x & 63) == 0 && c[j]) atomicAdd(&bins[j], c[j]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* __restrict__ o = counts + (int64_t)blockIdx.x * 3;
    o[0] = (int64_t)bins[0];
    o[1] = (int64_t)bins[1];
    o[2] = (int64_t)bins[2];
  }
}

// every check before anything is launched or copied: a rejected call leaves the stream and the counts untouched
int launch_label_box_counts(DeviceTable& table, int n, const fu_scene_train_entry* entries, int64_t* counts, hipStream_t s) {
  const char* fn = "fu_label_box_counts";
  FU_REQUIRE(n >= 1, "%s: n = %d (must be >= 1)", fn, n);
  std::vector<LabelBox> boxes;
  FU_TRY(check_label_boxes(fn, n, entries, boxes, nullptr));
  FU_TRY(table.upload(boxes.data(), (size_t)n * sizeof(LabelBox), sizeof(LabelBox), s));
  hipLaunchKernelGGL(k_label_box_counts, dim3((unsigned)n), dim3(256), 0, s, static_cast<const LabelBox*>(table.dev),
                     counts);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Streaming per-band statistics of tiles in HBM (fu_band_stats): what misc/compute_dataset_normalization_parameters.py
// gathers on the host with np.concatenate in a loop -- count, sum, sum of squares, min, max, a histogram and the count of
// non-finite pixels per channel, ADDED to caller-owned accumulators so that a data set streams through batch by batch.
// One pass: a thread owns VEC pixels along W of ALL channels (the pixel mask needs every channel of the first source, the
// finite test every channel of every source), loads them with one 16-byte read per channel, accumulates in registers
// (fp64 sums), and walks the batch with a grid stride.  Per block: a fixed xor tree over each wave, the waves folded in
// order through LDS, one row of partials [count, n_nonfinite, C x (sum, sumsq, min, max)] into the workspace; the
// histogram is counted with integer LDS atomics and written to the workspace once.  k_band_stats_fold then adds the rows
// in a fixed order (64 strided lanes per channel + xor tree) and k_band_hist_fold the per-block histograms: no
// floating-point atomic anywhere, so the same calls on the same data give the same bits.
// ------------------------------------------------------------------------------------------------
static constexpr int BST_MAX_C = 16;              // channels of all sources together (register accumulators)
static constexpr int BST_MAX_BLOCKS = 1024;       // rows of partials in the workspace
static constexpr int BST_HIST_BLOCKS = 256;       // blocks of a histogram launch: one per CU, each with its own LDS histogram
static constexpr int BST_LDS_WORDS = 38912;       // 152 KiB of the CU's 160 KiB LDS: 9 channels x 4096 bins fit
static constexpr int BST_MAX_BINS = 65536;

struct BandStatsArgs {
  BatchPlanes P;
  int C, B, QW, mask_mode, c_first, n_bins, c_lds;
  float lo, scale;
  unsigned* ws_hist;              // [gridDim.x][c_lds * n_bins]
  unsigned long long* hist;       // [C][n_bins]: channels >= c_lds (an LDS histogram too large) are added here directly
  double* ws;                     // [gridDim.x][2 + 4 * C]
};

__device__ __forceinline__ bool bst_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <int CMAX, int VEC, bool HIST>
__global__ __launch_bounds__(HIST ? 512 : 256) void k_band_stats(BandStatsArgs A) {
  constexpr int T = HIST ? 512 : 256, NW = T / 64;
  __shared__ double red[NW][2 + 4 * CMAX];
  __shared__ unsigned sh_hist[HIST ? BST_LDS_WORDS : 1];
  const int C = A.C, H = A.P.H, W = A.P.W, tid = threadIdx.x;
  const int nlds = HIST ? A.c_lds * A.n_bins : 0;
  if (HIST) {
    for (int i = tid; i < nlds; i += T) sh_hist[i] = 0u;
    __syncthreads();
  }
  double s[CMAX], q[CMAX];
  float mn[CMAX], mx[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) { s[c] = 0.0; q[c] = 0.0; mn[c] = INFINITY; mx[c] = -INFINITY; }
  long long cnt = 0, bad = 0;
  const unsigned total = (unsigned)A.B * (unsigned)H * (unsigned)A.QW;      // < 2^31 (launch_band_stats checks)
  for (unsigned idx = blockIdx.x * T + tid; idx < total; idx += gridDim.x * T) {
    const unsigned r = idx / (unsigned)A.QW;
    const int x0 = (int)(idx - r * (unsigned)A.QW) * VEC;
    const int b = (int)(r / (unsigned)H), y = (int)(r - (unsigned)b * (unsigned)H);
    const int vw = A.P.valid_w(b);
    if (y >= A.P.valid_h(b) || x0 >= vw) continue;
    const int off = y * W + x0;
    float v[CMAX][VEC];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        const float* p = A.P.plane(b, c) + off;
        if constexpr (VEC == 4) {
          const float4 t = *reinterpret_cast<const float4*>(p);
          v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        } else {
          v[c][0] = *p;
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[c][j] = 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const bool in = x0 + j < vw;
      bool fin = true;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) fin = fin && bst_finite(v[c][j]);
      bool take = in && fin;
      if (A.mask_mode == 1) {       // fp32 sum of the first source's channels, in channel order, is not 0
        float m = v[0][j];
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
          if (c < A.c_first) m = m + v[c][j];
        take = take && m != 0.f;
      }
      bad += (in && !fin) ? 1 : 0;
      cnt += take ? 1 : 0;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
          const float x = v[c][j];
          const double d = take ? (double)x : 0.0;
          s[c] += d;
          q[c] += d * d;
          mn[c] = take ? fminf(mn[c], x) : mn[c];
          mx[c] = take ? fmaxf(mx[c], x) : mx[c];
          if (HIST && take) {
            const float t = (x - A.lo) * A.scale;
            const int bin = t > 0.f ? (int)fminf(floorf(t), (float)(A.n_bins - 1)) : 0;
            if (c < A.c_lds) atomicAdd(&sh_hist[c * A.n_bins + bin], 1u);
            else atomicAdd(&A.hist[(size_t)c * A.n_bins + bin], 1ull);
          }
        }
      }
    }
  }
  // fixed xor tree over the wave, then the waves in order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    bad += __shfl_xor(bad, o, 64);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      s[c] += __shfl_xor(s[c], o, 64);
      q[c] += __shfl_xor(q[c], o, 64);
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
    }
  }
  if (lane == 0) {
    red[wave][0] = __longlong_as_double(cnt);
    red[wave][1] = __longlong_as_double(bad);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      red[wave][2 + 4 * c + 0] = s[c];
      red[wave][2 + 4 * c + 1] = q[c];
      red[wave][2 + 4 * c + 2] = (double)mn[c];
      red[wave][2 + 4 * c + 3] = (double)mx[c];
    }
  }
  __syncthreads();
  double* row = A.ws + (size_t)blockIdx.x * (2 + 4 * C);
  if (tid < 2) {
    long long t = 0;
    for (int w = 0; w < NW; ++w) t += __double_as_longlong(red[w][tid]);
    row[tid] = __longlong_as_double(t);
  } else if (tid < 2 + 4 * C) {
    const int k = (tid - 2) & 3;
    double t = red[0][tid];
    for (int w = 1; w < NW; ++w) t = k < 2 ? t + red[w][tid] : (k == 2 ? fmin(t, red[w][tid]) : fmax(t, red[w][tid]));
    row[tid] = t;
  }
  if (HIST) {
    unsigned* dst = A.ws_hist + (size_t)blockIdx.x * nlds;
    for (int i = tid; i < nlds; i += T) dst[i] = sh_hist[i];
  }
}

// one block of 64 lanes per channel: lane l adds rows l, l + 64, ... in order, then a fixed xor tree; lane 0 adds the
// result to the caller's accumulators (plain read-modify-write: one owner per channel)
__global__ __launch_bounds__(64) void k_band_stats_fold(const double* __restrict__ ws, int nblk, int C, BandAccum acc) {
  const int c = blockIdx.x, l = threadIdx.x;
  const int stride = 2 + 4 * C;
  long long cnt = 0, bad = 0;
  double s = 0.0, q = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int k = l; k < nblk; k += 64) {
    const double* row = ws + (size_t)k * stride;
    cnt += __double_as_longlong(row[0]);
    bad += __double_as_longlong(row[1]);
    s += row[2 + 4 * c + 0];
    q += row[2 + 4 * c + 1];
    mn = fmin(mn, row[2 + 4 * c + 2]);
    mx = fmax(mx, row[2 + 4 * c + 3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    bad += __shfl_xor(bad, o, 64);
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
    mn = fmin(mn, __shfl_xor(mn, o, 64));
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if (l != 0) return;
  acc.count[c] += cnt;
  acc.n_nonfinite[c] += bad;
  acc.sum[c] += s;
  acc.sumsq[c] += q;
  acc.vmin[c] = fminf(acc.vmin[c], (float)mn);
  acc.vmax[c] = fmaxf(acc.vmax[c], (float)mx);
}

// hist[i] += the blocks' LDS histograms: 64 bins x 4 lanes of blocks per workgroup, one owner per bin
__global__ __launch_bounds__(256) void k_band_hist_fold(const unsigned* __restrict__ ws_hist, int nblk, int n,
                                                        long long* __restrict__ hist) {
  __shared__ long long sm[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  long long t = 0;
  if (i < n) {
#pragma unroll 8
    for (int k = ty; k < nblk; k += 4) t += ws_hist[(size_t)k * n + i];
  }
  sm[ty][tx] = t;
  __syncthreads();
  if (ty == 0 && i < n) hist[i] += (sm[0][tx] + sm[1][tx]) + (sm[2][tx] + sm[3][tx]);
}

static int band_stats_c_lds(int C, int n_bins) { return n_bins > 0 ? (C < BST_LDS_WORDS / n_bins ? C : BST_LDS_WORDS / n_bins) : 0; }
static int64_t band_stats_rows_bytes(int C) { return (int64_t)BST_MAX_BLOCKS * (2 + 4 * C) * (int64_t)sizeof(double); }

int64_t band_stats_workspace_bytes(int C, int n_bins) {
  return band_stats_rows_bytes(C) + (int64_t)BST_HIST_BLOCKS * band_stats_c_lds(C, n_bins) * n_bins * (int64_t)sizeof(unsigned);
}

template <int CMAX, int VEC>
static void launch_band_stats_t(bool hist, int nblk, hipStream_t s, const BandStatsArgs& A) {
  if (hist) hipLaunchKernelGGL((k_band_stats<CMAX, VEC, true>), dim3(nblk), dim3(512), 0, s, A);
  else hipLaunchKernelGGL((k_band_stats<CMAX, VEC, false>), dim3(nblk), dim3(256), 0, s, A);
}

// Every check comes before the first launch: a rejected call leaves the stream and the accumulators untouched.
int launch_band_stats(const float* const* srcs, const int* src_channels, int n_src, int B, int H, int W, const int* vh,
                      const int* vw, int mask_mode, const BandAccum& acc, void* workspace, int64_t workspace_bytes,
                      hipStream_t s) {
  FU_REQUIRE(n_src >= 1 && n_src <= 8, "band_stats: 1..8 sources (got %d)", n_src);
  FU_REQUIRE(B >= 1 && H >= 1 && W >= 1, "band_stats: B = %d, H = %d, W = %d (all must be >= 1)", B, H, W);
  FU_REQUIRE(mask_mode == 0 || mask_mode == 1, "band_stats: mask_mode must be 0 (every pixel) or 1 (first source's "
             "channel sum != 0), got %d", mask_mode);
  BandStatsArgs A;
  A.P.S.n = n_src;
  int off = 0;
  bool aligned = W % 4 == 0;
  for (int k = 0; k < n_src; ++k) {
    FU_REQUIRE(srcs[k] && src_channels[k] >= 1 && src_channels[k] <= BST_MAX_C, "band_stats: bad source %d", k);
    A.P.S.p[k] = srcs[k]; A.P.S.c[k] = src_channels[k]; A.P.S.coff[k] = off; off += src_channels[k];
    aligned = aligned && ((uintptr_t)srcs[k] & 15) == 0;
  }
  const int C = off;
  A.P.S.coff[n_src] = C;
  A.P.H = H; A.P.W = W; A.P.vh = vh; A.P.vw = vw;
  FU_REQUIRE(C <= BST_MAX_C, "band_stats: %d channels in all, at most %d", C, BST_MAX_C);
  FU_REQUIRE((int64_t)H * W <= INT32_MAX && (int64_t)B * H * W < ((int64_t)1 << 31),
             "band_stats: batch of %d tiles of %dx%d is too large for one call", B, H, W);
  FU_REQUIRE(acc.count && acc.sum && acc.sumsq && acc.vmin && acc.vmax && acc.n_nonfinite,
             "band_stats: missing accumulators (count, sum, sumsq, min, max, n_nonfinite are all needed)");
  const bool hist = acc.hist != nullptr;
  if (hist) {
    FU_REQUIRE(acc.n_bins >= 1 && acc.n_bins <= BST_MAX_BINS, "band_stats: n_bins = %d out of range 1..%d", acc.n_bins,
               BST_MAX_BINS);
    FU_REQUIRE(acc.hi > acc.lo && acc.hi - acc.lo <= 3.0e38f && acc.lo >= -3.0e38f,
               "band_stats: histogram range needs finite lo < hi (got [%g, %g])", (double)acc.lo, (double)acc.hi);
  }
  const int n_bins = hist ? acc.n_bins : 0;
  FU_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= band_stats_workspace_bytes(C, n_bins),
             "band_stats: workspace missing, not 16-byte aligned or smaller than fu_band_stats_workspace_bytes = %lld",
             (long long)band_stats_workspace_bytes(C, n_bins));
  const int VEC = aligned ? 4 : 1;
  A.C = C; A.B = B; A.QW = W / VEC; A.mask_mode = mask_mode; A.c_first = src_channels[0];
  A.n_bins = n_bins; A.c_lds = band_stats_c_lds(C, n_bins);
  A.lo = acc.lo; A.scale = hist ? (float)n_bins / (acc.hi - acc.lo) : 0.f;
  A.ws = (double*)workspace;
  A.ws_hist = (unsigned*)((char*)workspace + band_stats_rows_bytes(C));
  A.hist = (unsigned long long*)acc.hist;
  const int T = hist ? 512 : 256;
  const int64_t units = (int64_t)B * H * A.QW;
  const int64_t want = ceil_div64(units, T), cap = hist ? BST_HIST_BLOCKS : BST_MAX_BLOCKS;
  const int nblk = (int)(want < cap ? want : cap);
#define FU_BST(CM) (VEC == 4 ? launch_band_stats_t<CM, 4>(hist, nblk, s, A) : launch_band_stats_t<CM, 1>(hist, nblk, s, A))
  if (C <= 4) FU_BST(4);
  else if (C <= 8) FU_BST(8);
  else if (C <= 12) FU_BST(12);
  else FU_BST(16);
#undef FU_BST
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_band_stats_fold, dim3(C), dim3(64), 0, s, (const double*)A.ws, nblk, C, acc);
  FU_LAUNCH_CHECK();
  if (hist && A.c_lds > 0) {
    const int n = A.c_lds * n_bins;
    hipLaunchKernelGGL(k_band_hist_fold, dim3(ceil_div(n, 64)), dim3(256), 0, s, (const unsigned*)A.ws_hist, nblk, n,
                       (long long*)acc.hist);
    FU_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace fu
