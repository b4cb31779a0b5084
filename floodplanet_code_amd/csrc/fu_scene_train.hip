// What works on a table of fu_scene_train_entry (gfx950): training tiles straight from resident scenes
// (fu_scene_train_tiles[_ex]) and the label counts of the entries' boxes (fu_label_class_counts, fu_label_box_counts).  The
// tables are validated here, next to the kernels that trust them.
#include "fu_data.h"

#include <algorithm>
#include <vector>

namespace fu {

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

// ------------------------------------------------------------------------------------------------
// The same pass with radiometric and zoom augmentation (fu_scene_train_tiles_ex; include/floodunet.h states the arithmetic).
// A sibling of k_scene_train_tiles, which stays as it is (DESIGN.md has the two folds that were measured, both slower for the
// plain call): with zoom every pixel has its own source in any case, so this kernel has one loop -- per output pixel the flips and the rotation yield an integer pixel of the un-augmented tile, ZOOM
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

// the kernel of a call: the plain one with nothing switched on, else the sibling's instance for what is
template <int PX, class... Args>
static void launch_scene_train_t(bool zoom, bool photo, dim3 grid, hipStream_t s, const SceneCropJob* jobs,
                                 const SceneTrainAug* augs, const SceneAugEx* exs, const ScenePhoto& T, Args... args) {
  if (zoom && photo) hipLaunchKernelGGL((k_scene_train_tiles_aug<PX, true, true>), grid, dim3(256), 0, s, jobs, augs, exs, T, args...);
  else if (zoom) hipLaunchKernelGGL((k_scene_train_tiles_aug<PX, true, false>), grid, dim3(256), 0, s, jobs, augs, exs, T, args...);
  else if (photo) hipLaunchKernelGGL((k_scene_train_tiles_aug<PX, false, true>), grid, dim3(256), 0, s, jobs, augs, exs, T, args...);
  else hipLaunchKernelGGL(k_scene_train_tiles<PX>, grid, dim3(256), 0, s, jobs, augs, args...);
}

// fu_scene_train_tiles (aug = null) and fu_scene_train_tiles_ex.  Every check before anything is launched or copied: a
// rejected call leaves the stream untouched.
int launch_scene_train_tiles(DeviceTable& table, int n, const fu_scene_train_entry* entries, int C, int H, int W,
                             int norm_mode, const float* gmean, const float* gstd, float pad_value, int64_t nodata_value,
                             int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out, float* std_out,
                             const fu_scene_aug* aug, hipStream_t s) {
  static const fu_scene_aug all_off = {};
  const fu_scene_aug& G = aug ? *aug : all_off;
  const bool photo = G.gain || G.bias || G.sigma;
  const bool zoom = G.out_h || G.out_w;
  const bool ex = photo || zoom;              // nothing switched on: the plain call, its table, its kernel and its bits
  const char* fn = ex ? "fu_scene_train_tiles_ex" : "fu_scene_train_tiles";
  FU_REQUIRE(n >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: n = %d, C = %d, tile %dx%d (all must be >= 1)", fn, n, C, H, W);
  FU_TRY(check_norm_mode(fn, "[n, C]", norm_mode, gmean, gstd, mean_out, std_out));
  // fu_scene_crops' bounds, with the target plane counted; the kernel's grid.y walks a plane 1024 pixel runs at a time, so
  // 2^25 pixels (32768 rows of blocks with one pixel per run) stay inside the 65535 a launch accepts
  FU_REQUIRE((int64_t)n * (C + 1) <= INT32_MAX && (int64_t)n * C * H * W <= ((int64_t)1 << 40) &&
             (int64_t)H * W <= ((int64_t)1 << 25),
             "%s: %d boxes of %d channels, tile %dx%d, are too many for one call", fn, n, C, H, W);
  FU_REQUIRE(!zoom || (G.out_h && G.out_w), "%s: out_h and out_w go together", fn);
  FU_REQUIRE(!G.sigma || G.noise_stream, "%s: sigma needs noise_stream", fn);
  const size_t nc = (size_t)n * (size_t)C;
  for (size_t i = 0; photo && i < nc; ++i) {
    FU_REQUIRE(!G.gain || std::isfinite(G.gain[i]), "%s: gain[%zu] is not finite", fn, i);
    FU_REQUIRE(!G.bias || std::isfinite(G.bias[i]), "%s: bias[%zu] is not finite", fn, i);
    FU_REQUIRE(!G.sigma || (std::isfinite(G.sigma[i]) && G.sigma[i] >= 0.f),
               "%s: sigma[%zu] = %g must be finite and >= 0", fn, i, G.sigma ? (double)G.sigma[i] : 0.0);
  }
  // one table: the boxes, the transforms and, with something switched on, the per-sample extras, then the per-(sample,
  // channel) terms that are given
  const size_t crop_bytes = (size_t)n * sizeof(SceneCropJob), aug_bytes = (size_t)n * sizeof(SceneTrainAug);
  const size_t ex_bytes = ex ? (size_t)n * sizeof(SceneAugEx) : 0, term_bytes = nc * sizeof(float);
  const float* terms[3] = {G.gain, G.bias, G.sigma};
  const int n_terms = (G.gain ? 1 : 0) + (G.bias ? 1 : 0) + (G.sigma ? 1 : 0);
  std::vector<unsigned char> host(crop_bytes + aug_bytes + ex_bytes + (size_t)n_terms * term_bytes);
  SceneCropJob* jobs = reinterpret_cast<SceneCropJob*>(host.data());
  SceneTrainAug* augs = reinterpret_cast<SceneTrainAug*>(host.data() + crop_bytes);
  SceneAugEx* exs = reinterpret_cast<SceneAugEx*>(host.data() + crop_bytes + aug_bytes);
  for (int i = 0; i < n; ++i) {
    const fu_scene_train_entry& E = entries[i];
    FU_TRY(check_scene_box(fn, i, E, H, W, jobs[i], zoom, zoom ? G.out_h[i] : 0, zoom ? G.out_w[i] : 0));
    FU_REQUIRE(!target_out || E.label, "%s: entry %d: target_out given but the entry has no label", fn, i);
    FU_REQUIRE((E.flags & ~(FU_AUG_HFLIP | FU_AUG_VFLIP | FU_AUG_ROTATE)) == 0, "%s: entry %d: unknown flag bits 0x%x", fn, i,
               (unsigned)E.flags);
    FU_REQUIRE(std::isfinite(E.angle_deg), "%s: entry %d: the angle is not finite", fn, i);
    augs[i] = SceneTrainAug{E.label, E.flags, E.angle_deg};
    if (ex) {
      const uint64_t st = G.noise_stream ? G.noise_stream[i] : 0;
      exs[i] = SceneAugEx{zoom ? G.out_h[i] : 0, zoom ? G.out_w[i] : 0, (uint32_t)st, (uint32_t)(st >> 32)};
    }
  }
  size_t term_off[3] = {0, 0, 0};
  for (size_t k = 0, off = crop_bytes + aug_bytes + ex_bytes; k < 3; ++k) {
    if (!terms[k]) continue;
    std::copy(terms[k], terms[k] + nc, reinterpret_cast<float*>(host.data() + off));
    term_off[k] = off;
    off += term_bytes;
  }
  FU_TRY(table.upload(host.data(), host.size(), sizeof(SceneCropJob) + sizeof(SceneTrainAug) +
                                                    (ex ? sizeof(SceneAugEx) + 3 * (size_t)C * sizeof(float) : 0), s));
  const unsigned char* dev = static_cast<const unsigned char*>(table.dev);
  const SceneCropJob* jobs_dev = reinterpret_cast<const SceneCropJob*>(dev);
  const SceneTrainAug* augs_dev = reinterpret_cast<const SceneTrainAug*>(dev + crop_bytes);
  const SceneAugEx* exs_dev = ex ? reinterpret_cast<const SceneAugEx*>(dev + crop_bytes + aug_bytes) : nullptr;
  ScenePhoto T;
  T.gain = G.gain ? reinterpret_cast<const float*>(dev + term_off[0]) : nullptr;
  T.bias = G.bias ? reinterpret_cast<const float*>(dev + term_off[1]) : nullptr;
  T.sigma = G.sigma ? reinterpret_cast<const float*>(dev + term_off[2]) : nullptr;
  T.key_lo = (uint32_t)G.noise_key;
  T.key_hi = (uint32_t)(G.noise_key >> 32);
  T.k = (float)(1.0 / sqrt(32.0 * (65536.0 * 65536.0 - 1.0) / 12.0));
  ScenePlanes P;
  P.jobs = jobs_dev;
  NormParams N;                               // 'local': the statistics of the source box's own pixels, fu_scene_crops' own kernel
  FU_TRY(resolve_norm(P, n, C, norm_mode, gmean, gstd, mean_out, std_out, s, N));
  const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(image_out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(target_out) & 15) == 0;
  const int64_t nq = (int64_t)H * (vec ? W / 4 : W);
  const dim3 grid((unsigned)(n * (C + (target_out ? 1 : 0))), (unsigned)ceil_div64(nq, (int64_t)256 * STT_RUNS));
  if (vec)
    launch_scene_train_t<4>(zoom, photo, grid, s, jobs_dev, augs_dev, exs_dev, T, C, H, W, N.mean, N.stdv, N.per_sample,
                            pad_value, nodata_value, target_fill, image_out, target_out);
  else
    launch_scene_train_t<1>(zoom, photo, grid, s, jobs_dev, augs_dev, exs_dev, T, C, H, W, N.mean, N.stdv, N.per_sample,
                            pad_value, nodata_value, target_fill, image_out, target_out);
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

}  // namespace fu
