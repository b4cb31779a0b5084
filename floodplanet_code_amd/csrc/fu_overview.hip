// fu_map_overviews (gfx950): the reduced-resolution levels of a device-resident raster -- base pointer plus element strides
// (band, row, column) -- for the overview images of a TIFF.  Level l >= 1 is ceil(h / 2^l) x ceil(w / 2^l); its pixel (y, x)
// is reduced from the pixels (2y..2y+1, 2x..2x+1) of level l - 1 that exist (a cascade: never from the base).  The numpy
// statement is datasets/overviews.py's overviews_host, and every comparison against it is equality of bits.
//
// One pass per launch.  Because the sizes are ceil-halved, pixel y of level l comes from rows y << l .. of the base and from
// nothing else, so a TILE-aligned base tile is self-contained for log2(TILE) levels: a workgroup loads its TILE x TILE tile
// (and the tile of the mask) into LDS once, 16-byte loads where the source is unit-stride and aligned, reduces it in LDS
// level by level and writes every level's block.  The base is read from HBM once and what is written is at most a third
// of it.  Deeper levels come from one further launch whose source is the last level written, with its mask level.
// LDS: the tile and its levels back to back, TILE^2 * 4 / 3 elements: 5.4 KB for uint8, 21.4 KB for fp32, plus 5.4 KB of mask.
// wave64, 256 lanes per workgroup, no atomics, no dependency between workgroups, 64-bit offsets.
#include "fu_common.h"
#include "../../include/floodunet.h"

#include <stdint.h>

namespace fu {

constexpr int OV_TILE = 64;                        // base pixels per tile side; a power of two
constexpr int OV_LEVELS = 6;                       // log2(OV_TILE): the levels one launch writes
constexpr int OV_LDS = 5464;                       // 4096 + 1024 + 256 + 64 + 16 + 4 + 1 elements, rounded up to 8

struct OvArgs {
  const void* src;
  const unsigned char* valid;                      // [h, w] of the source level, or null
  int64_t band_stride, row_stride, col_stride;     // of src, in elements
  int nodata;                                      // mode_u8: the value that takes no part (-1: none)
  int n_levels;                                    // of this launch, 1..OV_LEVELS
  int h[OV_LEVELS + 1], w[OV_LEVELS + 1];          // [0]: the source; [k]: level k of this launch
  void* dst[OV_LEVELS + 1];                        // [k]: [bands, h[k], w[k]] contiguous
  unsigned char* vdst[OV_LEVELS + 1];              // [k]: [h[k], w[k]] or null
};

// where level k of the tile starts in the LDS array (its row stride is OV_TILE >> k)
__device__ __forceinline__ int ov_off(int k) { return (4096 * 4 - (16384 >> (2 * k))) / 3; }

// a TILE x TILE tile of a strided raster -> lds (row stride OV_TILE); what lies outside the raster is not read and holds 0
template <typename T>
__device__ __forceinline__ void ov_load_tile(const T* src, int64_t row_stride, int64_t col_stride, int h, int w, int y0, int x0,
                                             T* lds) {
  constexpr int E = 16 / (int)sizeof(T);           // elements per 16-byte unit
  constexpr int UPR = OV_TILE / E;                 // units per tile row
  for (int u = threadIdx.x; u < OV_TILE * UPR; u += blockDim.x) {
    const int ly = u / UPR, lx = (u - ly * UPR) * E;
    const int gy = y0 + ly, gx = x0 + lx;
    T* out = lds + ly * OV_TILE + lx;
    if (gy >= h || gx >= w) {
#pragma unroll
      for (int j = 0; j < E; ++j) out[j] = T(0);
      continue;
    }
    const T* p = src + (int64_t)gy * row_stride + (int64_t)gx * col_stride;
    if (col_stride == 1 && gx + E <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(p);
    } else {
#pragma unroll
      for (int j = 0; j < E; ++j) out[j] = gx + j < w ? p[(int64_t)j * col_stride] : T(0);
    }
  }
}

// KIND: fu_overview_kind.  T: uint8 for the three integer kinds, float for mean_f32.
template <int KIND, typename T>
__global__ __launch_bounds__(256) void k_map_overviews(const OvArgs a) {
  __shared__ __attribute__((aligned(16))) T s_val[OV_LDS];
  __shared__ __attribute__((aligned(16))) unsigned char s_ok[OV_LDS];
  constexpr bool MEAN = KIND == FU_OVERVIEW_MEAN_U8 || KIND == FU_OVERVIEW_MEAN_F32;
  const int tiles_x = (a.w[0] + OV_TILE - 1) / OV_TILE;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int band = blockIdx.y;
  const bool masked = MEAN && a.valid != nullptr;
  ov_load_tile<T>(static_cast<const T*>(a.src) + (int64_t)band * a.band_stride, a.row_stride, a.col_stride, a.h[0], a.w[0],
                  ty * OV_TILE, tx * OV_TILE, s_val);
  if (masked) ov_load_tile<unsigned char>(a.valid, a.w[0], 1, a.h[0], a.w[0], ty * OV_TILE, tx * OV_TILE, s_ok);
  __syncthreads();
  for (int k = 1; k <= a.n_levels; ++k) {
    const int side = OV_TILE >> k;                 // of this level's block; the level below has 2 * side
    const int y0 = ty * side, x0 = tx * side;
    const int hp = a.h[k - 1] - 2 * y0, wp = a.w[k - 1] - 2 * x0;    // rows / columns of the level below inside the tile
    const T* pv = s_val + ov_off(k - 1);
    const unsigned char* pm = s_ok + ov_off(k - 1);
    T* qv = s_val + ov_off(k);
    unsigned char* qm = s_ok + ov_off(k);
    for (int i = threadIdx.x; i < side * side; i += blockDim.x) {
      const int ly = i / side, lx = i - ly * side;
      const int gy = y0 + ly, gx = x0 + lx;
      if (gy >= a.h[k] || gx >= a.w[k]) continue;
      T v[4];
      bool ok[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                // row-major: (0, 0), (0, 1), (1, 0), (1, 1)
        const int sy = 2 * ly + (j >> 1), sx = 2 * lx + (j & 1);
        const int at = sy * (2 * side) + sx;
        v[j] = pv[at];
        ok[j] = sy < hp && sx < wp;
        if (masked) ok[j] = ok[j] && pm[at] != 0;
        if (KIND == FU_OVERVIEW_MODE_U8) ok[j] = ok[j] && (int)v[j] != a.nodata;
      }
      T r;
      if constexpr (KIND == FU_OVERVIEW_MODE_U8) {
        int best = -1;                             // count << 8 | 255 - value: the most frequent, ties to the smaller value
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int n = 0;
#pragma unroll
          for (int m = 0; m < 4; ++m) n += ok[m] && v[m] == v[j];
          const int key = ok[j] ? (n << 8) | (255 - (int)v[j]) : -1;
          best = max(best, key);
        }
        r = best < 0 ? (T)a.nodata : (T)(255 - (best & 255));
      } else if constexpr (KIND == FU_OVERVIEW_MEAN_U8) {
        int sum = 0, n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += ok[j] ? (int)v[j] : 0, n += ok[j];
        r = n ? (T)((2 * sum + n) / (2 * n)) : T(0);
      } else if constexpr (KIND == FU_OVERVIEW_MEAN_F32) {
        float acc = 0.f;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ok[j]) acc = __fadd_rn(acc, (float)v[j]), ++n;
        r = n ? (T)__fdiv_rn(acc, (float)n) : T(0);
      } else {
        r = (T)((ok[0] && v[0] != T(0)) || (ok[1] && v[1] != T(0)) || (ok[2] && v[2] != T(0)) || (ok[3] && v[3] != T(0)));
      }
      qv[ly * side + lx] = r;
      const int64_t at = (int64_t)gy * a.w[k] + gx;
      static_cast<T*>(a.dst[k])[(int64_t)band * a.h[k] * a.w[k] + at] = r;
      if (masked) {
        const unsigned char m = ok[0] || ok[1] || ok[2] || ok[3];
        qm[ly * side + lx] = m;
        if (band == 0) a.vdst[k][at] = m;
      }
    }
    __syncthreads();
  }
}

// ceil(log2(max(h, w))): the levels down to 1 x 1
static int ov_max_levels(int h, int w) {
  int n = 0;
  for (int m = h > w ? h : w; m > 1; m = (m + 1) / 2) ++n;
  return n;
}

// Every check before the first launch.  The kernels' stores stay inside dst / valid_dst because dst_elems covers the levels'
// arithmetic total and every store is guarded by its level's size; their loads stay inside the raster the strides describe.
int launch_map_overviews(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, int bands, int h, int w,
                         int kind, const uint8_t* valid, int nodata_value, int n_levels, void* dst, int64_t dst_elems,
                         uint8_t* valid_dst, hipStream_t s) {
  const char* fn = "fu_map_overviews";
  FU_REQUIRE(src && dst, "%s: null src / dst", fn);
  FU_REQUIRE(kind >= FU_OVERVIEW_MODE_U8 && kind <= FU_OVERVIEW_ANY_U8, "%s: unknown kind %d", fn, kind);
  FU_REQUIRE(bands >= 1 && bands <= FU_TIFF_MAX_BANDS, "%s: bands = %d not in 1..%d", fn, bands, FU_TIFF_MAX_BANDS);
  FU_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= FU_MAP_MAX_PIXELS, "%s: raster %dx%d is empty or has more than 2^28 pixels",
             fn, h, w);
  FU_REQUIRE(band_stride >= 0 && row_stride >= 0 && col_stride >= 0, "%s: negative source stride", fn);
  FU_REQUIRE(n_levels >= 0 && n_levels <= ov_max_levels(h, w), "%s: n_levels = %d not in 0..%d (the levels of %dx%d down to 1x1)",
             fn, n_levels, ov_max_levels(h, w), h, w);
  const bool mean = kind == FU_OVERVIEW_MEAN_U8 || kind == FU_OVERVIEW_MEAN_F32;
  FU_REQUIRE((valid != nullptr) == (valid_dst != nullptr), "%s: valid and valid_dst go together", fn);
  FU_REQUIRE(mean || !valid, "%s: only the mean kinds take a valid mask", fn);
  if (kind == FU_OVERVIEW_MODE_U8)
    FU_REQUIRE(nodata_value >= -1 && nodata_value <= 255, "%s: nodata_value %d not in -1..255", fn, nodata_value);
  else
    FU_REQUIRE(nodata_value == -1, "%s: only mode_u8 takes a nodata_value (got %d, want -1)", fn, nodata_value);
  const int esize = kind == FU_OVERVIEW_MEAN_F32 ? 4 : 1;
  FU_REQUIRE(reinterpret_cast<uintptr_t>(src) % esize == 0 && reinterpret_cast<uintptr_t>(dst) % esize == 0,
             "%s: misaligned src / dst (the sample size)", fn);
  int64_t total = 0;
  for (int l = 1, lh = h, lw = w; l <= n_levels; ++l) {
    lh = (lh + 1) / 2, lw = (lw + 1) / 2;
    total += (int64_t)lh * lw;
  }
  FU_REQUIRE(dst_elems >= (int64_t)bands * total, "%s: dst_elems = %lld, the levels hold %lld", fn, (long long)dst_elems,
             (long long)bands * total);
  // launches of up to OV_LEVELS levels each; the source of a later one is the last level the one before it wrote
  OvArgs a{};
  a.src = src, a.valid = valid;
  a.band_stride = band_stride, a.row_stride = row_stride, a.col_stride = col_stride;
  a.nodata = nodata_value;
  a.h[0] = h, a.w[0] = w;
  char* out = static_cast<char*>(dst);
  uint8_t* vout = valid_dst;
  for (int done = 0; done < n_levels;) {
    a.n_levels = n_levels - done < OV_LEVELS ? n_levels - done : OV_LEVELS;
    for (int k = 1; k <= a.n_levels; ++k) {
      a.h[k] = (a.h[k - 1] + 1) / 2, a.w[k] = (a.w[k - 1] + 1) / 2;
      a.dst[k] = out, a.vdst[k] = vout;
      out += (int64_t)bands * a.h[k] * a.w[k] * esize;
      if (vout) vout += (int64_t)a.h[k] * a.w[k];
    }
    const dim3 grid((unsigned)(ceil_div64(a.h[0], OV_TILE) * ceil_div64(a.w[0], OV_TILE)), (unsigned)bands);
    const dim3 block(256);
    switch (kind) {
      case FU_OVERVIEW_MODE_U8:
        hipLaunchKernelGGL((k_map_overviews<FU_OVERVIEW_MODE_U8, unsigned char>), grid, block, 0, s, a); break;
      case FU_OVERVIEW_MEAN_U8:
        hipLaunchKernelGGL((k_map_overviews<FU_OVERVIEW_MEAN_U8, unsigned char>), grid, block, 0, s, a); break;
      case FU_OVERVIEW_MEAN_F32:
        hipLaunchKernelGGL((k_map_overviews<FU_OVERVIEW_MEAN_F32, float>), grid, block, 0, s, a); break;
      default:
        hipLaunchKernelGGL((k_map_overviews<FU_OVERVIEW_ANY_U8, unsigned char>), grid, block, 0, s, a); break;
    }
    FU_LAUNCH_CHECK();
    done += a.n_levels;
    const int last = a.n_levels;                   // the next launch reads what this one wrote last
    a.src = a.dst[last], a.valid = a.vdst[last];
    a.band_stride = (int64_t)a.h[last] * a.w[last], a.row_stride = a.w[last], a.col_stride = 1;
    a.h[0] = a.h[last], a.w[0] = a.w[last];
  }
  return 0;
}

}  // namespace fu
