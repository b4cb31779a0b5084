// fu_tiff_pack (gfx950): a device-resident raster -- base pointer plus element strides (band, row, column) -- to the byte
// buffer a TIFF writer hands its entropy coder: planes after each other, cut into tiles or strips at their nominal size,
// edge tiles padded by edge replication, the predictor applied.  The exact inverse of fu_tiff_unpack; the numpy statement is
// datasets/geotiff_write.py's pack_host, and every comparison against it is equality of bytes.
//
// Encoding needs no scan: an output byte is a difference of at most two input bytes, so the kernel is a streaming gather.
// The samples inside a segment are always one per pixel (several samples are planar-separate), so a segment row holds wc =
// seg_w values in row_bytes = wc * bytes_per_sample bytes, every row of the buffer has that size, and row q of the buffer
// starts at q * row_bytes -- for strips the plane's rows in order, for tiles the tile's rows, tiles in offset-array order.
//
// Two kernels, one launch per call:
//   k_tiff_pack_rows   wc is a multiple of 16 (every tile; a strip whose width is): a lane takes 16 consecutive values of one
//                      row, loads them ONCE (16-byte loads where the source is unit-stride, aligned and needs no clamp) with
//                      the one value in front of them, and stores bytes_per_sample groups of 16 bytes: the differenced values
//                      themselves, or under the floating-point predictor one group in each byte plane.  The first byte of
//                      plane b > 0 differences against the last byte of plane b - 1, which is a byte of the row's last value.
//   k_tiff_pack_groups every other layout (strips of any width): a lane takes one 16-byte group of the flat buffer, which may
//                      begin in one row and end in another (a row can be shorter than a group), and stores it once.  A group
//                      inside one row (and one byte plane) is straight-line code: its 16, 8 or 4 values and the one in front
//                      loaded independently; a group across a row or plane boundary walks its 16 bytes with the row, plane
//                      and value indices carried along.  Only the buffer's last group can be short; it is stored byte by
//                      byte.  Under the floating-point predictor this kernel reads a value once per byte plane.
// All byte offsets are 64-bit.  No atomics, no LDS, no dependency between workgroups.
#include "fu_common.h"
#include "../../include/floodunet.h"

#include <stdint.h>

namespace fu {

struct TiffPack {
  const unsigned char* src;
  unsigned char* dst;
  int64_t band_stride, row_stride, col_stride;   // in elements
  int64_t n_bytes, n_rows, row_bytes;
  int width, height, seg_w, seg_h, tiled, predictor;
  int tiles_across, tiles_down;                  // 1, 1 for strips
};

// the source row and first column of buffer row q: (plane, image row clamped to the image, x0)
struct PackRow {
  int64_t base;   // element offset of (plane, clamped row, column 0)
  int x0;
};

__device__ __forceinline__ PackRow pack_row(const TiffPack& a, int64_t q) {
  int p, y, x0;
  if (a.tiled) {
    const int64_t seg = q / a.seg_h;
    const int r = (int)(q - seg * a.seg_h);
    const int tx = (int)(seg % a.tiles_across);
    const int64_t t = seg / a.tiles_across;
    const int ty = (int)(t % a.tiles_down);
    p = (int)(t / a.tiles_down);
    y = ty * a.seg_h + r, x0 = tx * a.seg_w;
  } else {
    p = (int)(q / a.height), y = (int)(q - (int64_t)p * a.height), x0 = 0;
  }
  y = min(y, a.height - 1);
  return PackRow{(int64_t)p * a.band_stride + (int64_t)y * a.row_stride, x0};
}

// value i of the row as a little-endian integer of BPS bytes; a column outside the image is the image's last column
template <int BPS>
__device__ __forceinline__ uint32_t pack_value(const TiffPack& a, const PackRow& r, int i) {
  const int x = min(r.x0 + i, a.width - 1);
  const int64_t e = r.base + (int64_t)x * a.col_stride;
  if (BPS == 1) return a.src[e];
  if (BPS == 2) return reinterpret_cast<const uint16_t*>(a.src)[e];
  return reinterpret_cast<const uint32_t*>(a.src)[e];
}

template <int BPS>
__global__ __launch_bounds__(256) void k_tiff_pack_rows(const TiffPack a) {
  constexpr uint32_t kMask = BPS == 4 ? 0xffffffffu : (1u << (8 * (BPS & 3))) - 1u;
  const int wc = a.seg_w;
  const int chunks = wc >> 4;                                 // wc % 16 == 0
  const int64_t n_units = a.n_rows * chunks;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = u / chunks;
    const int i0 = (int)(u - q * chunks) << 4;
    const PackRow r = pack_row(a, q);
    uint32_t v[16];
    const unsigned char* first = a.src + (r.base + (int64_t)(r.x0 + i0) * a.col_stride) * BPS;
    if (a.col_stride == 1 && r.x0 + i0 + 16 <= a.width && (reinterpret_cast<uintptr_t>(first) & 15) == 0) {
      uint32_t w[4 * BPS];
#pragma unroll
      for (int k = 0; k < BPS; ++k) {
        const uint4 t = reinterpret_cast<const uint4*>(first)[k];
        w[4 * k] = t.x, w[4 * k + 1] = t.y, w[4 * k + 2] = t.z, w[4 * k + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (BPS == 4) v[j] = w[j];
        else if (BPS == 2) v[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        else v[j] = (w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = pack_value<BPS>(a, r, i0 + j);
    }
    unsigned char* out = a.dst + q * a.row_bytes;
    if (a.predictor == 3) {                                   // BPS == 4: one 16-byte group in each byte plane
      const uint32_t before = i0 > 0 ? pack_value<BPS>(a, r, i0 - 1) : 0u;
      const uint32_t last = i0 == 0 ? pack_value<BPS>(a, r, wc - 1) : 0u;
#pragma unroll
      for (int b = 0; b < BPS; ++b) {
        const int sh = 8 * (BPS - 1 - b);
        // the byte in front of the group: the same plane's of value i0 - 1, or at the start of plane b > 0 the last
        // byte of plane b - 1; the row's first byte is stored as it is
        uint32_t prev = i0 > 0 ? (before >> sh) & 0xffu : b > 0 ? (last >> (sh + 8)) & 0xffu : 0u;
        uint32_t g[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const uint32_t cur = (v[j] >> sh) & 0xffu;
          g[j >> 2] |= ((cur - prev) & 0xffu) << ((j & 3) * 8);
          prev = cur;
        }
        *reinterpret_cast<uint4*>(out + (int64_t)b * wc + i0) = make_uint4(g[0], g[1], g[2], g[3]);
      }
    } else {
      uint32_t d[16];
      if (a.predictor == 2) {
        uint32_t prev = i0 > 0 ? pack_value<BPS>(a, r, i0 - 1) : 0u;   // the row's first value is stored as it is
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = (v[j] - prev) & kMask, prev = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = v[j];
      }
      uint4* o = reinterpret_cast<uint4*>(out + (int64_t)i0 * BPS);
#pragma unroll
      for (int k = 0; k < BPS; ++k) {
        uint32_t g[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (BPS == 4) g[m] = d[4 * k + m];
          else if (BPS == 2) g[m] = d[8 * k + 2 * m] | (d[8 * k + 2 * m + 1] << 16);
          else g[m] = d[4 * m] | (d[4 * m + 1] << 8) | (d[4 * m + 2] << 16) | (d[4 * m + 3] << 24);
        }
        o[k] = make_uint4(g[0], g[1], g[2], g[3]);
      }
    }
  }
}

template <int BPS>
__global__ __launch_bounds__(256) void k_tiff_pack_groups(const TiffPack a) {
  constexpr uint32_t kMask = BPS == 4 ? 0xffffffffu : (1u << (8 * (BPS & 3))) - 1u;
  const int wc = a.seg_w;
  const int64_t n_groups = (a.n_bytes + 15) >> 4;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t at = g << 4;
    const int n = (int)min((int64_t)16, a.n_bytes - at);
    int64_t q = at / a.row_bytes;
    int o = (int)(at - q * a.row_bytes);                      // the byte inside the row; row_bytes <= 2^30
    PackRow r = pack_row(a, q);
    // where byte o lies, carried along the walk: value index i and byte k inside the value (k counts byte planes, most
    // significant first, under the floating-point predictor, else the value's bytes in little-endian order)
    int i, k;
    if (a.predictor == 3) k = o / wc, i = o - k * wc;
    else i = o / BPS, k = o - i * BPS;
    // The common case, straight-line: the group lies in one row and, under the floating-point predictor, in one byte plane.
    // Its bytes are then those of consecutive values (a group starts on a value: rows are whole values long), which are
    // loaded independently of each other, with the one value in front.
    if (n == 16 && o + 16 <= (int)a.row_bytes && (a.predictor != 3 || i + 16 <= wc)) {
      uint32_t w4[4] = {0u, 0u, 0u, 0u};
      if (a.predictor == 3) {
        const int sh = 8 * (BPS - 1 - k);
        uint32_t prev = 0u;                                   // the row's first byte is stored as it is
        if (i > 0) prev = (pack_value<BPS>(a, r, i - 1) >> sh) & 0xffu;
        else if (k > 0) prev = (pack_value<BPS>(a, r, wc - 1) >> (sh + 8)) & 0xffu;   // the last byte of the plane in front
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = pack_value<BPS>(a, r, i + j);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const uint32_t cur = (v[j] >> sh) & 0xffu;
          w4[j >> 2] |= ((cur - prev) & 0xffu) << ((j & 3) * 8);
          prev = cur;
        }
      } else {
        constexpr int NV = 16 / BPS;
        uint32_t v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = pack_value<BPS>(a, r, i + j);
        if (a.predictor == 2) {
          uint32_t prev = i > 0 ? pack_value<BPS>(a, r, i - 1) : 0u;   // the row's first value is stored as it is
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const uint32_t cur = v[j];
            v[j] = (cur - prev) & kMask, prev = cur;
          }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) w4[(j * BPS) >> 2] |= v[j] << (((j * BPS) & 3) * 8);
      }
      *reinterpret_cast<uint4*>(a.dst + at) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
      continue;
    }
    // the value the byte belongs to and the one in front of it, kept while the walk stays on them
    int have = -1, have_prev = -1;
    uint32_t val = 0, val_prev = 0;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    for (int t = 0; t < n; ++t) {
      int sh;                                                 // shift of the byte inside the value
      int ip, shp;                                            // value and shift of the byte this one is differenced against
      bool as_is;                                             // no byte in front of it
      if (a.predictor == 3) {
        sh = 8 * (BPS - 1 - k);
        as_is = o == 0;
        if (i > 0) ip = i - 1, shp = sh;
        else ip = wc - 1, shp = sh + 8;                       // the last byte of the plane in front
      } else {
        sh = 8 * k;
        as_is = a.predictor == 1 || i == 0;
        ip = i - 1, shp = sh;
      }
      if (i != have) {
        if (i == have_prev) {
          const uint32_t tv = val; val = val_prev, val_prev = tv;
          const int ti = have; have = have_prev, have_prev = ti;
        } else {
          val_prev = val, have_prev = have;
          val = pack_value<BPS>(a, r, i), have = i;
        }
      }
      uint32_t byte;
      if (a.predictor == 3) {
        byte = (val >> sh) & 0xffu;
        if (!as_is) {
          if (ip != have_prev) val_prev = pack_value<BPS>(a, r, ip), have_prev = ip;
          byte = (byte - ((val_prev >> shp) & 0xffu)) & 0xffu;
        }
      } else {
        uint32_t d = val;
        if (!as_is) {
          if (ip != have_prev) val_prev = pack_value<BPS>(a, r, ip), have_prev = ip;
          d = (val - val_prev) & kMask;
        }
        byte = (d >> sh) & 0xffu;
      }
      word[t >> 2] |= byte << ((t & 3) * 8);
      if (a.predictor == 3) {
        if (++i == wc) i = 0, ++k;
      } else if (++k == BPS) {
        k = 0, ++i;
      }
      if (++o == (int)a.row_bytes) {                          // the group runs on into the next row
        o = i = k = 0, ++q;
        if (q < a.n_rows) r = pack_row(a, q);
        have = have_prev = -1;
      }
    }
    if (n == 16) {
      *reinterpret_cast<uint4*>(a.dst + at) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
      for (int t = 0; t < n; ++t) a.dst[at + t] = (unsigned char)(word[t >> 2] >> ((t & 3) * 8));
    }
  }
}

// Every check before the launch.  The kernels compute offsets into dst from the layout alone, and n_bytes == the layout's
// arithmetic total is what keeps their stores inside dst; their loads stay inside the raster the three strides describe
// (band < samples, row < height, column < width: indices are clamped to the image).
int launch_tiff_pack(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, const fu_tiff_layout& L,
                     uint8_t* dst, int64_t n_bytes, hipStream_t s) {
  const char* fn = "fu_tiff_pack";
  FU_REQUIRE(src && dst, "%s: null src / dst", fn);
  FU_REQUIRE(L.width >= 1 && L.height >= 1 && (int64_t)L.width * L.height <= FU_MAP_MAX_PIXELS,
             "%s: image %dx%d is empty or has more than 2^28 pixels", fn, L.height, L.width);
  FU_REQUIRE(L.samples >= 1 && L.samples <= FU_TIFF_MAX_BANDS, "%s: samples = %d not in 1..%d", fn, L.samples,
             FU_TIFF_MAX_BANDS);
  const int bps = L.bytes_per_sample;
  FU_REQUIRE(bps == 1 || bps == 2 || bps == 4, "%s: bytes_per_sample = %d is not 1, 2 or 4", fn, bps);
  FU_REQUIRE(L.sample_kind == FU_TIFF_UINT || L.sample_kind == FU_TIFF_INT || L.sample_kind == FU_TIFF_FLOAT,
             "%s: unknown sample_kind %d", fn, L.sample_kind);
  FU_REQUIRE(L.sample_kind != FU_TIFF_FLOAT || bps == 4, "%s: %d-byte float samples", fn, bps);
  FU_REQUIRE(L.big_endian == 0, "%s: big-endian output is not supported", fn);
  FU_REQUIRE(L.samples == 1 || L.planar != 0, "%s: chunky output of %d samples is not supported (planar-separate only)", fn,
             L.samples);
  FU_REQUIRE(L.predictor >= 1 && L.predictor <= 3, "%s: predictor %d is not 1, 2 or 3", fn, L.predictor);
  FU_REQUIRE(L.predictor != 3 || L.sample_kind == FU_TIFF_FLOAT, "%s: predictor 3 (floating point) on integer samples", fn);
  FU_REQUIRE(L.predictor != 2 || L.sample_kind != FU_TIFF_FLOAT, "%s: predictor 2 (horizontal differencing) on float samples",
             fn);
  FU_REQUIRE(L.seg_w >= 1 && L.seg_h >= 1 && (int64_t)L.seg_w * L.seg_h <= FU_MAP_MAX_PIXELS,
             "%s: segment %dx%d is empty or has more than 2^28 pixels", fn, L.seg_h, L.seg_w);
  if (L.tiled)
    FU_REQUIRE(L.seg_w % 16 == 0 && L.seg_h % 16 == 0, "%s: tile sides %dx%d are not multiples of 16", fn, L.seg_h, L.seg_w);
  else
    FU_REQUIRE(L.seg_w == L.width, "%s: strips are as wide as the image (seg_w %d, width %d)", fn, L.seg_w, L.width);
  FU_REQUIRE(reinterpret_cast<uintptr_t>(src) % bps == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0,
             "%s: misaligned src (the sample size) / dst (16 bytes)", fn);
  FU_REQUIRE(band_stride >= 0 && row_stride >= 0 && col_stride >= 0, "%s: negative source stride", fn);
  TiffPack a{};
  a.src = static_cast<const unsigned char*>(src), a.dst = dst;
  a.band_stride = band_stride, a.row_stride = row_stride, a.col_stride = col_stride;
  a.width = L.width, a.height = L.height, a.seg_w = L.seg_w, a.seg_h = L.seg_h, a.tiled = L.tiled != 0;
  a.predictor = L.predictor;
  a.row_bytes = (int64_t)L.seg_w * bps;
  if (a.tiled) {
    a.tiles_across = (int)ceil_div64(L.width, L.seg_w), a.tiles_down = (int)ceil_div64(L.height, L.seg_h);
    a.n_rows = (int64_t)L.samples * a.tiles_across * a.tiles_down * L.seg_h;
  } else {
    a.tiles_across = a.tiles_down = 1;
    a.n_rows = (int64_t)L.samples * L.height;                 // strips at nominal size are the plane's rows in order
  }
  const int64_t total = a.n_rows * a.row_bytes;
  FU_REQUIRE(n_bytes == total, "%s: n_bytes = %lld, the layout holds %lld", fn, (long long)n_bytes, (long long)total);
  a.n_bytes = n_bytes;
  const dim3 block(256);
  if (L.seg_w % 16 == 0) {
    const dim3 grid(grid_for(a.n_rows * (L.seg_w / 16), 256, 16384));
    switch (bps) {
      case 1: hipLaunchKernelGGL((k_tiff_pack_rows<1>), grid, block, 0, s, a); break;
      case 2: hipLaunchKernelGGL((k_tiff_pack_rows<2>), grid, block, 0, s, a); break;
      default: hipLaunchKernelGGL((k_tiff_pack_rows<4>), grid, block, 0, s, a); break;
    }
  } else {
    const dim3 grid(grid_for((n_bytes + 15) / 16, 256, 16384));
    switch (bps) {
      case 1: hipLaunchKernelGGL((k_tiff_pack_groups<1>), grid, block, 0, s, a); break;
      case 2: hipLaunchKernelGGL((k_tiff_pack_groups<2>), grid, block, 0, s, a); break;
      default: hipLaunchKernelGGL((k_tiff_pack_groups<4>), grid, block, 0, s, a); break;
    }
  }
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
