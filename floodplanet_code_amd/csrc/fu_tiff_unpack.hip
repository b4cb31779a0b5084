// fu_tiff_unpack (gfx950): the entropy-decoded segments of a TIFF -- strips or tiles at their nominal size, back to back in
// the order of the file's offset array -- to the fp32 [n_bands, height, width] raster scene inference uploads today.  One
// launch undoes the predictor, swaps bytes, takes tiles apart, picks bands and converts; datasets/geotiff.py holds the numpy
// statement (read_raster), and every comparison against it is equality of bits.
//
// Decomposition.  The unit of work is one row of one segment, taken by one wave: a predictor never crosses a segment row,
// so rows are independent, and the rows of a scene (height x tiles across x planes) outnumber the waves of the chip.  A
// wave walks its row in passes of FU_TIFF_UNPACK_CHUNK = 256 pixels, 4 consecutive pixels per lane, and inside a pass
// over the selected bands, so the lines of a chunky row are reused from cache while they are hot (a chunky pixel of 16
// bytes -- 8 x uint16, 4 x float32 -- is read with one 16-byte load for all its bands).  Per band and pass:
// load, a serial prefix over the lane's 4 values, a wave-level inclusive scan of the lane totals (__shfl_up, 6 steps),
// plus the carry of the passes before, which is kept per band in LDS (one cell per wave and band slot, written and read
// by the same wave).  Both predictors are the same scan with another addition: horizontal differencing adds modulo
// 2^bits, the floating-point predictor adds byte-wise modulo 2^8 on the bytes of a value gathered from its byte planes
// (most significant first), with the carry of each plane started at the sum of the planes in front of it -- which needs
// the plane totals, a first walk over the row with a wave reduction.  The sums are associative, so scan order does not
// change a bit.  Stores: a lane owns 4 consecutive floats of one output row, 16 bytes where aligned; no atomics.
#include "fu_common.h"
#include "../../include/floodunet.h"

#include <stdint.h>
#include <type_traits>

namespace fu {

constexpr int kUnpackLaneValues = 4;
static_assert(FU_TIFF_UNPACK_CHUNK == 64 * kUnpackLaneValues, "a pass is one wave of 4-pixel lanes");

struct TiffUnpack {
  const unsigned char* src;   // the decoded segments
  uint32_t* out;              // fp32 bits [n_bands, height, width]
  int width, height, n_bands;
  int spp_seg;                // samples per pixel inside a segment: samples when chunky, 1 when planar
  int kind, big_endian, planar, tiled, seg_w, seg_h, predictor;
  int tiles_across;           // 1 for strips
  int rows_grid;              // segment rows per plane: tiles down * seg_h, or height for strips
  int64_t n_rows;             // planes * rows_grid * tiles_across: the wave's work items
  int64_t seg_bytes;          // bytes of a tile (tiled only)
  int64_t row_bytes;          // bytes of a segment row
  int vec_pixels;             // a pixel of the segment is 16 bytes, 16-byte aligned, and stored as values: one load per pixel
  int bands[FU_TIFF_MAX_BANDS];
};

// float64 bits -> float32 bits, round to nearest even, subnormal results kept, in integer arithmetic (no dependence on the
// float mode).  A NaN stays a NaN (sign, quiet bit, the payload's top bits).
__device__ __forceinline__ uint32_t f64_bits_to_f32_bits(uint64_t u) {
  const uint32_t sign = (uint32_t)(u >> 32) & 0x80000000u;
  const int exp = (int)((u >> 52) & 0x7ffu);
  const uint64_t man = u & 0xfffffffffffffull;
  if (exp == 0x7ff) return man ? (sign | 0x7fc00000u | (uint32_t)(man >> 29)) : (sign | 0x7f800000u);
  if (exp == 0) return sign;                                  // float64 zero / subnormal: far below float32's range
  const int e = exp - 1023 + 127;
  if (e >= 255) return sign | 0x7f800000u;
  if (e <= 0) {                                               // float32 subnormal (or zero): shift the full significand
    const int shift = 29 + 1 - e;
    if (shift > 63) return sign;
    const uint64_t m = man | (1ull << 52);
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1ull))) ++q;
    return sign | (uint32_t)q;                                // q == 2^23 is the smallest normal: the encoding is right
  }
  uint32_t q = ((uint32_t)e << 23) | (uint32_t)(man >> 29);
  const uint32_t rem = (uint32_t)man & 0x1fffffffu;
  if (rem > 0x10000000u || (rem == 0x10000000u && (q & 1u))) ++q;   // a carry runs into the exponent, up to infinity
  return sign | q;
}

// the raw value (BPS bytes, in T) -> the fp32 bits of np.float32(value)
template <typename T, int BPS>
__device__ __forceinline__ uint32_t unpack_convert(T v, int kind) {
  if (kind == FU_TIFF_FLOAT) {
    if (BPS == 8) return f64_bits_to_f32_bits((uint64_t)v);
    return (uint32_t)v;                                       // float32: a bit copy, NaN payloads included
  }
  if (kind == FU_TIFF_INT) {
    if (BPS == 1) return __float_as_uint((float)(int)(int8_t)(uint8_t)v);
    if (BPS == 2) return __float_as_uint((float)(int)(int16_t)(uint16_t)v);
    if (BPS == 4) return __float_as_uint((float)(int32_t)(uint32_t)v);
    return __float_as_uint((float)(long long)(uint64_t)v);
  }
  if (BPS == 1) return __float_as_uint((float)(uint32_t)(uint8_t)v);
  if (BPS == 2) return __float_as_uint((float)(uint32_t)(uint16_t)v);
  if (BPS == 4) return __float_as_uint((float)(uint32_t)v);
  return __float_as_uint((float)(unsigned long long)v);
}

// a + b: modulo 2^bits of T (the caller truncates to the sample's width), or byte-wise modulo 2^8
template <typename T>
__device__ __forceinline__ T unpack_add(T a, T b, bool bytewise) {
  if (!bytewise) return (T)(a + b);
  const T hi = (T)0x8080808080808080ull, lo = (T)~hi;
  return (T)((((a & lo) + (b & lo))) ^ ((a ^ b) & hi));
}

__device__ __forceinline__ uint32_t unpack_shfl_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ uint64_t unpack_shfl_up(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t unpack_shfl(uint32_t v, int l) { return (uint32_t)__shfl((int)v, l, 64); }
__device__ __forceinline__ uint64_t unpack_shfl(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, l, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), l, 64);
  return ((uint64_t)hi << 32) | lo;
}

// value (x, c) of a segment row, as stored: byte-swapped to native order, or under the floating-point predictor gathered
// from the row's byte planes, most significant first (in both file byte orders).  wc: values per row.
template <typename T, int BPS>
__device__ __forceinline__ T unpack_load(const unsigned char* __restrict__ row, int x, int c, int spp, int64_t wc, bool planes,
                                         bool big_endian) {
  const int64_t i = (int64_t)x * spp + c;
  if (planes) {
    T v = 0;
#pragma unroll
    for (int b = 0; b < BPS; ++b) v = (T)((v << (BPS > 1 ? 8 : 0)) | row[b * wc + i]);
    return v;
  }
  const unsigned char* q = row + i * BPS;
  if (BPS == 1) return (T)*q;
  if (BPS == 2) {
    const uint16_t v = *reinterpret_cast<const uint16_t*>(q);
    return (T)(big_endian ? __builtin_bswap16(v) : v);
  }
  if (BPS == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(q);
    return (T)(big_endian ? __builtin_bswap32(v) : v);
  }
  const uint64_t v = *reinterpret_cast<const uint64_t*>(q);
  return (T)(big_endian ? __builtin_bswap64(v) : v);
}

// one 32-bit word of a pixel held in registers, by a wave-uniform index: selects, not an indexed register file
__device__ __forceinline__ uint32_t unpack_pick(const uint32_t (&p)[4], int k) {
  return k == 0 ? p[0] : k == 1 ? p[1] : k == 2 ? p[2] : p[3];
}

// value c of a 16-byte pixel in registers, byte-swapped to native order
template <typename T, int BPS>
__device__ __forceinline__ T unpack_from_pixel(const uint32_t (&p)[4], int c, bool big_endian) {
  const int off = c * BPS;                                    // byte offset inside the pixel
  if (BPS == 8) {
    const uint64_t v = ((uint64_t)unpack_pick(p, (off >> 2) + 1) << 32) | unpack_pick(p, off >> 2);
    return (T)(big_endian ? __builtin_bswap64(v) : v);
  }
  const uint32_t w = unpack_pick(p, off >> 2);
  if (BPS == 4) return (T)(big_endian ? __builtin_bswap32(w) : w);
  if (BPS == 2) {
    const uint16_t h = (uint16_t)(w >> ((off & 2) * 8));
    return (T)(big_endian ? __builtin_bswap16(h) : h);
  }
  return (T)((w >> ((off & 3) * 8)) & 0xffu);
}

template <typename T, int BPS>
__global__ __launch_bounds__(256) void k_tiff_unpack(const TiffUnpack a) {
  __shared__ T s_carry[4][FU_TIFF_MAX_BANDS];                 // per wave and band slot: the scan's carry along the row
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, n_waves = (int64_t)gridDim.x * 4;
  const bool planes = a.predictor == 3, scan = a.predictor != 1;
  const int spp = a.spp_seg;
  const int64_t wc = (int64_t)a.seg_w * spp;
  for (int64_t q = wave0; q < a.n_rows; q += n_waves) {       // everything below is uniform over the wave
    const int tx = (int)(q % a.tiles_across);
    const int64_t t = q / a.tiles_across;
    const int y = (int)(t % a.rows_grid), p = (int)(t / a.rows_grid);
    if (y >= a.height) continue;                              // the rows of an edge tile below the image
    const int x_img = tx * a.seg_w;
    const int nx = min(a.seg_w, a.width - x_img);             // the row's pixels inside the image
    const unsigned char* __restrict__ row;
    if (a.tiled) {
      const int ty = y / a.seg_h, r = y - ty * a.seg_h;
      const int64_t seg = ((int64_t)p * (a.rows_grid / a.seg_h) + ty) * a.tiles_across + tx;
      row = a.src + seg * a.seg_bytes + (int64_t)r * a.row_bytes;
    } else {
      row = a.src + ((int64_t)p * a.height + y) * a.row_bytes;  // strips at nominal size are the plane's rows in order
    }
    if (scan) {
      for (int n = 0; n < a.n_bands; ++n) {
        if (a.planar && a.bands[n] != p) continue;
        T start = 0;
        if (planes) {
          // plane totals over the WHOLE segment row (the part of an edge tile outside the image included), then the start
          // of plane b = the sum of the planes in front of it: total >> 8k lands plane b - k's total on plane b
          const int c = a.planar ? 0 : a.bands[n];
          T tot = 0;
          for (int x = lane; x < a.seg_w; x += 64)
            tot = unpack_add<T>(tot, unpack_load<T, BPS>(row, x, c, spp, wc, true, false), true);
          for (int o = 32; o > 0; o >>= 1) tot = unpack_add<T>(tot, unpack_shfl(tot, lane ^ o), true);
#pragma unroll
          for (int k = 1; k < BPS; ++k) start = unpack_add<T>(start, (T)(tot >> (8 * k)), true);
        }
        s_carry[w][n] = start;
      }
    }
    for (int x0 = 0; x0 < nx; x0 += FU_TIFF_UNPACK_CHUNK) {
      const int x = x0 + lane * kUnpackLaneValues;
      // a chunky pixel of 16 bytes (8 x uint16, 4 x float32, ...): the lane's 4 pixels are 4 16-byte loads, read once for
      // all bands, in place of one narrow strided load per band and pixel
      uint32_t px[kUnpackLaneValues][4];
      if (a.vec_pixels) {
#pragma unroll
        for (int j = 0; j < kUnpackLaneValues; ++j) {
          uint4 t = make_uint4(0u, 0u, 0u, 0u);
          if (x + j < nx) t = *reinterpret_cast<const uint4*>(row + (int64_t)(x + j) * 16);
          px[j][0] = t.x, px[j][1] = t.y, px[j][2] = t.z, px[j][3] = t.w;
        }
      }
      for (int n = 0; n < a.n_bands; ++n) {
        const int band = a.bands[n];
        if (a.planar && band != p) continue;
        const int c = a.planar ? 0 : band;
        T v[kUnpackLaneValues];
        if (a.vec_pixels) {
#pragma unroll
          for (int j = 0; j < kUnpackLaneValues; ++j) v[j] = unpack_from_pixel<T, BPS>(px[j], c, a.big_endian != 0);
        } else {
#pragma unroll
          for (int j = 0; j < kUnpackLaneValues; ++j)
            v[j] = x + j < nx ? unpack_load<T, BPS>(row, x + j, c, spp, wc, planes, a.big_endian != 0) : (T)0;
        }
        if (scan) {
#pragma unroll
          for (int j = 1; j < kUnpackLaneValues; ++j) v[j] = unpack_add<T>(v[j - 1], v[j], planes);
          T s = v[kUnpackLaneValues - 1];                     // inclusive scan of the lane totals over the wave
          for (int d = 1; d < 64; d <<= 1) {
            const T up = unpack_shfl_up(s, d);
            if (lane >= d) s = unpack_add<T>(s, up, planes);
          }
          T before = unpack_shfl_up(s, 1);
          if (lane == 0) before = 0;
          const T carry = s_carry[w][n];
          before = unpack_add<T>(carry, before, planes);
#pragma unroll
          for (int j = 0; j < kUnpackLaneValues; ++j) v[j] = unpack_add<T>(before, v[j], planes);
          s_carry[w][n] = unpack_add<T>(carry, unpack_shfl(s, 63), planes);
        }
        if (x < nx) {
          uint32_t* o = a.out + ((int64_t)n * a.height + y) * a.width + x_img + x;
          uint32_t f[kUnpackLaneValues];
#pragma unroll
          for (int j = 0; j < kUnpackLaneValues; ++j) f[j] = unpack_convert<T, BPS>(v[j], a.kind);
          if (x + kUnpackLaneValues <= nx && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            *reinterpret_cast<uint4*>(o) = make_uint4(f[0], f[1], f[2], f[3]);
          } else {
#pragma unroll
            for (int j = 0; j < kUnpackLaneValues; ++j)
              if (x + j < nx) o[j] = f[j];
          }
        }
      }
    }
  }
}

// Every check before the launch: the kernel computes offsets into the caller's buffers from the layout alone, and n_bytes
// == the layout's arithmetic total is what keeps its reads inside src; its writes stay inside [n_bands, height, width].
int launch_tiff_unpack(const uint8_t* src, int64_t n_bytes, const fu_tiff_layout& L, const int32_t* bands, int n_bands,
                       float* out, hipStream_t s) {
  const char* fn = "fu_tiff_unpack";
  FU_REQUIRE(src && bands && out, "%s: null src / bands / out", fn);
  FU_REQUIRE(reinterpret_cast<uintptr_t>(src) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
             "%s: misaligned src (8 bytes) / out (4 bytes)", fn);
  FU_REQUIRE(L.width >= 1 && L.height >= 1 && (int64_t)L.width * L.height <= FU_MAP_MAX_PIXELS,
             "%s: image %dx%d is empty or has more than 2^28 pixels", fn, L.height, L.width);
  FU_REQUIRE(L.samples >= 1 && L.samples <= 64, "%s: samples = %d not in 1..64", fn, L.samples);
  const int bps = L.bytes_per_sample;
  FU_REQUIRE(bps == 1 || bps == 2 || bps == 4 || bps == 8, "%s: bytes_per_sample = %d is not 1, 2, 4 or 8", fn, bps);
  FU_REQUIRE(L.sample_kind == FU_TIFF_UINT || L.sample_kind == FU_TIFF_INT || L.sample_kind == FU_TIFF_FLOAT,
             "%s: unknown sample_kind %d", fn, L.sample_kind);
  FU_REQUIRE(L.sample_kind != FU_TIFF_FLOAT || bps >= 4, "%s: %d-byte float samples", fn, bps);
  FU_REQUIRE(L.predictor >= 1 && L.predictor <= 3, "%s: predictor %d is not 1, 2 or 3", fn, L.predictor);
  FU_REQUIRE(L.predictor != 3 || L.sample_kind == FU_TIFF_FLOAT, "%s: predictor 3 (floating point) on integer samples", fn);
  FU_REQUIRE(L.predictor != 2 || L.sample_kind != FU_TIFF_FLOAT, "%s: predictor 2 (horizontal differencing) on float samples",
             fn);
  FU_REQUIRE(L.seg_w >= 1 && L.seg_h >= 1 && (int64_t)L.seg_w * L.seg_h <= FU_MAP_MAX_PIXELS,
             "%s: segment %dx%d is empty or has more than 2^28 pixels", fn, L.seg_h, L.seg_w);
  FU_REQUIRE(L.tiled || L.seg_w == L.width, "%s: strips are as wide as the image (seg_w %d, width %d)", fn, L.seg_w, L.width);
  FU_REQUIRE(n_bands >= 1 && n_bands <= FU_TIFF_MAX_BANDS, "%s: n_bands = %d not in 1..%d", fn, n_bands, FU_TIFF_MAX_BANDS);
  for (int n = 0; n < n_bands; ++n)
    FU_REQUIRE(bands[n] >= 0 && bands[n] < L.samples, "%s: band index %d (slot %d) not in 0..%d", fn, (int)bands[n], n,
               L.samples - 1);
  TiffUnpack a{};
  a.src = src, a.out = reinterpret_cast<uint32_t*>(out);
  a.width = L.width, a.height = L.height, a.n_bands = n_bands;
  a.planar = L.planar != 0 && L.samples > 1, a.tiled = L.tiled != 0;
  a.spp_seg = a.planar ? 1 : L.samples;
  a.kind = L.sample_kind, a.big_endian = L.big_endian != 0, a.seg_w = L.seg_w, a.seg_h = L.seg_h, a.predictor = L.predictor;
  const int64_t n_planes = a.planar ? L.samples : 1;
  a.row_bytes = (int64_t)L.seg_w * a.spp_seg * bps;
  int64_t total;
  if (a.tiled) {
    const int64_t across = ceil_div64(L.width, L.seg_w), down = ceil_div64(L.height, L.seg_h);
    a.tiles_across = (int)across, a.rows_grid = (int)(down * L.seg_h);
    a.seg_bytes = a.row_bytes * L.seg_h;
    FU_REQUIRE(down * L.seg_h <= INT32_MAX, "%s: %lld tile rows", fn, (long long)(down * L.seg_h));
    total = n_planes * across * down * a.seg_bytes;
  } else {
    a.tiles_across = 1, a.rows_grid = L.height, a.seg_bytes = 0;
    total = n_planes * L.height * a.row_bytes;
  }
  FU_REQUIRE(n_bytes == total, "%s: n_bytes = %lld, the layout holds %lld", fn, (long long)n_bytes, (long long)total);
  a.n_rows = n_planes * a.rows_grid * a.tiles_across;
  // (segment and row sizes are then multiples of 16 bytes, so every pixel is aligned as src is)
  a.vec_pixels = a.spp_seg * bps == 16 && L.predictor != 3 && reinterpret_cast<uintptr_t>(src) % 16 == 0;
  for (int n = 0; n < n_bands; ++n) a.bands[n] = bands[n];
  const dim3 grid(grid_for(a.n_rows, 4, 2048)), block(256);
  switch (bps) {
    case 1: hipLaunchKernelGGL((k_tiff_unpack<uint32_t, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_tiff_unpack<uint32_t, 2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_tiff_unpack<uint32_t, 4>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_tiff_unpack<uint64_t, 8>), grid, block, 0, s, a); break;
  }
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
