// Nodata in scene inference (gfx950): which pixels of a resident scene hold data, and how many of them every crop box
// holds.  fu_scene_valid_mask derives the mask from the uploaded raster (datasets/valid_mask.py holds the numpy
// statements: source_valid_host, then grid_valid_host); fu_mask_box_counts is the census of a table of boxes
// (box_valid_counts_host), the twin of fu_label_box_counts.  Integer results throughout: every comparison against the host
// statements is equality.  The masked finalisation that consumes the mask is in fu_eval.hip.
#include "fu_data.h"

#include <algorithm>
#include <vector>

namespace fu {

// ------------------------------------------------------------------------------------------------
// Source pass: src_valid[p] = every band finite and not every band == nodata (fp32 ==), over the npix = src_h * src_w
// pixels of a [C, src_h, src_w] raster.  Memory bound, every element read once: a thread takes 4 consecutive pixels -- one
// 16-byte load per band, one 4-byte store of the mask -- between a misaligned head and a tail that run one pixel at a
// time (as k_stitch_finalize_maps); bands that are not aligned alike (npix % 4 != 0 with C > 1), or a mask that is not,
// are accessed one element at a time inside the groups too.
// ------------------------------------------------------------------------------------------------
struct SourceValid {
  const float* raster;      // [C, npix]
  unsigned char* out;       // [npix]
  int64_t npix, head;       // head: the pixels in front of band 0's first 16-byte boundary (npix: no groups at all)
  int C, use_nodata;
  float nodata;
  int vec_in, vec_out;      // the bands / the mask are aligned for the group's wide access
};

// fold band value x into the pixel's two flags: every band finite so far, every band == nodata so far
__device__ __forceinline__ void source_valid_fold(float x, float nodata, bool& finite, bool& fill) {
  finite = finite && fabsf(x) < INFINITY;     // false for NaN too
  fill = fill && x == nodata;
}

__global__ __launch_bounds__(256) void k_source_valid(const SourceValid a) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = (a.npix - a.head) / 4;
  for (int64_t j = tid; j < nvec; j += nthr) {
    const int64_t p = a.head + 4 * j;
    bool finite[4] = {true, true, true, true};
    bool fill[4] = {a.use_nodata != 0, a.use_nodata != 0, a.use_nodata != 0, a.use_nodata != 0};
    for (int c = 0; c < a.C; ++c) {
      const float* band = a.raster + (int64_t)c * a.npix + p;
      float x[4];
      if (a.vec_in) {
        const float4 t = *reinterpret_cast<const float4*>(band);
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = band[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) source_valid_fold(x[q], a.nodata, finite[q], fill[q]);
    }
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m |= (finite[q] && !fill[q] ? 1u : 0u) << (8 * q);
    if (a.vec_out) {
      *reinterpret_cast<unsigned*>(a.out + p) = m;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a.out[p + q] = (unsigned char)(m >> (8 * q));
    }
  }
  const int64_t tail0 = a.head + 4 * nvec, nrest = a.head + (a.npix - tail0);   // misaligned head and tail: plain code
  for (int64_t r = tid; r < nrest; r += nthr) {
    const int64_t p = r < a.head ? r : tail0 + (r - a.head);
    bool finite = true, fill = a.use_nodata != 0;
    for (int c = 0; c < a.C; ++c) source_valid_fold(a.raster[(int64_t)c * a.npix + p], a.nodata, finite, fill);
    a.out[p] = finite && !fill ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------
// Grid pass: valid[Y, X] = AND of src_valid[iy[Y, a], ix[X, b]] over the tap pairs with wy[Y, a] != 0 and wx[X, b] != 0
// (the tables of fu_resize_lanczos4_tiles for the whole grid), one grid pixel per thread, direct reads: the byte mask is
// C * 4 times smaller than the raster and its 8 x 8 neighbourhoods are re-read from cache; with identity tables it is one
// read.  A tap index is clamped into the source before it is used, so a table can not send a read out of bounds.  The
// loop's trip count is the same for every lane of a wave, so the count can be taken with a ballot: lane 0 of each wave
// adds the wave's population count to one LDS cell, and the workgroup finishes with ONE 64-bit integer atomic into
// n_valid (zeroed by the launcher on the same stream): exact and order-free.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_grid_valid(const unsigned char* __restrict__ src_valid, int src_h, int src_w,
                                                    const int* __restrict__ iy, const float* __restrict__ wy,
                                                    const int* __restrict__ ix, const float* __restrict__ wx, int grid_w,
                                                    int64_t npix, unsigned char* __restrict__ valid,
                                                    unsigned long long* __restrict__ n_valid) {
  __shared__ unsigned int block_count;
  if (threadIdx.x == 0) block_count = 0u;
  __syncthreads();
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p0 = (int64_t)blockIdx.x * blockDim.x; p0 < npix; p0 += nthr) {   // uniform trips: the ballot below
    const int64_t p = p0 + threadIdx.x;
    bool ok = false;
    if (p < npix) {
      const int Y = (int)(p / grid_w), X = (int)(p - (int64_t)Y * grid_w);
      ok = true;
      int xs[8];
      unsigned xmask = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        xs[b] = min(max(ix[X * 8 + b], 0), src_w - 1);
        xmask |= (wx[X * 8 + b] != 0.f ? 1u : 0u) << b;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (wy[Y * 8 + t] == 0.f) continue;
        const unsigned char* row = src_valid + (int64_t)min(max(iy[Y * 8 + t], 0), src_h - 1) * src_w;
#pragma unroll
        for (int b = 0; b < 8; ++b)
          if ((xmask >> b) & 1u) ok = ok && row[xs[b]] == 1;
      }
      valid[p] = ok ? 1 : 0;
    }
    const unsigned long long wave = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && wave) atomicAdd(&block_count, (unsigned int)__popcll(wave));
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_count) atomicAdd(n_valid, (unsigned long long)block_count);
}

// fu_scene_valid_mask: every check before anything is launched; two launches behind the memset of n_valid's cell
int launch_scene_valid_mask(const float* raster, int C, int src_h, int src_w, bool use_nodata, float nodata, const int* iy,
                            const float* wy, const int* ix, const float* wx, int grid_h, int grid_w,
                            unsigned char* src_valid, unsigned char* valid, int64_t* n_valid, hipStream_t s) {
  const char* fn = "fu_scene_valid_mask";
  FU_REQUIRE(raster && iy && wy && ix && wx && src_valid && valid && n_valid, "%s: null argument", fn);
  FU_REQUIRE(C >= 1 && C <= 16, "%s: C = %d not in 1..16", fn, C);
  FU_REQUIRE(src_h >= 1 && src_w >= 1 && (int64_t)src_h * src_w <= FU_MAP_MAX_PIXELS,
             "%s: source %dx%d is empty or has more than 2^28 pixels", fn, src_h, src_w);
  FU_REQUIRE(grid_h >= 1 && grid_w >= 1 && (int64_t)grid_h * grid_w <= FU_MAP_MAX_PIXELS,
             "%s: grid %dx%d is empty or has more than 2^28 pixels", fn, grid_h, grid_w);
  FU_REQUIRE(!use_nodata || isfinite(nodata), "%s: nodata %g is not finite", fn, (double)nodata);
  FU_REQUIRE(reinterpret_cast<uintptr_t>(raster) % 4 == 0 && reinterpret_cast<uintptr_t>(n_valid) % 8 == 0,
             "%s: misaligned raster / n_valid_out", fn);
  SourceValid a{};
  a.raster = raster, a.out = src_valid, a.npix = (int64_t)src_h * src_w, a.C = C;
  a.use_nodata = use_nodata ? 1 : 0, a.nodata = use_nodata ? nodata : 0.f;
  const uintptr_t ra = reinterpret_cast<uintptr_t>(raster);
  a.head = std::min<int64_t>(a.npix, (int64_t)((16 - ra % 16) % 16) / 4);
  a.vec_in = C == 1 || a.npix % 4 == 0;   // every band's group then starts on a 16-byte boundary, as band 0's do
  a.vec_out = (reinterpret_cast<uintptr_t>(src_valid) + (uintptr_t)a.head) % 4 == 0;
  FU_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int64_t), s));
  hipLaunchKernelGGL(k_source_valid, dim3(grid_for(ceil_div64(a.npix, 4), 256, 4096)), dim3(256), 0, s, a);
  FU_LAUNCH_CHECK();
  const int64_t gpix = (int64_t)grid_h * grid_w;
  hipLaunchKernelGGL(k_grid_valid, dim3(grid_for(gpix, 256, 8192)), dim3(256), 0, s, src_valid, src_h, src_w, iy, wy, ix,
                     wx, grid_w, gpix, valid, reinterpret_cast<unsigned long long*>(n_valid));
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Census (fu_mask_box_counts): counts[i] = the non-zero bytes of box i of its mask.  One 256-thread workgroup per box owns
// its cell of the output: no global atomic, nothing to zero, no dependence on launch order.  A row of the box is seen as
// the 4-byte aligned words of memory it touches, at most wpr = (dw + 6) / 4 of them (3 bytes of head, then whole words);
// the block's threads stride over the dh * wpr (row, word) pairs.  A word that lies wholly inside the row is one 4-byte
// load, the partial word at either end is read byte by byte, a pair past the row's last word is skipped.  One register per
// thread, a xor tree over the wave, an LDS fold over the four waves, one 64-bit store by thread 0.
// ------------------------------------------------------------------------------------------------
struct MaskBoxJob {          // one box of the table (device copy of a validated fu_mask_box)
  const unsigned char* box;  // the mask at the box's first pixel
  int mask_w, dh, dw, pad;
};

__global__ __launch_bounds__(256) void k_mask_box_counts(const MaskBoxJob* __restrict__ jobs, int64_t* __restrict__ counts) {
  __shared__ unsigned int total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  const MaskBoxJob J = jobs[blockIdx.x];
  const unsigned wpr = ((unsigned)J.dw + 6u) / 4u;
  // dh * dw <= 2^28 (the launcher's check), so dh * wpr <= dh * dw * 7 / 4 < 2^32
  const unsigned n_items = (unsigned)J.dh * wpr;
  unsigned c = 0u;
  for (unsigned i = threadIdx.x; i < n_items; i += 256u) {
    const unsigned y = i / wpr, k = i - y * wpr;
    const unsigned char* __restrict__ row = J.box + (int64_t)y * J.mask_w;
    const int head = (int)(reinterpret_cast<uintptr_t>(row) & 3);   // bytes of the first word that precede the row
    const int x0 = (int)k * 4 - head;                               // the word is row[x0, x0 + 4)
    if (x0 >= J.dw) continue;
    if (x0 >= 0 && x0 + 4 <= J.dw) {
      const unsigned v = *reinterpret_cast<const unsigned*>(row + x0);
#pragma unroll
      for (int b = 0; b < 4; ++b) c += ((v >> (8 * b)) & 0xffu) ? 1u : 0u;
    } else {
      for (int x = max(x0, 0); x < min(x0 + 4, J.dw); ++x) c += row[x] ? 1u : 0u;
    }
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)total;
}

// every check before anything is launched or copied: a rejected call leaves the stream and the counts untouched
int launch_mask_box_counts(DeviceTable& table, int n, const fu_mask_box* entries, int64_t* counts, hipStream_t s) {
  const char* fn = "fu_mask_box_counts";
  FU_REQUIRE(n >= 1, "%s: n = %d (must be >= 1)", fn, n);
  FU_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 8 == 0, "%s: misaligned counts_out", fn);
  std::vector<MaskBoxJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const fu_mask_box& E = entries[i];
    FU_REQUIRE(E.mask, "%s: entry %d: null mask", fn, i);
    FU_REQUIRE(E.mask_h >= 1 && E.mask_w >= 1 && (int64_t)E.mask_h * E.mask_w <= FU_MAP_MAX_PIXELS,
               "%s: entry %d: mask %dx%d is empty or has more than 2^28 pixels", fn, i, E.mask_h, E.mask_w);
    FU_REQUIRE(E.h0 >= 0 && E.w0 >= 0 && E.hE <= E.mask_h && E.wE <= E.mask_w,
               "%s: entry %d: box [%d:%d, %d:%d] lies outside its mask %dx%d", fn, i, E.h0, E.hE, E.w0, E.wE, E.mask_h,
               E.mask_w);
    FU_REQUIRE(E.hE > E.h0 && E.wE > E.w0, "%s: entry %d: box [%d:%d, %d:%d] is empty", fn, i, E.h0, E.hE, E.w0, E.wE);
    jobs[i] = MaskBoxJob{E.mask + (int64_t)E.h0 * E.mask_w + E.w0, E.mask_w, E.hE - E.h0, E.wE - E.w0, 0};
  }
  FU_TRY(table.upload(jobs.data(), (size_t)n * sizeof(MaskBoxJob), sizeof(MaskBoxJob), s));
  hipLaunchKernelGGL(k_mask_box_counts, dim3((unsigned)n), dim3(256), 0, s, static_cast<const MaskBoxJob*>(table.dev),
                     counts);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
