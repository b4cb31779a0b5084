// Streaming per-band statistics of tiles in HBM (gfx950; fu_band_stats): the kernel, its two folds and their launcher.
#include "fu_data.h"

namespace fu {

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
