// BatchNorm kernels of the UNet training path (gfx950): forward statistics -> coefficients, and BatchNorm + ReLU backward
// (plain, with the max-pool backward folded in, with the head gradient recomputed).  fp32 math, deterministic two-level
// reductions (per-block partials -> fixed-order finalisation in fp64), wave64 shuffles.
#include "fu_common.h"
#include "fu_elem.h"

namespace fu {

// ------------------------------------------------------------------------------------------------
// two-level per-channel reduction of partials [nPart][C][NV] (fp32) -> [G][C][NV] (fp64)
// ------------------------------------------------------------------------------------------------
static constexpr int RED_GROUPS = 32;

template <int NV>
__global__ void k_partials_reduce(const float* __restrict__ part, double* __restrict__ out, int nPart, int C,
                                  int perGroup) {
  // block: 32 channels x 8 partial lanes; grid (ceil(C/32), G)
  __shared__ double sm[8][32][NV];
  const int cl = threadIdx.x & 31, j = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int g = blockIdx.y;
  const int t0 = g * perGroup;
  const int t1 = min(nPart, t0 + perGroup);
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  if (c < C) {
#pragma unroll 4
    for (int t = t0 + j; t < t1; t += 8) {
      const float* q = part + ((int64_t)t * C + c) * NV;
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] += (double)q[v];
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) sm[j][cl][v] = acc[v];
  __syncthreads();
  if (j == 0 && c < C) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      double s = 0.0;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) s += sm[jj][cl][v];
      out[((int64_t)g * C + c) * NV + v] = s;
    }
  }
}

// scratch for the fp64 second level lives in a static device buffer per call site (passed in)
template <int NV>
static int reduce_partials(const float* part, double* out, int nPart, int C, hipStream_t s, int* groups_out) {
  int G = nPart < RED_GROUPS ? nPart : RED_GROUPS;
  if (G < 1) G = 1;
  const int perGroup = ceil_div(nPart, G);
  G = ceil_div(nPart, perGroup);
  if (G < 1) G = 1;
  hipLaunchKernelGGL(k_partials_reduce<NV>, dim3(ceil_div(C, 32), G), dim3(256), 0, s, part, out, nPart, C, perGroup);
  FU_LAUNCH_CHECK();
  *groups_out = G;
  return 0;
}

// lane g of a 32-lane group fetches group g's fp64 partial pair of channel c (one memory latency instead of a G-long
// dependent chain), then a fixed xor tree; true on the one lane per channel that carries on with the totals
__device__ __forceinline__ bool channel_totals(const double* __restrict__ dpart, int G, int C, int* c_out, double* S, double* Q) {
  const int g = threadIdx.x & 31;
  const int c = blockIdx.x * 8 + (threadIdx.x >> 5);      // 8 channels per block
  const bool ok = c < C && g < G;
  *S = half_wave_sum(ok ? dpart[((int64_t)g * C + c) * 2 + 0] : 0.0);
  *Q = half_wave_sum(ok ? dpart[((int64_t)g * C + c) * 2 + 1] : 0.0);
  *c_out = c;
  return c < C && g == 0;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm forward statistics -> coefficients (bn_fwd_finish, fu_elem.h), second level of the two-launch form
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_finalize(const double* __restrict__ dpart, int G, int C, double count, BnFwdOut o) {
  int c;
  double S, Q;
  if (channel_totals(dpart, G, C, &c, &S, &Q)) bn_fwd_finish(S, Q, count, c, o);
}

// the same for the backward sums (bn_bwd_finish)
__global__ __launch_bounds__(256) void k_bn_bwd_finalize(const double* __restrict__ dpart, int G, int C, double count,
                                                         double grad_share, BnBwdOut o) {
  int c;
  double S1, S2;
  if (channel_totals(dpart, G, C, &c, &S1, &S2)) bn_bwd_finish(S1, S2, count, grad_share, c, o);
}

// ------------------------------------------------------------------------------------------------
// One launch per BatchNorm instead of two (k_partials_reduce + finalize): per-CHANNEL parallelism.  Channels are
// independent, so a block that owns 4 channels can reduce ALL their tile partials ([nPart][C][2] fp32, 32 contiguous
// bytes per tile and block) and finalise them itself -- no second level across blocks, no inter-block hand-off.  128 tile
// lanes x 2 float4 columns; fp64 accumulation; lanes meet in LDS and are summed in a fixed order (deterministic).
// MODE 0: forward statistics -> mean / invstd / a / b (+ running statistics); MODE 1: backward sums -> dgamma / dbeta / coef.
// (The exact data-parallel mode exchanges the partials between the two levels and keeps the two-launch form.)
// ------------------------------------------------------------------------------------------------
template <int MODE, typename OUT>
__global__ __launch_bounds__(256) void k_bn_stats_fused(const float* __restrict__ part, int nPart, int C, double count,
                                                        OUT o) {
  __shared__ double sm[128][8];
  const int col = threadIdx.x & 1, tl = threadIdx.x >> 1;
  const int c0 = blockIdx.x * 4;                        // C % 4 == 0
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  const float* base = part + (size_t)c0 * 2 + col * 4;
  int t = tl;
  for (; t + 3 * 128 < nPart; t += 4 * 128) {           // four independent 16-byte loads in flight per thread
    const float4 v0 = *reinterpret_cast<const float4*>(base + (size_t)t * C * 2);
    const float4 v1 = *reinterpret_cast<const float4*>(base + (size_t)(t + 128) * C * 2);
    const float4 v2 = *reinterpret_cast<const float4*>(base + (size_t)(t + 256) * C * 2);
    const float4 v3 = *reinterpret_cast<const float4*>(base + (size_t)(t + 384) * C * 2);
    a0 += ((double)v0.x + (double)v1.x) + ((double)v2.x + (double)v3.x);
    a1 += ((double)v0.y + (double)v1.y) + ((double)v2.y + (double)v3.y);
    a2 += ((double)v0.z + (double)v1.z) + ((double)v2.z + (double)v3.z);
    a3 += ((double)v0.w + (double)v1.w) + ((double)v2.w + (double)v3.w);
  }
  for (; t < nPart; t += 128) {
    const float4 v0 = *reinterpret_cast<const float4*>(base + (size_t)t * C * 2);
    a0 += (double)v0.x; a1 += (double)v0.y; a2 += (double)v0.z; a3 += (double)v0.w;
  }
  sm[tl][col * 4 + 0] = a0; sm[tl][col * 4 + 1] = a1; sm[tl][col * 4 + 2] = a2; sm[tl][col * 4 + 3] = a3;
  __syncthreads();
  // 8 values (4 channels x 2) x 16 lanes each: lane j sums tile lanes j, j+16, ... (8 adds), then a fixed xor tree
  const int v = threadIdx.x >> 4, j = threadIdx.x & 15;
  double s = 0.0;
  if (v < 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s += sm[j + 16 * k][v];
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  __syncthreads();
  if (v < 8 && j == 0) sm[0][v] = s;
  __syncthreads();
  if (threadIdx.x >= 4) return;
  const int c = c0 + threadIdx.x;
  const double S = sm[0][threadIdx.x * 2 + 0], Q = sm[0][threadIdx.x * 2 + 1];
  if constexpr (MODE == 0) bn_fwd_finish(S, Q, count, c, o);
  else bn_bwd_finish(S, Q, count, 1.0, c, o);
}

int launch_bn_finalize(const BnFwdOut& o, const float* partials, int nTiles, int C, int64_t count, double* dscratch,
                       const SyncDesc* sync, hipStream_t s) {
  const int world = sync_world(sync);
  if (world <= 1 && C % 4 == 0) {
    hipLaunchKernelGGL((k_bn_stats_fused<0, BnFwdOut>), dim3(C / 4), dim3(256), 0, s, partials, nTiles, C, (double)count, o);
    FU_LAUNCH_CHECK();
    return 0;
  }
  int G = 0;
  FU_TRY(reduce_partials<2>(partials, dscratch, nTiles, C, s, &G));
  FU_TRY(sync_sum_over_ranks(sync, dscratch, (int64_t)G * C * 2, true, s));     // exact DP: global batch statistics
  hipLaunchKernelGGL(k_bn_finalize, dim3(ceil_div(C, 8)), dim3(256), 0, s, dscratch, G, C, (double)count * world, o);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm + ReLU backward.  g = dL/d relu(bn(y)) in place -> dL/dy.  The formulas, the per-thread coefficient record
// (BnbCoef) and the block epilogue (block_rows_to_partials) are in fu_elem.h; the kernels differ in where g comes from.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void k_bn_bwd_reduce(const T* __restrict__ g, const T* __restrict__ y, int C, int64_t npix,
                                const float* __restrict__ a, const float* __restrict__ b,
                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                float* __restrict__ partials) {
  extern __shared__ float sm[];  // [rows][C][2]
  const int CV = C >> 2;
  const int rows = BNB_THREADS / CV;
  const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
  float s[2][4] = {};
  if (row < rows) {
    BnbCoef<4, false> K;
    K.load(a, b, mean, invstd, nullptr, cv * 4);
    for (int64_t p = (int64_t)blockIdx.x * rows + row; p < npix; p += (int64_t)gridDim.x * rows) {
      float gv[4], yv[4];
      ElemIO<T>::load4(g + p * C + cv * 4, gv);
      ElemIO<T>::load4(y + p * C + cv * 4, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gm = K.masked(j, gv[j], yv[j]);
        s[0][j] += gm;
        s[1][j] = fmaf(gm, K.xhat(j, yv[j]), s[1][j]);
      }
    }
  }
  block_rows_to_partials<2, 4>(sm, row, rows, C, cv * 4, s, partials);
}

template <typename T>
__global__ void k_bn_bwd_apply(T* __restrict__ g, const T* __restrict__ y, int C, int64_t npix,
                               const float* __restrict__ a, const float* __restrict__ b,
                               const float* __restrict__ mean, const float* __restrict__ invstd,
                               const float* __restrict__ coef, float* __restrict__ db_partials) {
  extern __shared__ float sm[];  // [rows][C]
  const int CV = C >> 2;
  const int rows = BNB_THREADS / CV;
  const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
  float sd[1][4] = {};
  if (row < rows) {
    BnbCoef<4, true> K;
    K.load(a, b, mean, invstd, coef, cv * 4);
    for (int64_t p = (int64_t)blockIdx.x * rows + row; p < npix; p += (int64_t)gridDim.x * rows) {
      float gv[4], yv[4], o[4];
      ElemIO<T>::load4(g + p * C + cv * 4, gv);
      ElemIO<T>::load4(y + p * C + cv * 4, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = K.dy(j, K.masked(j, gv[j], yv[j]), yv[j]);
        sd[0][j] += o[j];
      }
      ElemIO<T>::store4(g + p * C + cv * 4, o);
    }
  }
  block_rows_to_partials<1, 4>(sm, row, rows, C, cv * 4, sd, db_partials);
}

// The same apply pass for the BatchNorm in front of the 1x1 head, with g = dl . w recomputed per element (HeadGrad,
// fu_common.h) instead of read: g stays in fp32 (the stored copy was rounded to the element type), the sums in `coef`
// were taken by k_head_bwd from the same fp32 values.  16-byte vectors, one pixel's channels on C / V lanes.
template <typename T, int NC>
__global__ __launch_bounds__(BNB_THREADS) void k_bn_bwd_apply_head(const float* __restrict__ dl, const float* __restrict__ w,
                                                                    int ncls_rt, T* __restrict__ g, const T* __restrict__ y,
                                                                    int C, int64_t npix, const float* __restrict__ a,
                                                                    const float* __restrict__ b,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ invstd,
                                                                    const float* __restrict__ coef,
                                                                    float* __restrict__ db_partials) {
  constexpr int V = VecIO<T>::V;
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  extern __shared__ float sm[];  // [rows][C]
  const int CV = C / V;
  const int rows = BNB_THREADS / CV;
  const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
  float sd[1][V] = {};
  if (row < rows) {
    BnbCoef<V, true> K;
    K.load(a, b, mean, invstd, coef, cv * V);
    float wv[KMAX][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) wv[k][j] = k < ncls ? w[k * C + cv * V + j] : 0.f;
    }
    constexpr int U = 2;                                         // pixels in flight per thread
    const int64_t step = (int64_t)gridDim.x * rows;
    for (int64_t p0 = (int64_t)blockIdx.x * rows + row; p0 < npix; p0 += U * step) {
      float yv[U][V], d[U][KMAX];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + u * step;
        const bool ok = p < npix;
        VecIO<T>::load(y + (ok ? p : p0) * C + cv * V, yv[u]);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) d[u][k] = (ok && k < ncls) ? dl[p * ncls + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + u * step;
        if (p < npix) {
          float o[V];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            float gv = 0.f;                                      // same expression and order as k_head_bwd
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
              if (k < ncls) gv += d[u][k] * wv[k][j];
            o[j] = K.dy(j, K.masked(j, gv, yv[u][j]), yv[u][j]);
            sd[0][j] += o[j];
          }
          VecIO<T>::store(g + p * C + cv * V, o);
        }
      }
    }
  }
  block_rows_to_partials<1, V>(sm, row, rows, C, cv * V, sd, db_partials);
}

// ------------------------------------------------------------------------------------------------
// BatchNorm + ReLU backward with the max-pool backward folded in (round 2).  For the four encoder outputs that feed a pool,
// dL/d relu(bn(y)) = g (the skip gradient written by the decoder's dgrad) + the pooled gradient routed to the first argmax
// of every 2x2 window.  k_maxpool2_bwd used to add that into g in a read-modify-write pass of its own (a y-sized read, a
// g-sized read and write); here one thread owns a whole 2x2 window x 4 channels, recomputes the window's activations (it
// needs them for the ReLU mask anyway), routes the pooled gradient in registers and does the BN-backward reduction /
// apply on the four pixels.  Same tie rule (first maximum in row-major order, as ATen), same fixed-order block partials.
// ------------------------------------------------------------------------------------------------
template <typename T, bool APPLY>
__global__ void k_bn_bwd_pool(T* __restrict__ g, const T* __restrict__ y, const T* __restrict__ gpool, int C, int B,
                              int H, int W, const float* __restrict__ a, const float* __restrict__ b,
                              const float* __restrict__ mean, const float* __restrict__ invstd,
                              const float* __restrict__ coef, float* __restrict__ partials, unsigned rcpWw,
                              unsigned rcpHw) {
  extern __shared__ float sm[];  // APPLY: [rows][C] (sum dy);  reduce: [rows][C][2]
  const int CV = C >> 2;
  const int rows = BNB_THREADS / CV;
  const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
  const int Ho = H >> 1, Wo = W >> 1, Hw = (H + 1) >> 1, Ww = (W + 1) >> 1;     // pool outputs; windows incl. odd edges
  const int nwin = B * Hw * Ww;             // pixel and window counts < 2^31 (launch_bn_bwd checks): 32-bit window decode by
                                            // host reciprocals (it was two 64-bit divisions per window); 64-bit element offsets
  float s[APPLY ? 1 : 2][4] = {};            // APPLY: sum dy;  reduce: s1, s2
  if (row < rows) {
    BnbCoef<4, APPLY> K;
    K.load(a, b, mean, invstd, coef, cv * 4);
    for (int wi = blockIdx.x * rows + row; wi < nwin; wi += gridDim.x * rows) {
      const int r = fast_div(wi, Ww, rcpWw);
      const int wx = wi - r * Ww;
      const int bb = fast_div(r, Hw, rcpHw);
      const int wy = r - bb * Hw;
      const bool pooled = wy < Ho && wx < Wo;                     // complete window: has a pool output
      float yv[4][4], gv[4][4], z[4][4], gp[4] = {0, 0, 0, 0};
      bool ok[4];
      int64_t off[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int py = 2 * wy + (q >> 1), px = 2 * wx + (q & 1);
        ok[q] = py < H && px < W;
        off[q] = (int64_t)((bb * H + (ok[q] ? py : 0)) * W + (ok[q] ? px : 0)) * C + cv * 4;
        ElemIO<T>::load4(y + off[q], yv[q]);
        ElemIO<T>::load4(g + off[q], gv[q]);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[q][j] = K.pre(j, yv[q][j]);
      }
      if (pooled) ElemIO<T>::load4(gpool + (int64_t)((bb * Ho + wy) * Wo + wx) * C + cv * 4, gp);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int am = 0;
        float m = fmaxf(z[0][j], 0.f);
#pragma unroll
        for (int q = 1; q < 4; ++q) {
          const float zq = fmaxf(z[q][j], 0.f);
          if (zq > m) { m = zq; am = q; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) gv[q][j] += (am == q) ? gp[j] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gm = (z[q][j] > 0.f && ok[q]) ? gv[q][j] : 0.f;   // K.masked on the z kept for the argmax, off the map: 0
          if constexpr (APPLY) {
            o[j] = K.dy(j, gm, yv[q][j]);
            s[0][j] += ok[q] ? o[j] : 0.f;
          } else {
            s[0][j] += gm;
            s[1][j] = fmaf(gm, K.xhat(j, yv[q][j]), s[1][j]);
          }
        }
        if (APPLY && ok[q]) ElemIO<T>::store4(g + off[q], o);
      }
    }
  }
  block_rows_to_partials<APPLY ? 1 : 2, 4>(sm, row, rows, C, cv * 4, s, partials);
}

static int bn_bwd_blocks(int C, int64_t npix) {
  if (C < 4 || C > 4 * BNB_THREADS) return 1;        // no pixel row fits a block: launch_bn_bwd rejects the width
  const int rows = BNB_THREADS / (C >> 2);
  int64_t nb = ceil_div64(npix, (int64_t)rows * 8);  // ~8 pixels per thread
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  return (int)nb;
}
int64_t bn_bwd_partial_elems(int C, int64_t npix) { return (int64_t)bn_bwd_blocks(C, npix) * C * 2; }

template <typename T, bool APPLY>
static void launch_bn_bwd_pool_t(int nb, size_t sh, hipStream_t s, const BnBwdArgs& A, float* partials) {
  hipLaunchKernelGGL((k_bn_bwd_pool<T, APPLY>), dim3(nb), dim3(BNB_THREADS), sh, s, (T*)A.g, (const T*)A.y, (const T*)A.g_pool,
                     A.C, A.B, A.H, A.W, A.a, A.b, A.mean, A.invstd, A.coef, partials, host_rcp((A.W + 1) >> 1),
                     host_rcp((A.H + 1) >> 1));
}

int launch_bn_bwd(Prec p, const BnBwdArgs& A, hipStream_t s) {
  const int C = A.C, B = A.B, H = A.H, W = A.W, ext_partials = A.ext_partials;
  const int64_t npix = A.npix;
  const void* g_pool = A.g_pool;
  const HeadGrad* head = A.head;
  const int world = sync_world(A.sync);
  FU_REQUIRE(head == nullptr || (ext_partials > 0 && g_pool == nullptr && p != PREC_F32 && C % 8 == 0 && BNB_THREADS % (C / 8) == 0),
             "bn_bwd: a recomputed head gradient needs the producer's sums, a 16-bit element type and C | 2048");
  FU_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, "bn_bwd: channels must be a multiple of 4 and <= 1024 (got %d)", C);
  // ext_partials > 0: `partials` already holds that many [C][2] rows of the two sums (written by the producer of g, see
  // BnbFuse in fu_common.h) -- the reduce pass is skipped, the apply pass keeps its own grid
  FU_REQUIRE(ext_partials == 0 || (g_pool == nullptr && world <= 1), "bn_bwd: external partial sums with a pooled source / exact sync");
  const int nb = bn_bwd_blocks(C, npix);
  const int rows = BNB_THREADS / (C >> 2);
  const size_t sh1 = (size_t)rows * C * 2 * sizeof(float);
  const bool pool = g_pool != nullptr;     // the max-pool backward of this tensor is folded into the two passes
  if (pool) {
    FU_REQUIRE((int64_t)B * H * W == npix && BNB_THREADS % (C >> 2) == 0, "bn_bwd (pooled): bad geometry");
    // both fast_div decodes of k_bn_bwd_pool need n * d < 2^32: windows / Ww and (windows / Ww) / Hw
    FU_REQUIRE(npix < ((int64_t)1 << 31) && (int64_t)B * ((H + 1) / 2) * (int64_t)((W + 1) / 2) * ((W + 1) / 2) < ((int64_t)1 << 32) &&
                   (int64_t)B * ((H + 1) / 2) * (int64_t)((H + 1) / 2) < ((int64_t)1 << 32),
               "bn_bwd (pooled): tensor too large for the 32-bit window decode");
    dispatch_prec(p, [&](auto tag) {
      launch_bn_bwd_pool_t<decltype(tag), false>(nb, sh1, s, A, A.partials);
    });
  } else if (ext_partials > 0) {
    // (nothing to launch)
  } else {
    dispatch_prec(p, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(k_bn_bwd_reduce<T>, dim3(nb), dim3(BNB_THREADS), sh1, s, (const T*)A.g, (const T*)A.y, C, npix, A.a,
                         A.b, A.mean, A.invstd, A.partials);
    });
  }
  FU_LAUNCH_CHECK();
  const BnBwdOut o{A.unscale, A.dgamma, A.dbeta, A.coef};
  const int n_rows = ext_partials > 0 ? ext_partials : nb;     // (exact sync never comes with external sums: n_rows = nb there)
  if (world <= 1 && !A.two_level) {
    hipLaunchKernelGGL((k_bn_stats_fused<1, BnBwdOut>), dim3(C / 4), dim3(256), 0, s, A.partials, n_rows, C, (double)npix, o);
    FU_LAUNCH_CHECK();
  } else {
    int G = 0;
    FU_TRY(reduce_partials<2>(A.partials, A.dscratch, n_rows, C, s, &G));
    FU_TRY(sync_sum_over_ranks(A.sync, A.dscratch, (int64_t)G * C * 2, true, s));     // exact DP: global sums of g and g*xhat
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(ceil_div(C, 8)), dim3(256), 0, s, A.dscratch, G, C,
                       (double)npix * world, 1.0 / world, o);
    FU_LAUNCH_CHECK();
  }
  const size_t sh2 = (size_t)rows * C * sizeof(float);
  if (pool) {
    dispatch_prec(p, [&](auto tag) {
      launch_bn_bwd_pool_t<decltype(tag), true>(nb, sh2, s, A, A.db_partials);
    });
  } else if (head) {
    const size_t shh = (size_t)(BNB_THREADS / (C / 8)) * C * sizeof(float);
#define FU_APPLY_HEAD(NC) \
    hipLaunchKernelGGL((k_bn_bwd_apply_head<T, NC>), dim3(nb), dim3(BNB_THREADS), shh, s, head->dl, head->w, head->ncls, \
                       (T*)A.g, (const T*)A.y, C, npix, A.a, A.b, A.mean, A.invstd, A.coef, A.db_partials)
    dispatch_prec(p, [&](auto tag) {
      using T = decltype(tag);
      if constexpr (sizeof(T) == 2) {   // 16-bit element types only (required above)
        switch (head->ncls) {
          case 2: FU_APPLY_HEAD(2); break;
          case 3: FU_APPLY_HEAD(3); break;
          default: FU_APPLY_HEAD(0); break;
        }
      }
    });
#undef FU_APPLY_HEAD
  } else {
    dispatch_prec(p, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(k_bn_bwd_apply<T>, dim3(nb), dim3(BNB_THREADS), sh2, s, (T*)A.g, (const T*)A.y, C, npix, A.a, A.b,
                         A.mean, A.invstd, A.coef, A.db_partials);
    });
  }
  FU_LAUNCH_CHECK();
  *A.n_db_partials = nb;
  return 0;
}

}  // namespace fu
