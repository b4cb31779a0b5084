// The 1x1 head (OutConv) of the UNet path (gfx950), forward and backward; the backward can also emit the BatchNorm-backward
// sums of the gradient it writes (BnbFuse, fu_common.h).
#include "fu_common.h"
#include "fu_elem.h"

namespace fu {

// ------------------------------------------------------------------------------------------------
// head: logits[p][k] = bias[k] + sum_c relu(a*y+b)[p][c] * w[k][c]      (OutConv, unet.py:74-77)
// LPP = C/4 lanes cooperate on one pixel (16 for C = 64); partial dot products meet through wave shuffles.
// ------------------------------------------------------------------------------------------------
// sum over the LPP (power of two <= 16) consecutive lanes of a group; the result is valid in the LAST lane of the
// group.  DPP only: quad_perm for xor 1 / 2, row_shr for the quad-to-quad steps (a __shfl_xor is a ds_bpermute).
__device__ __forceinline__ float dpp_add(float v, const int ctrl_sel) {
  int r;
  const int x = __float_as_int(v);
  switch (ctrl_sel) {
    case 0: r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); break;    // quad_perm [1,0,3,2]
    case 1: r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); break;    // quad_perm [2,3,0,1]
    case 2: r = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true); break;   // row_shr:4
    default: r = __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true); break;  // row_shr:8
  }
  return v + __int_as_float(r);
}
__device__ __forceinline__ float group_sum_last(float v, int LPP) {
  // largest distance first: the same association as the xor-shuffle tree this replaces (bit-identical fp32 logits)
  if (LPP >= 16) v = dpp_add(v, 3);
  if (LPP >= 8) v = dpp_add(v, 2);
  if (LPP >= 4) v = dpp_add(v, 1);
  if (LPP >= 2) v = dpp_add(v, 0);
  return v;
}

// NC: compile-time class count (register arrays sized for it); NC == 0: any count up to HEAD_MAX_CLS.
// Every thread keeps U pixels in flight per iteration (the loop is latency bound otherwise: one 16-byte load per
// thread and ~200 VGPRs for 8 classes gave 89 us for 134 MB).
template <typename T, int NC, int U>
__global__ __launch_bounds__(256) void k_head_fwd(const T* __restrict__ y, const float* __restrict__ a,
                                                  const float* __restrict__ b, const float* __restrict__ w,
                                                  const float* __restrict__ bias, int C, int ncls_rt, int HW, int LPP,
                                                  float* __restrict__ logits_nhwc, float* __restrict__ logits_nchw) {
  constexpr int V = VecIO<T>::V;
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  const int lane_in = threadIdx.x & (LPP - 1);
  const int ppb = 256 / LPP;                 // pixels per block and unroll slot
  const int grp = threadIdx.x / LPP;
  const int bb = blockIdx.y;
  float av[V], bv[V];
  const bool bn = a != nullptr;
  if (bn) load_coef<V>(a, b, lane_in * V, av, bv);
  float wv[KMAX][V];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) wv[k][j] = (k < ncls) ? w[k * C + lane_in * V + j] : 0.f;
  }
  const T* yb = y + (size_t)bb * HW * C + lane_in * V;
  for (int p0 = blockIdx.x * ppb * U; p0 < HW; p0 += gridDim.x * ppb * U) {
    float z[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * ppb + grp;
#pragma unroll
      for (int j = 0; j < V; ++j) z[u][j] = 0.f;
      if (p < HW) load_act<T, V>(yb + (size_t)p * C, av, bv, bn, z[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * ppb + grp;
      float acc[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        float d = 0.f;
        if (k < ncls) {   // uniform
          d = z[u][0] * wv[k][0] + z[u][1] * wv[k][1];   // same expression (and contraction) as the 4-wide original
#pragma unroll
          for (int j = 2; j < V; ++j) d = d + z[u][j] * wv[k][j];
          d = group_sum_last(d, LPP);
        }
        acc[k] = d;
      }
      if (p < HW && lane_in == LPP - 1) {
        const size_t pg = (size_t)bb * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          if (k < ncls) {
            const float v = acc[k] + bias[k];
            logits_nhwc[pg * ncls + k] = v;
            if (logits_nchw) logits_nchw[((size_t)bb * ncls + k) * HW + p] = v;
          }
        }
      }
    }
  }
}

template <typename T>
static bool head_geometry(int C, int* LPP) {
  constexpr int V = 16 / (int)sizeof(T);
  if (C % V != 0) return false;
  *LPP = C / V;
  return *LPP >= 1 && *LPP <= 16 && (*LPP & (*LPP - 1)) == 0;
}

int launch_head_fwd(Prec p, const void* y, const float* a, const float* b, const float* w, const float* bias, int C,
                    int ncls, int B, int H, int W, float* logits_nhwc, float* logits_nchw, hipStream_t s) {
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "head: n_classes must be 1..%d", HEAD_MAX_CLS);
  FU_REQUIRE(B <= 65535, "head: batch too large (%d)", B);
  const int HW = H * W;
  const char* name = p == PREC_F32 ? "fp32" : p == PREC_BF16 ? "bf16" : "fp16";   // for the message below
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    constexpr int V = VecIO<T>::V, U = 4;
    int LPP;
    FU_REQUIRE(head_geometry<T>(C, &LPP), "head: base channels must be %d, %d, %d, %d or %d in %s (got %d)", V, 2 * V, 4 * V,
               8 * V, 16 * V, name, C);
    const int g = ceil_div(ceil_div(HW, (256 / LPP) * U), 2);
#define FU_HEAD_FWD(NC)                                                                                                  \
  hipLaunchKernelGGL((k_head_fwd<T, NC, U>), dim3(g, B), dim3(256), 0, s, (const T*)y, a, b, w, bias, C, ncls, HW, LPP, \
                     logits_nhwc, logits_nchw)
    switch (ncls) {
      case 1: FU_HEAD_FWD(1); break;
      case 2: FU_HEAD_FWD(2); break;
      case 3: FU_HEAD_FWD(3); break;
      case 4: FU_HEAD_FWD(4); break;
      default: FU_HEAD_FWD(0); break;
    }
#undef FU_HEAD_FWD
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// head backward: G[p][c] = sum_k dl[p][k] w[k][c];  dW[k][c] = sum_p dl[p][k] z[p][c];  db[k] = sum_p dl[p][k]
// ------------------------------------------------------------------------------------------------
static constexpr int HB_BLOCKS = 2048;

// BNB: also emit the BatchNorm-backward sums of g (sum g*m, sum g*m*xhat per channel, BnbFuse in fu_common.h) -- y and the
// mask are in registers here anyway; bnpart[block][C][2], one row per block.
template <typename T, int NC, int U, bool BNB, bool STORE = true>
__global__ __launch_bounds__(256) void k_head_bwd(const float* __restrict__ dl, const T* __restrict__ y,
                                                  const float* __restrict__ a, const float* __restrict__ b,
                                                  const float* __restrict__ w, int C, int ncls_rt, int npix, int LPP,
                                                  T* __restrict__ g, float* __restrict__ partials,
                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                  float* __restrict__ bnpart, int kpass) {
  constexpr int V = VecIO<T>::V;
  constexpr int KMAX = NC ? NC : HEAD_MAX_CLS;
  const int ncls = NC ? NC : ncls_rt;
  extern __shared__ float sm[];  // [groups][kpass*C + kpass]
  const int lane_in = threadIdx.x & (LPP - 1);
  const int grp = threadIdx.x / LPP;
  const int ppb = 256 / LPP;
  const int stride = ncls * C + ncls;
  float av[V], bv[V];
  const bool bn = a != nullptr;
  if (bn) load_coef<V>(a, b, lane_in * V, av, bv);
  float wv[KMAX][V], dw[KMAX][V], db[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) { wv[k][j] = (k < ncls) ? w[k * C + lane_in * V + j] : 0.f; dw[k][j] = 0.f; }
    db[k] = 0.f;
  }
  float iv[V], mi[V], s1[V], s2[V];                   // BNB: invstd, -mean * invstd, the two sums
#pragma unroll
  for (int j = 0; j < V; ++j) {
    iv[j] = BNB ? invstd[lane_in * V + j] : 0.f;
    mi[j] = BNB ? -mean[lane_in * V + j] * iv[j] : 0.f;
    s1[j] = 0.f; s2[j] = 0.f;
  }
  // U pixels per thread in flight per iteration; dW / db are summed per thread in visiting order, then per block in
  // LDS and over the blocks in k_head_bwd_finalize (fixed order, deterministic)
  for (int p0 = blockIdx.x * ppb * U; p0 < npix; p0 += gridDim.x * ppb * U) {
    float z[U][V], xh[BNB ? U : 1][V], d[U][KMAX];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * ppb + grp;
      const bool ok = p < npix;
#pragma unroll
      for (int j = 0; j < V; ++j) z[u][j] = 0.f;
      if constexpr (BNB) {
        // (z = 0 marks the masked elements: the mask of the BatchNorm backward is a*y + b > 0, and z = max(a*y + b, 0))
#pragma unroll
        for (int j = 0; j < V; ++j) xh[u][j] = 0.f;
        if (ok) {
          float yv[V];
          VecIO<T>::load(y + (size_t)p * C + lane_in * V, yv);
#pragma unroll
          for (int j = 0; j < V; ++j) { z[u][j] = bn_act(av[j], yv[j], bv[j]); xh[u][j] = fmaf(yv[j], iv[j], mi[j]); }
        }
      } else if (ok) load_act<T, V>(y + (size_t)p * C + lane_in * V, av, bv, bn, z[u]);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) d[u][k] = (ok && k < ncls) ? dl[(size_t)p * ncls + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * ppb + grp;
      if (p < npix) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          if (k < ncls) {
#pragma unroll
            for (int j = 0; j < V; ++j) { o[j] += d[u][k] * wv[k][j]; dw[k][j] += d[u][k] * z[u][j]; }
            db[k] += d[u][k];
          }
        }
        if constexpr (STORE) VecIO<T>::store(g + (size_t)p * C + lane_in * V, o);
        if constexpr (BNB) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float gm = z[u][j] > 0.f ? o[j] : 0.f;
            s1[j] += gm;
            s2[j] = fmaf(gm, xh[u][j], s2[j]);
          }
        }
      }
    }
  }
  // The block's rows meet in LDS, [groups][ncls*C + ncls], wherever that fits the 64 KiB the launch may ask for: every
  // specialised count, and the generic one except 8 classes in the 16-bit types, which take the classes kpass at a time in two
  // passes.  An element's own sum -- the groups in order -- is the same either way.
  if (NC != 0 || kpass >= ncls) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < ncls) {
#pragma unroll
        for (int j = 0; j < V; ++j) sm[grp * stride + k * C + lane_in * V + j] = dw[k][j];
        if (lane_in == 0) sm[grp * stride + ncls * C + k] = db[k];
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < stride; e += blockDim.x) {
      float t = 0.f;
      for (int gq = 0; gq < ppb; ++gq) t += sm[gq * stride + e];
      partials[(size_t)blockIdx.x * stride + e] = t;
    }
  } else {
    for (int k0 = 0; k0 < ncls; k0 += kpass) {
      const int nk = min(kpass, ncls - k0);
      const int pstride = nk * C + nk;   // sm: [groups][nk*C + nk], classes k0 .. k0 + nk - 1
      if (k0 > 0) __syncthreads();
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k >= k0 && k < k0 + nk) {
#pragma unroll
          for (int j = 0; j < V; ++j) sm[grp * pstride + (k - k0) * C + lane_in * V + j] = dw[k][j];
          if (lane_in == 0) sm[grp * pstride + nk * C + (k - k0)] = db[k];
        }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < pstride; e += blockDim.x) {
        float t = 0.f;
        for (int gq = 0; gq < ppb; ++gq) t += sm[gq * pstride + e];
        const int dst = e < nk * C ? k0 * C + e : ncls * C + k0 + (e - nk * C);
        partials[(size_t)blockIdx.x * stride + dst] = t;
      }
    }
  }
  if constexpr (BNB) {
    __syncthreads();                                   // sm: now [groups][C][2]
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sm[(grp * C + lane_in * V + j) * 2 + 0] = s1[j];
      sm[(grp * C + lane_in * V + j) * 2 + 1] = s2[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += blockDim.x) {
      float t = 0.f;
      for (int gq = 0; gq < ppb; ++gq) t += sm[gq * 2 * C + e];
      bnpart[(size_t)blockIdx.x * 2 * C + e] = t;
    }
  }
}

__global__ __launch_bounds__(256) void k_head_bwd_finalize(const float* __restrict__ partials, int nblk, int C,
                                                           int ncls, const float* __restrict__ unscale,
                                                           float* __restrict__ dw, float* __restrict__ db) {
  // 8 elements per block, 32 lanes per element; each lane sums every 32nd block partial, fixed xor tree at the end
  const int stride = ncls * C + ncls;
  const int g = threadIdx.x & 31;
  const int e = blockIdx.x * 8 + (threadIdx.x >> 5);
  double s = 0.0;
  if (e < stride) {
#pragma unroll 4
    for (int i = g; i < nblk; i += 32) s += (double)partials[(int64_t)i * stride + e];
  }
  s = half_wave_sum(s);
  if (e >= stride || g != 0) return;
  if (unscale) s *= (double)*unscale;       // fp16 mode: dlogits carried the loss scale
  if (e < ncls * C) dw[e] = (float)s;
  else db[e - ncls * C] = (float)s;
}

int64_t head_bwd_partial_elems(int C, int ncls) { return (int64_t)HB_BLOCKS * (ncls * C + ncls); }

int launch_head_bwd(Prec p, const float* dlogits_nhwc, const void* y, const float* a, const float* b, const float* w,
                    int C, int ncls, int64_t npix, void* g, float* partials, float* dw, float* db,
                    const float* unscale, hipStream_t s, const BnbFuse* fuse) {
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "head_bwd: n_classes must be 1..%d", HEAD_MAX_CLS);
  FU_REQUIRE(npix < ((int64_t)1 << 31), "head_bwd: too many pixels");
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    int LPP;
    FU_REQUIRE(head_geometry<T>(C, &LPP), "head_bwd: unsupported channel count %d", C);
    constexpr int U = 4;
    const int ppb = 256 / LPP;
    int nblk = (int)ceil_div64(npix, (int64_t)ppb * U);
    if (nblk > HB_BLOCKS) nblk = HB_BLOCKS;
    const int stride = ncls * C + ncls;
    // the BatchNorm-backward sums of g, if asked for (16-bit modes with BatchNorm coefficients: the bench path)
    const bool bnb = fuse && fuse->y == y && fuse->tiles_out && a != nullptr && p != PREC_F32 &&
                     (int64_t)nblk * C * 2 <= fuse->max_elems;
    // classes per LDS pass of the block reduction: all of them where the rows fit in 64 KiB, half otherwise (16-bit, 8 classes:
    // 65536 * (1 + 1/C) bytes in one pass at every width)
    const int kpass = (size_t)ppb * stride * sizeof(float) <= 64 * 1024 ? ncls : ceil_div(ncls, 2);
    size_t sh = (size_t)ppb * (kpass * C + kpass) * sizeof(float);
    FU_REQUIRE(kpass == ncls || ncls > 4, "head_bwd: the specialised class counts reduce in one LDS pass");
    if (bnb && (size_t)ppb * C * 2 * sizeof(float) > sh) sh = (size_t)ppb * C * 2 * sizeof(float);
    FU_REQUIRE(sh <= 64 * 1024, "head_bwd: LDS request too large (%zu)", sh);
    const float* bmean = bnb ? fuse->mean : nullptr;
    const float* binv = bnb ? fuse->invstd : nullptr;
    float* bpart = bnb ? fuse->part : nullptr;
#define FU_HEAD_BWD(NC)                                                                                                      \
  do {                                                                                                                       \
    if (bnb && fuse->skip_g)                                                                                                 \
      hipLaunchKernelGGL((k_head_bwd<T, NC, U, true, false>), dim3(nblk), dim3(256), sh, s, dlogits_nhwc, (const T*)y, a, b, \
                         w, C, ncls, (int)npix, LPP, (T*)g, partials, bmean, binv, bpart, kpass);                            \
    else if (bnb)                                                                                                            \
      hipLaunchKernelGGL((k_head_bwd<T, NC, U, true>), dim3(nblk), dim3(256), sh, s, dlogits_nhwc, (const T*)y, a, b, w, C,  \
                         ncls, (int)npix, LPP, (T*)g, partials, bmean, binv, bpart, kpass);                                  \
    else                                                                                                                     \
      hipLaunchKernelGGL((k_head_bwd<T, NC, U, false>), dim3(nblk), dim3(256), sh, s, dlogits_nhwc, (const T*)y, a, b, w,    \
                         C, ncls, (int)npix, LPP, (T*)g, partials, bmean, binv, bpart, kpass);                               \
  } while (0)
    switch (ncls) {
      case 1: FU_HEAD_BWD(1); break;
      case 2: FU_HEAD_BWD(2); break;
      case 3: FU_HEAD_BWD(3); break;
      case 4: FU_HEAD_BWD(4); break;
      default: FU_HEAD_BWD(0); break;
    }
#undef FU_HEAD_BWD
    FU_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_head_bwd_finalize, dim3(ceil_div(stride, 8)), dim3(256), 0, s, partials, nblk, C, ncls,
                       unscale, dw, db);
    FU_LAUNCH_CHECK();
    if (bnb) *fuse->tiles_out = nblk;
    return 0;
  });
}

}  // namespace fu
