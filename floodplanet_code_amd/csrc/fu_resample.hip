// Resolution-changing kernels of the UNet path (gfx950): max-pool, bilinear x2 resize forward and backward, and the
// ConvTranspose2d(k=2, s=2) helpers (depth-to-space / space-to-depth, bias-gradient sums, weight embedding).
// HBM-bound: 16-byte vector accesses along the NHWC channel dimension, fp32 math, fixed-order reductions.
#include "fu_common.h"
#include "fu_elem.h"

namespace fu {

// ------------------------------------------------------------------------------------------------
// MaxPool2d(2) on relu(a*y+b) (or on y as is when a == null)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_maxpool2(const T* __restrict__ src, const float* __restrict__ a,
                                                  const float* __restrict__ b, T* __restrict__ dst, int H, int W, int C,
                                                  int Ho, int Wo, int CV, unsigned rcpCV) {
  constexpr int V = VecIO<T>::V;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= Wo * CV) return;
  const int ox = fast_div(item, CV, rcpCV), cv = item - ox * CV;
  const int oy = blockIdx.y, bb = blockIdx.z;
  float av[V], bv[V];
  const bool bn = a != nullptr;
  if (bn) load_coef<V>(a, b, cv * V, av, bv);
  const T* base = src + ((size_t)(bb * H + oy * 2) * W + ox * 2) * C + cv * V;
  float z00[V], z01[V], z10[V], z11[V], o[V];
  load_act<T, V>(base, av, bv, bn, z00);
  load_act<T, V>(base + C, av, bv, bn, z01);
  load_act<T, V>(base + (size_t)W * C, av, bv, bn, z10);
  load_act<T, V>(base + (size_t)W * C + C, av, bv, bn, z11);
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = fmaxf(fmaxf(z00[j], z01[j]), fmaxf(z10[j], z11[j]));
  VecIO<T>::store(dst + ((size_t)(bb * Ho + oy) * Wo + ox) * C + cv * V, o);
}

int launch_maxpool2(Prec p, const void* src, const float* a, const float* b, void* dst, int B, int H, int W, int C,
                    hipStream_t s) {
  const int Ho = H / 2, Wo = W / 2;
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    dim3 g; int CV; unsigned rcp;
    FU_REQUIRE(row_grid<T>(C, Wo, Ho, B, &g, &CV, &rcp), "maxpool: unsupported shape (C=%d H=%d B=%d)", C, H, B);
    hipLaunchKernelGGL(k_maxpool2<T>, g, dim3(256), 0, s, (const T*)src, a, b, (T*)dst, H, W, C, Ho, Wo, CV, rcp);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// bilinear x2 (align_corners=True) of relu(a*y+b), zero-padded to outH x outW (F.pad of unet.py:57-62)
// ------------------------------------------------------------------------------------------------
// R consecutive output rows per thread: one row per thread was latency-bound (a wave lived ~2.5 us for one 16-byte store
// per lane: 3.0 TB/s on the 256x256 level); the 4R loads of a thread are independent and issued ahead of the arithmetic
template <typename T, int R>
__global__ __launch_bounds__(256) void k_upsample2(const T* __restrict__ src, const float* __restrict__ a,
                                                   const float* __restrict__ b, T* __restrict__ dst, int H, int W, int C,
                                                   int outH, int outW, int py0, int px0, UpTables t, int CV,
                                                   unsigned rcpCV) {
  constexpr int V = VecIO<T>::V;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= outW * CV) return;
  const int ox = fast_div(item, CV, rcpCV), cv = item - ox * CV;
  const int oy0 = blockIdx.y * R, bb = blockIdx.z;
  const int ux = ox - px0;
  const bool in_x = ux >= 0 && ux < 2 * W;
  float av[V], bv[V];
  const bool bn = a != nullptr;
  if (bn) load_coef<V>(a, b, cv * V, av, bv);
  // source index and weight as ATen computes them (area_pixel_compute_scale<float>, align_corners=True): the same
  // float expressions as the host tables of the backward pass (fu_plan.hip build_axis), evaluated here so that no
  // load depends on a table load
  const float sx = t.scale_x * (float)ux;
  const int x0 = in_x ? (int)sx : 0;
  const int x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float wx1 = fminf(fmaxf(sx - (float)x0, 0.f), 1.f), wx0 = 1.f - wx1;
  const T* base = src + (size_t)bb * H * W * C + cv * V;
  float z00[R][V], z01[R][V], z10[R][V], z11[R][V], wy1[R];
  bool in[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int uy = oy0 + r - py0;                               // block-uniform
    in[r] = in_x && uy >= 0 && uy < 2 * H && oy0 + r < outH;
    const float sy = t.scale_y * (float)uy;
    const int y0 = in[r] ? (int)sy : 0;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0);
    wy1[r] = fminf(fmaxf(sy - (float)y0, 0.f), 1.f);
    VecIO<T>::load(base + ((size_t)y0 * W + x0) * C, z00[r]);
    VecIO<T>::load(base + ((size_t)y0 * W + x1) * C, z01[r]);
    VecIO<T>::load(base + ((size_t)y1 * W + x0) * C, z10[r]);
    VecIO<T>::load(base + ((size_t)y1 * W + x1) * C, z11[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (oy0 + r >= outH) break;
    float o[V];
    const float wy0 = 1.f - wy1[r];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float p00 = z00[r][j], p01 = z01[r][j], p10 = z10[r][j], p11 = z11[r][j];
      if (bn) {
        p00 = bn_act(av[j], p00, bv[j]); p01 = bn_act(av[j], p01, bv[j]);
        p10 = bn_act(av[j], p10, bv[j]); p11 = bn_act(av[j], p11, bv[j]);
      }
      o[j] = in[r] ? wy0 * (wx0 * p00 + wx1 * p01) + wy1[r] * (wx0 * p10 + wx1 * p11) : 0.f;
    }
    VecIO<T>::store(dst + ((size_t)(bb * outH + oy0 + r) * outW + ox) * C + cv * V, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_upsample2_bwd(const T* __restrict__ gdst, T* __restrict__ gsrc, int H, int W,
                                                       int C, int outH, int outW, int py0, int px0, UpTables t, int CV,
                                                       unsigned rcpCV) {
  constexpr int V = VecIO<T>::V;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= W * CV) return;
  const int ix = fast_div(item, CV, rcpCV), cv = item - ix * CV;
  const int iy = blockIdx.y, bb = blockIdx.z;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  const T* base = gdst + (size_t)bb * outH * outW * C + cv * V;
  // the column list of this lane once, ahead of the row loop (it was re-read from the table inside it, a dependent load
  // and a data-dependent break per tap); same taps in the same order, so the sums are unchanged
  int xo[UP_BWD_MAX];
  float xw[UP_BWD_MAX];
#pragma unroll
  for (int jx = 0; jx < UP_BWD_MAX; ++jx) { xo[jx] = t.xb_o[ix * UP_BWD_MAX + jx]; xw[jx] = t.xb_w[ix * UP_BWD_MAX + jx]; }
  for (int jy = 0; jy < UP_BWD_MAX; ++jy) {
    const int oy = t.yb_o[iy * UP_BWD_MAX + jy];                // block-uniform
    if (oy < 0) break;
    const float wy = t.yb_w[iy * UP_BWD_MAX + jy];
    const T* rowp = base + (size_t)(oy + py0) * outW * C;
#pragma unroll
    for (int jx = 0; jx < UP_BWD_MAX; ++jx) {
      if (__builtin_amdgcn_ballot_w64(xo[jx] >= 0) == 0) break;  // wave-uniform: lists are filled front to back
      if (xo[jx] >= 0) {
        const float w = wy * xw[jx];
        float gv[V];
        VecIO<T>::load(rowp + (size_t)(xo[jx] + px0) * C, gv);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += w * gv[j];
      }
    }
  }
  VecIO<T>::store(gsrc + ((size_t)(bb * H + iy) * W + ix) * C + cv * V, acc);
}

int launch_upsample2(Prec p, const void* src, const float* a, const float* b, void* dst, int B, int H, int W, int C,
                     int outH, int outW, const UpTables& t, hipStream_t s) {
  FU_REQUIRE(outH >= 2 * H && outW >= 2 * W, "upsample: target smaller than 2x source");
  const int py0 = (outH - 2 * H) / 2, px0 = (outW - 2 * W) / 2;
  // four rows per thread where that still leaves >= 2048 workgroups, else one
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    dim3 g; int CV; unsigned rcp;
    FU_REQUIRE(row_grid<T>(C, outW, outH, B, &g, &CV, &rcp), "upsample: unsupported shape (C=%d H=%d B=%d)", C, outH, B);
    if ((int64_t)g.x * ceil_div(outH, 4) * B >= 2048) {
      g.y = ceil_div(outH, 4);
      hipLaunchKernelGGL((k_upsample2<T, 4>), g, dim3(256), 0, s, (const T*)src, a, b, (T*)dst, H, W, C, outH, outW, py0, px0,
                         t, CV, rcp);
    } else {
      hipLaunchKernelGGL((k_upsample2<T, 1>), g, dim3(256), 0, s, (const T*)src, a, b, (T*)dst, H, W, C, outH, outW, py0, px0,
                         t, CV, rcp);
    }
    FU_LAUNCH_CHECK();
    return 0;
  });
}

int launch_upsample2_bwd(Prec p, const void* g_dst, void* g_src, int B, int H, int W, int C, int outH, int outW,
                         const UpTables& t, hipStream_t s) {
  // a smaller target makes py0 / px0 negative: the gather would read in front of the row / of g_dst
  FU_REQUIRE(outH >= 2 * H && outW >= 2 * W, "upsample_bwd: target smaller than 2x source");
  const int py0 = (outH - 2 * H) / 2, px0 = (outW - 2 * W) / 2;
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    dim3 g; int CV; unsigned rcp;
    FU_REQUIRE(row_grid<T>(C, W, H, B, &g, &CV, &rcp), "upsample_bwd: unsupported shape (C=%d H=%d B=%d)", C, H, B);
    hipLaunchKernelGGL(k_upsample2_bwd<T>, g, dim3(256), 0, s, (const T*)g_dst, (T*)g_src, H, W, C, outH, outW, py0, px0, t,
                       CV, rcp);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// ConvTranspose2d(k=2, s=2) support (bilinear=False variant, unet.py:48-51).  out[2y+ky][2x+kx][co] =
// sum_ci in[y][x][ci] * w[ci][co][ky][kx] + b[co]: four independent 1x1 GEMMs, one per output phase p = 2 ky + kx.  They
// run as ONE 1x1 convolution at the LOW resolution with N = 4 cout output channels ordered (p, co) -- on the MFMA conv
// kernels with the weight embedded as a centre tap, exactly the MACs the operator needs (the first version convolved the
// zero-stuffed input with a 3x3 kernel: 9/4 of the MACs and three extra passes) -- followed by a depth-to-space pass that
// interleaves the phases and applies F.pad (unet.py:57-62).  Backward: space-to-depth of dL/d(up) (which crops the pad),
// then the 1x1 conv's dgrad and its one-tap wgrad.
// ------------------------------------------------------------------------------------------------
// up[b][py0 + 2y + ky][px0 + 2x + kx][co] = y4[b][y][x][(2 ky + kx) cout + co]; zero outside the 2h x 2w window
template <typename T>
__global__ void k_depth_to_space(const T* __restrict__ y4, T* __restrict__ up, int h, int w, int C, int outH, int outW,
                                 int py0, int px0, int64_t total) {
  const int CV = C >> 2;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % CV);
    int64_t r = idx / CV;
    const int ox = (int)(r % outW); r /= outW;
    const int oy = (int)(r % outH);
    const int64_t bb = r / outH;
    float o[4] = {0, 0, 0, 0};
    const int uy = oy - py0, ux = ox - px0;
    if (uy >= 0 && uy < 2 * h && ux >= 0 && ux < 2 * w) {
      const int ph = (uy & 1) * 2 + (ux & 1);
      ElemIO<T>::load4(y4 + (((bb * h + (uy >> 1)) * w + (ux >> 1)) * 4 + ph) * (int64_t)C + cv * 4, o);
    }
    ElemIO<T>::store4(up + idx * 4, o);
  }
}
// g4[b][y][x][(2 ky + kx) cout + co] = g_up[b][py0 + 2y + ky][px0 + 2x + kx][co]  (the pad region is dropped)
template <typename T>
__global__ void k_space_to_depth(const T* __restrict__ gup, T* __restrict__ g4, int h, int w, int C, int outH, int outW,
                                 int py0, int px0, int64_t total) {
  const int CV = C >> 2;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % CV);
    int64_t r = idx / CV;
    const int ph = (int)(r & 3); r >>= 2;
    const int x = (int)(r % w); r /= w;
    const int y = (int)(r % h);
    const int64_t bb = r / h;
    float v[4];
    ElemIO<T>::load4(gup + ((bb * outH + py0 + 2 * y + (ph >> 1)) * outW + px0 + 2 * x + (ph & 1)) * (int64_t)C + cv * 4, v);
    ElemIO<T>::store4(g4 + idx * 4, v);
  }
}

// per-channel sums of g [npix][C] -> partials [block][C] (the bias gradient of the ConvTranspose), rows summed in a fixed order
template <typename T>
__global__ void k_channel_partial_sums(const T* __restrict__ g, int C, int64_t npix, float* __restrict__ partials) {
  extern __shared__ float sm[];  // [rows][C]
  const int CV = C >> 2;
  const int rows = BNB_THREADS / CV;
  const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
  if (row < rows) {
    float sd[4] = {0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * rows + row; p < npix; p += (int64_t)gridDim.x * rows) {
      float gv[4];
      ElemIO<T>::load4(g + p * C + cv * 4, gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) sd[j] += gv[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sm[row * C + cv * 4 + j] = sd[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += BNB_THREADS) {
    float t = 0.f;
    for (int r = 0; r < rows; ++r) t += sm[r * C + c];
    partials[(int64_t)blockIdx.x * C + c] = t;
  }
}

// convT weight [Cin][Cout][2][2] -> the embedded 1x1: OIHW 3x3 [(p, co)][Cin][3][3] with w3[...][centre] = w[ci][co][ky][kx]
// (p = 2 ky + kx), zeros elsewhere; bias4[(p, co)] = b[co]
__global__ void k_convT_to_w3(const float* __restrict__ w, const float* __restrict__ b, int Cin, int Cout,
                              float* __restrict__ w3, float* __restrict__ bias4, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int tap = (int)(idx % 9);
    const int64_t r = idx / 9;
    const int ci = (int)(r % Cin);
    const int n4 = (int)(r / Cin);                 // (p, co)
    const int ph = n4 / Cout, co = n4 - ph * Cout;
    w3[idx] = tap == 4 ? w[(((int64_t)ci * Cout + co) * 2 + (ph >> 1)) * 2 + (ph & 1)] : 0.f;
    if (tap == 4 && ci == 0) bias4[n4] = b[co];
  }
}
__global__ void k_convT_grad_from_w3(const float* __restrict__ dw3, int Cin, int Cout, float* __restrict__ dw,
                                     int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int kx = (int)(idx & 1), ky = (int)((idx >> 1) & 1);
    const int64_t r = idx >> 2;
    const int co = (int)(r % Cout);
    const int ci = (int)(r / Cout);
    dw[idx] = dw3[((int64_t)((ky * 2 + kx) * Cout + co) * Cin + ci) * 9 + 4];
  }
}
// out[c] = unscale * sum_i partials[i][c]  (bias gradient of the transposed conv; fixed order)
__global__ void k_colsum_partials(const float* __restrict__ partials, int n, int C, const float* __restrict__ unscale,
                                  float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += (double)partials[(int64_t)i * C + c];
  if (unscale) s *= (double)*unscale;
  out[c] = (float)s;
}

int launch_depth_to_space(Prec p, const void* y4, void* up, int B, int h, int w, int C, int outH, int outW,
                          hipStream_t s) {
  // a smaller target makes py0 / px0 negative (an access in front of the padded map); the kernels move 4 channels at a time
  FU_REQUIRE(outH >= 2 * h && outW >= 2 * w, "depth_to_space: target smaller than 2x source");
  FU_REQUIRE(C % 4 == 0, "depth_to_space: channels must be a multiple of 4 (C=%d)", C);
  const int py0 = (outH - 2 * h) / 2, px0 = (outW - 2 * w) / 2;
  const int64_t total = (int64_t)B * outH * outW * (C / 4);
  const int g = grid_for(total, 256);
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_depth_to_space<T>, dim3(g), dim3(256), 0, s, (const T*)y4, (T*)up, h, w, C, outH, outW, py0, px0,
                       total);
    FU_LAUNCH_CHECK();
    return 0;
  });
}
int launch_space_to_depth(Prec p, const void* gup, void* g4, int B, int h, int w, int C, int outH, int outW,
                          hipStream_t s) {
  // a smaller target makes py0 / px0 negative (an access in front of the padded map); the kernels move 4 channels at a time
  FU_REQUIRE(outH >= 2 * h && outW >= 2 * w, "space_to_depth: target smaller than 2x source");
  FU_REQUIRE(C % 4 == 0, "space_to_depth: channels must be a multiple of 4 (C=%d)", C);
  const int py0 = (outH - 2 * h) / 2, px0 = (outW - 2 * w) / 2;
  const int64_t total = (int64_t)B * h * w * 4 * (C / 4);
  const int g = grid_for(total, 256);
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_space_to_depth<T>, dim3(g), dim3(256), 0, s, (const T*)gup, (T*)g4, h, w, C, outH, outW, py0, px0,
                       total);
    FU_LAUNCH_CHECK();
    return 0;
  });
}
int launch_colsum_partials(const float* partials, int n, int C, const float* unscale, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_colsum_partials, dim3(ceil_div(C, 64)), dim3(64), 0, s, partials, n, C, unscale, out);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_channel_partial_sums(Prec p, const void* g, int C, int64_t npix, float* partials, int* n_partials,
                                hipStream_t s) {
  FU_REQUIRE(C % 4 == 0 && C <= 1024, "channel_sum: channels must be a multiple of 4 and <= 1024");
  const int rows = BNB_THREADS / (C >> 2);
  int64_t nb = ceil_div64(npix, (int64_t)rows * 8);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  const size_t sh = (size_t)rows * C * sizeof(float);
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_channel_partial_sums<T>, dim3((unsigned)nb), dim3(BNB_THREADS), sh, s, (const T*)g, C, npix,
                       partials);
    FU_LAUNCH_CHECK();
    *n_partials = (int)nb;
    return 0;
  });
}
int launch_convT_to_w3(const float* w, const float* b, int Cin, int Cout, float* w3, float* bias4, hipStream_t s) {
  const int64_t total = (int64_t)4 * Cout * Cin * 9;
  hipLaunchKernelGGL(k_convT_to_w3, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, w, b, Cin, Cout, w3, bias4, total);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_convT_grad_from_w3(const float* dw3, int Cin, int Cout, float* dw, hipStream_t s) {
  const int64_t total = (int64_t)Cin * Cout * 4;
  hipLaunchKernelGGL(k_convT_grad_from_w3, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, dw3, Cin, Cout, dw, total);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
