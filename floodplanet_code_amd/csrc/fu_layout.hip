// Layout kernels of the UNet path (gfx950): NCHW fp32 <-> NHWC conversion, the gathers that concatenate several NCHW sources
// (and take test-time-augmentation views) on the way, channel-window copies and the centre-tap embedding of 1x1 weights.
// HBM-bound: 16-byte vector accesses along the NHWC channel dimension.
// Every kernel here runs on its own, bit for bit against a host statement, in tests/test_gpu_layout_ops.py (hooks: fu_ops.hip).
#include "fu_common.h"

namespace fu {

// ------------------------------------------------------------------------------------------------
// NCHW fp32 <-> NHWC T
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, T* __restrict__ dst, int C, int HW, int cpad,
                               int64_t total, int srcC) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % cpad);
    const int64_t bp = idx / cpad;
    const int p = (int)(bp % HW);
    const int64_t b = bp / HW;
    const float v = (c < C) ? src[(b * srcC + c) * HW + p] : 0.f;   // srcC: channels per sample of the source
    ElemIO<T>::store1(dst + idx, v);
  }
}

// 16-bit destinations with c_pad % 8 == 0 (the training path): one thread per (pixel, channel octet) -- eight plane reads
// that are coalesced across the threads of a wave, one 16-byte store; 32-bit indices.  (The flat kernel above decodes a
// 64-bit index twice per ELEMENT and reads with a stride of H*W floats between neighbouring threads.)
template <typename T>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_v8(const float* __restrict__ src, T* __restrict__ dst, int C, int HW,
                                                          int cpad, int srcC) {
  const int p = blockIdx.x * 256 + threadIdx.x;        // pixel inside the sample
  const int o = blockIdx.y, b = blockIdx.z;            // channel octet, sample
  if (p >= HW) return;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = o * 8 + j;
    v[j] = c < C ? src[((size_t)b * srcC + c) * HW + p] : 0.f;
  }
  VecIO<T>::store(dst + ((size_t)b * HW + p) * cpad + o * 8, v);
}

template <typename T>
__global__ void k_nhwc_to_nchw(const T* __restrict__ src, float* __restrict__ dst, int C, int HW, int cpad,
                               int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(idx % HW);
    const int64_t bc = idx / HW;
    const int c = (int)(bc % C);
    const int64_t b = bc / C;
    dst[idx] = ElemIO<T>::load1(src + (b * HW + p) * cpad + c);
  }
}

int launch_nchw_to_nhwc(Prec p, const float* src, void* dst, int B, int C, int H, int W, int c_pad, hipStream_t s,
                        int src_channels, int src_channel_offset) {
  // C channels starting at src_channel_offset of an NCHW tensor with src_channels per sample (0 = C: the whole tensor)
  const int64_t total = (int64_t)B * H * W * c_pad;
  const int g = grid_for(total, 256);
  const int srcC = src_channels > 0 ? src_channels : C;
  src += (int64_t)src_channel_offset * H * W;
  if (p != PREC_F32 && c_pad % 8 == 0 && B <= 65535 && c_pad / 8 <= 65535) {
    const dim3 g8((unsigned)ceil_div(H * W, 256), (unsigned)(c_pad / 8), (unsigned)B);
    return dispatch_prec(p, [&](auto tag) {
      using T = decltype(tag);
      if constexpr (sizeof(T) == 2)   // the octet kernel exists for the 16-bit types only
        hipLaunchKernelGGL(k_nchw_to_nhwc_v8<T>, g8, dim3(256), 0, s, src, (T*)dst, C, H * W, c_pad, srcC);
      FU_LAUNCH_CHECK();
      return 0;
    });
  }
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_nchw_to_nhwc<T>, dim3(g), dim3(256), 0, s, src, (T*)dst, C, H * W, c_pad, total, srcC);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// The same conversion from SEVERAL NCHW sources taken side by side along the channel axis (ef_model.py:28-44: the image and
// the auxiliary maps; stacked sensors): destination channel c is channel ch_off + c of the virtual concatenation.  The
// torch.concat copy of the reference disappears into the layout conversion the first conv needs anyway.  One thread per
// (pixel, vector of V channels); plane reads are coalesced across the threads of a wave, one 16-byte store.
template <typename T>
__global__ __launch_bounds__(256) void k_gather_nchw_to_nhwc(SrcList S, T* __restrict__ dst, int C, int HW, int cpad,
                                                              int ch_off) {
  constexpr int V = VecIO<T>::V;
  const int p = blockIdx.x * 256 + threadIdx.x;        // pixel inside the sample
  const int o = blockIdx.y, b = blockIdx.z;            // channel vector, sample
  if (p >= HW) return;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = o * V + j;
    v[j] = 0.f;
    if (c < C) {
      const int cg = ch_off + c;
      int si = 0;
      for (int k = 1; k < S.n; ++k) si = cg >= S.coff[k] ? k : si;
      v[j] = S.p[si][((size_t)b * S.c[si] + (cg - S.coff[si])) * HW + p];
    }
  }
  VecIO<T>::store(dst + ((size_t)b * HW + p) * cpad + o * V, v);
}

int make_src_list(const char* who, const float* const* srcs, const int32_t* src_channels, int n_src, SrcList* S) {
  FU_REQUIRE(srcs && src_channels && n_src >= 1 && n_src <= 8, "%s: 1..8 sources", who);
  S->n = n_src;
  int off = 0;
  for (int k = 0; k < n_src; ++k) {
    FU_REQUIRE(srcs[k] && src_channels[k] >= 1, "%s: bad source %d", who, k);
    S->p[k] = srcs[k]; S->c[k] = src_channels[k]; S->coff[k] = off; off += src_channels[k];
  }
  S->coff[n_src] = off;
  return 0;
}

int pack_view_codes(const char* who, const int32_t* codes, int n_views, bool distinct, unsigned* packed) {
  FU_REQUIRE(codes && n_views >= 1 && n_views <= 8, "%s: n_views = %d outside 1..8 (or null codes)", who, n_views);
  unsigned pk = 0, seen = 0;
  for (int v = 0; v < n_views; ++v) {
    const int code = codes[v];
    FU_REQUIRE(code >= 0 && code <= 7, "%s: view %d: code %d outside 0..7", who, v, code);
    FU_REQUIRE(!distinct || !((seen >> code) & 1u), "%s: view %d repeats code %d (codes must be distinct)", who, v, code);
    seen |= 1u << code;
    pk |= (unsigned)code << (3 * v);
  }
  *packed = pk;
  return 0;
}

int check_view_geometry(const char* who, int n_views, unsigned codes, int H, int W) {
  for (int v = 0; v < n_views && v < 8; ++v) {
    const int code = (int)((codes >> (3 * v)) & 7u);
    FU_REQUIRE(!(code & 4) || H == W, "%s: view %d: code %d transposes, which needs a square tile (got %dx%d)", who, v, code, H, W);
  }
  return 0;
}

int launch_gather_nchw_to_nhwc(Prec p, const SrcList& S, void* dst, int B, int C, int H, int W, int c_pad, int ch_off,
                               hipStream_t s) {
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    constexpr int V = VecIO<T>::V;
    FU_REQUIRE(c_pad % V == 0 && B <= 65535 && c_pad / V <= 65535, "gather_nchw_to_nhwc: bad geometry (c_pad %d, batch %d)", c_pad, B);
    FU_REQUIRE(ch_off >= 0 && ch_off + C <= S.coff[S.n], "gather_nchw_to_nhwc: channels [%d, %d) outside the %d source channels",
               ch_off, ch_off + C, S.coff[S.n]);
    const dim3 g((unsigned)ceil_div(H * W, 256), (unsigned)(c_pad / V), (unsigned)B);
    hipLaunchKernelGGL(k_gather_nchw_to_nhwc<T>, g, dim3(256), 0, s, S, (T*)dst, C, H * W, c_pad, ch_off);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// Test-time augmentation (fu_forward_views): the gather above, where destination sample v * B + b is view codes[v] of
// crop b -- no transformed copy of the batch is ever written.  A view code is a bit set (1 = flip(-1), 2 = flip(-2),
// 4 = transpose, applied in the order transpose, flip(-1), flip(-2)); `codes` packs 3 bits per view (view_src_pixel in
// fu_common.h).  The transposing codes need H == W; their plane reads go down columns.
template <typename T>
__global__ __launch_bounds__(256) void k_gather_views_nchw_to_nhwc(SrcList S, T* __restrict__ dst, int C, int H, int W,
                                                                    int cpad, int ch_off, int B, unsigned codes) {
  constexpr int V = VecIO<T>::V;
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;        // pixel inside the view
  const int o = blockIdx.y, n = blockIdx.z;            // channel vector, destination sample v * B + b
  if (p >= HW) return;
  const int v = n / B, b = n - v * B;
  const int q = view_src_pixel((codes >> (3 * v)) & 7, p / W, p % W, H, W);
  float val[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = o * V + j;
    val[j] = 0.f;
    if (c < C) {
      const int cg = ch_off + c;
      int si = 0;
      for (int k = 1; k < S.n; ++k) si = cg >= S.coff[k] ? k : si;
      val[j] = S.p[si][((size_t)b * S.c[si] + (cg - S.coff[si])) * HW + q];
    }
  }
  VecIO<T>::store(dst + ((size_t)n * HW + p) * cpad + o * V, val);
}

int launch_gather_views_nchw_to_nhwc(Prec p, const SrcList& S, void* dst, int B, int n_views, unsigned codes, int C, int H,
                                     int W, int c_pad, int ch_off, hipStream_t s) {
  FU_TRY(check_view_geometry("gather_views_nchw_to_nhwc", n_views, codes, H, W));   // x * W + y is a pixel only where H == W
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    constexpr int V = VecIO<T>::V;
    FU_REQUIRE(c_pad % V == 0 && n_views >= 1 && n_views <= 8 && (int64_t)B * n_views <= 65535 && c_pad / V <= 65535,
               "gather_views_nchw_to_nhwc: bad geometry (c_pad %d, batch %d, views %d)", c_pad, B, n_views);
    FU_REQUIRE(ch_off >= 0 && ch_off + C <= S.coff[S.n], "gather_views_nchw_to_nhwc: channels [%d, %d) outside the %d source "
               "channels", ch_off, ch_off + C, S.coff[S.n]);
    const dim3 g((unsigned)ceil_div(H * W, 256), (unsigned)(c_pad / V), (unsigned)(B * n_views));
    hipLaunchKernelGGL(k_gather_views_nchw_to_nhwc<T>, g, dim3(256), 0, s, S, (T*)dst, C, H, W, c_pad, ch_off, B, codes);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

int launch_nhwc_to_nchw(Prec p, const void* src, float* dst, int B, int C, int H, int W, int c_pad, hipStream_t s) {
  const int64_t total = (int64_t)B * C * H * W;
  const int g = grid_for(total, 256);
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_nhwc_to_nchw<T>, dim3(g), dim3(256), 0, s, (const T*)src, dst, C, H * W, c_pad, total);
    FU_LAUNCH_CHECK();
    return 0;
  });
}

// ------------------------------------------------------------------------------------------------
// Late fusion (lf_model.py:78-90): channel-window copies between NHWC tensors, with the producer's BN + ReLU applied on
// the way in (concat of the encoders' features) or plain (split of the concat's gradient), and the 1x1 fusion weight
// embedded as the centre tap of a 3x3 one (the fusion conv runs on the 3x3 kernels for now: 9x the MACs it needs).
// ------------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void k_copy_channels(const T* __restrict__ src, int srcC, int src_off, const float* __restrict__ a,
                                const float* __restrict__ b, T* __restrict__ dst, int dstC, int dst_off, int C,
                                int64_t npix) {
  const int vec = C / V;
  const int64_t total = npix * vec;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % vec);
    const int64_t p = idx / vec;
    float v[V];
    VecIO<T>::load(src + p * srcC + src_off + cv * V, v);
    if (a != nullptr) {
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = bn_act(a[cv * V + k], v[k], b[cv * V + k]);
    }
    VecIO<T>::store(dst + p * dstC + dst_off + cv * V, v);
  }
}
int launch_copy_channels(Prec p, const void* src, int srcC, int src_off, const float* a, const float* b, void* dst,
                         int dstC, int dst_off, int C, int64_t npix, hipStream_t s) {
  return dispatch_prec(p, [&](auto tag) {
    using T = decltype(tag);
    constexpr int V = VecIO<T>::V;
    FU_REQUIRE(C % V == 0 && srcC % V == 0 && dstC % V == 0 && src_off % V == 0 && dst_off % V == 0,
               "copy_channels: channel counts / offsets must be multiples of %d", V);
    const int g = grid_for(npix * (C / V), 256);
    hipLaunchKernelGGL((k_copy_channels<T, V>), dim3(g), dim3(256), 0, s, (const T*)src, srcC, src_off, a, b, (T*)dst, dstC,
                       dst_off, C, npix);
    FU_LAUNCH_CHECK();
    return 0;
  });
}
__global__ void k_center_to_w3(const float* __restrict__ w, float* __restrict__ w3, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * 9; i += (int64_t)gridDim.x * blockDim.x)
    w3[i] = (i % 9 == 4) ? w[i / 9] : 0.f;
}
__global__ void k_center_from_w3(const float* __restrict__ dw3, float* __restrict__ dw, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dw[i] = dw3[i * 9 + 4];
}
int launch_center_to_w3(const float* w, int64_t n, float* w3, hipStream_t s) {
  hipLaunchKernelGGL(k_center_to_w3, dim3(grid_for(n * 9, 256, 4096)), dim3(256), 0, s, w, w3, n);
  FU_LAUNCH_CHECK();
  return 0;
}
int launch_center_from_w3(const float* dw3, int64_t n, float* dw, hipStream_t s) {
  hipLaunchKernelGGL(k_center_from_w3, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, dw3, dw, n);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
