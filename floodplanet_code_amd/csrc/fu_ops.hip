// Single operators behind the C ABI (fu_op_*): one launcher each on caller-owned buffers, with temporary packs and
// partial buffers of their own -- the hooks of the op-level parity tests -- and fu_test_get_buffer,
// fu_test_loss_buffers, fu_test_get_pack, fu_test_fp16_state and fu_test_set_fp16_backoff, the only entry points here that
// look inside a context.
#include "fu_ctx.h"
#include "fu_elem.h"
#include "fu_optim.h"

#include <vector>

using namespace fu;

extern "C" {

// ---- single operators --------------------------------------------------------------------------------
int fu_elem_size(int precision) { return precision == FU_F32 ? 4 : 2; }   /* FU_BF16 and FU_F16: 2 */

static int prec_of(int precision, Prec* p) {
  FU_REQUIRE(precision == FU_F32 || precision == FU_BF16 || precision == FU_F16, "unknown precision %d", precision);
  *p = precision == FU_F32 ? PREC_F32 : (precision == FU_BF16 ? PREC_BF16 : PREC_F16);
  return 0;
}

int fu_op_nchw_to_nhwc(int precision, const float* src, void* dst, int B, int C, int H, int W, int c_pad,
                       fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  return launch_nchw_to_nhwc(p, src, dst, B, C, H, W, c_pad, (hipStream_t)stream);
}
int fu_op_nhwc_to_nchw(int precision, const void* src, float* dst, int B, int C, int H, int W, int c_pad,
                       fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  return launch_nhwc_to_nchw(p, src, dst, B, C, H, W, c_pad, (hipStream_t)stream);
}

// ---- op-level test hooks of the layout kernels (fu_layout.hip): every argument check precedes the launch, so a rejected call
// answers on a machine without a GPU and launches nothing; none of them synchronises ------------------------------------------
namespace {
int layout_shape(const char* who, int B, int C, int H, int W, int c_pad) {
  FU_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: empty shape (B=%d C=%d H=%d W=%d)", who, B, C, H, W);
  FU_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "%s: too many pixels per image", who);
  FU_REQUIRE(c_pad >= C, "%s: c_pad = %d below the %d channels", who, c_pad, C);
  return 0;
}
}  // namespace

int fu_op_nchw_to_nhwc_window(int precision, const float* src, void* dst, int B, int C, int H, int W, int c_pad,
                              int src_channels, int src_channel_offset, fu_stream stream) {
  const char* who = "fu_op_nchw_to_nhwc_window";
  Prec p; FU_TRY(prec_of(precision, &p));
  FU_REQUIRE(src && dst, "%s: null argument", who);
  FU_TRY(layout_shape(who, B, C, H, W, c_pad));
  const int srcC = src_channels > 0 ? src_channels : C;
  FU_REQUIRE(src_channels >= 0 && src_channel_offset >= 0 && src_channel_offset <= srcC - C,
             "%s: channels [%d, %d) outside the %d source channels", who, src_channel_offset, src_channel_offset + C, srcC);
  return launch_nchw_to_nhwc(p, src, dst, B, C, H, W, c_pad, (hipStream_t)stream, src_channels, src_channel_offset);
}

int fu_op_gather_nchw_to_nhwc(int precision, const float* const* srcs, const int32_t* src_channels, int n_src, void* dst,
                              int B, int C, int H, int W, int c_pad, int ch_off, int n_views, const int32_t* view_codes,
                              fu_stream stream) {
  const char* who = "fu_op_gather_nchw_to_nhwc";
  Prec p; FU_TRY(prec_of(precision, &p));
  FU_REQUIRE(dst, "%s: null argument", who);
  FU_TRY(layout_shape(who, B, C, H, W, c_pad));
  SrcList S;
  FU_TRY(make_src_list(who, srcs, src_channels, n_src, &S));
  FU_REQUIRE(ch_off >= 0 && ch_off <= S.coff[S.n] - C, "%s: channels [%d, %d) outside the %d source channels", who, ch_off,
             ch_off + C, S.coff[S.n]);
  FU_REQUIRE(n_views >= 0, "%s: n_views = %d outside 0..8", who, n_views);
  if (n_views == 0) return launch_gather_nchw_to_nhwc(p, S, dst, B, C, H, W, c_pad, ch_off, (hipStream_t)stream);
  unsigned packed = 0;
  FU_TRY(pack_view_codes(who, view_codes, n_views, false, &packed));
  return launch_gather_views_nchw_to_nhwc(p, S, dst, B, n_views, packed, C, H, W, c_pad, ch_off, (hipStream_t)stream);
}

int fu_op_copy_channels(int precision, const void* src, int srcC, int src_off, const float* bn_a, const float* bn_b,
                        void* dst, int dstC, int dst_off, int C, int64_t npix, fu_stream stream) {
  const char* who = "fu_op_copy_channels";
  Prec p; FU_TRY(prec_of(precision, &p));
  FU_REQUIRE(src && dst, "%s: null argument", who);
  FU_REQUIRE(!bn_a == !bn_b, "%s: bn_a and bn_b go together (both or neither)", who);
  FU_REQUIRE(C > 0 && npix > 0, "%s: empty shape (C=%d npix=%lld)", who, C, (long long)npix);
  FU_REQUIRE(src_off >= 0 && src_off <= srcC - C, "%s: channels [%d, %d) outside the %d source channels", who, src_off,
             src_off + C, srcC);
  FU_REQUIRE(dst_off >= 0 && dst_off <= dstC - C, "%s: channels [%d, %d) outside the %d destination channels", who, dst_off,
             dst_off + C, dstC);
  return launch_copy_channels(p, src, srcC, src_off, bn_a, bn_b, dst, dstC, dst_off, C, npix, (hipStream_t)stream);
}

int fu_op_center_to_w3(const float* w, int64_t n, float* w3, fu_stream stream) {
  FU_REQUIRE(w && w3, "fu_op_center_to_w3: null argument");
  FU_REQUIRE(n >= 1, "fu_op_center_to_w3: n must be >= 1 (got %lld)", (long long)n);
  return launch_center_to_w3(w, n, w3, (hipStream_t)stream);
}

int fu_op_center_from_w3(const float* dw3, int64_t n, float* dw, fu_stream stream) {
  FU_REQUIRE(dw3 && dw, "fu_op_center_from_w3: null argument");
  FU_REQUIRE(n >= 1, "fu_op_center_from_w3: n must be >= 1 (got %lld)", (long long)n);
  return launch_center_from_w3(dw3, n, dw, (hipStream_t)stream);
}

namespace {
struct TmpBuf {
  void* p = nullptr;
  ~TmpBuf() { if (p) (void)hipFree(p); }
  int get(size_t bytes) { FU_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16)); return 0; }
};
__global__ void k_stats_collapse(const float* part, int nTiles, int C, float* sum, float* sq) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0, q = 0;
  for (int t = 0; t < nTiles; ++t) { s += part[((int64_t)t * C + c) * 2]; q += part[((int64_t)t * C + c) * 2 + 1]; }
  sum[c] = (float)s; sq[c] = (float)q;
}
}  // namespace

int fu_op_conv3x3_fwd(int precision, const void* src0, int C0, const float* bn_a0, const float* bn_b0,
                      const void* src1, int C1, const float* w_oihw, const float* bias, void* y, int Cout, int B, int H,
                      int W, float* stats_sum, float* stats_sqsum, fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  hipStream_t s = (hipStream_t)stream;
  const int Cin = C0 + (src1 ? C1 : 0);
  TmpBuf wf, st;
  FU_TRY(wf.get(conv3x3_pack_elems(p, Cin, Cout) * fu_elem_size(precision)));
  FU_TRY(launch_pack_conv3x3(p, w_oihw, Cout, Cin, Cin, wf.p, nullptr, s));
  const bool want_stats = stats_sum && stats_sqsum;
  if (want_stats) FU_TRY(st.get((size_t)conv3x3_num_stat_tiles(p, B, H, W) * Cout * 2 * sizeof(float)));
  ConvIn in{src0, C0, bn_a0, bn_b0, src1, src1 ? C1 : 0};
  in.center_only = test_op_center_only();
  int nt = 0;
  FU_TRY(launch_conv3x3(p, in, wf.p, bias, y, Cout, nullptr, 0, want_stats ? (float*)st.p : nullptr, &nt, B, H, W, s));
  if (want_stats)
    hipLaunchKernelGGL(k_stats_collapse, dim3(ceil_div(Cout, 64)), dim3(64), 0, s, (const float*)st.p, nt, Cout,
                       stats_sum, stats_sqsum);
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

int fu_op_conv3x3_dgrad(int precision, const void* dy, int Cout, const float* w_oihw, void* dx0, int C0, void* dx1,
                        int C1, int B, int H, int W, fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  hipStream_t s = (hipStream_t)stream;
  const int Cin = C0 + (dx1 ? C1 : 0);
  TmpBuf wd;
  FU_TRY(wd.get(conv3x3_pack_elems(p, Cin, Cout) * fu_elem_size(precision)));
  FU_TRY(launch_pack_conv3x3(p, w_oihw, Cout, Cin, Cin, nullptr, wd.p, s));
  ConvIn in{dy, Cout, nullptr, nullptr, nullptr, 0};
  in.center_only = test_op_center_only();
  FU_TRY(launch_conv3x3(p, in, wd.p, nullptr, dx0, C0, dx1, dx1 ? C1 : 0, nullptr, nullptr, B, H, W, s));
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

int fu_op_conv3x3_wgrad(int precision, const void* src0, int C0, const float* bn_a0, const float* bn_b0,
                        const void* src1, int C1, const void* dy, int Cout, float* dw_oihw, int B, int H, int W,
                        fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  hipStream_t s = (hipStream_t)stream;
  const int Cin = C0 + (src1 ? C1 : 0);
  TmpBuf slab;
  FU_TRY(slab.get(conv3x3_wgrad_slab_elems(p, Cin, Cout, B, H, W) * sizeof(float)));
  ConvIn in{src0, C0, bn_a0, bn_b0, src1, src1 ? C1 : 0};
  in.center_only = test_op_center_only();
  // a one-tap launch writes the centre tap's slabs only and the reduce reads all nine: zero slabs make dw's other taps 0 here
  // (in the network they are whatever the workspace held; no caller reads them)
  if (in.center_only)
    FU_HIP_CHECK(hipMemsetAsync(slab.p, 0, conv3x3_wgrad_slab_elems(p, Cin, Cout, B, H, W) * sizeof(float), s));
  FU_TRY(launch_conv3x3_wgrad(p, in, dy, Cout, (float*)slab.p, dw_oihw, Cin, nullptr, 0, nullptr, B, H, W, s));
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

int fu_op_maxpool2(int precision, const void* src, const float* bn_a, const float* bn_b, void* dst, int B, int H,
                   int W, int C, fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  const int V = 16 / fu_elem_size(precision);
  FU_REQUIRE(C > 0 && C % V == 0, "maxpool: unsupported shape (C=%d H=%d B=%d)", C, H, B);
  FU_REQUIRE(src && dst, "fu_op_maxpool2: null argument");
  FU_REQUIRE(!bn_a == !bn_b, "fu_op_maxpool2: bn_a and bn_b go together (both or neither)");
  FU_REQUIRE(B > 0 && H >= 2 && W >= 2, "fu_op_maxpool2: no complete 2x2 window (B=%d H=%d W=%d)", B, H, W);
  return launch_maxpool2(p, src, bn_a, bn_b, dst, B, H, W, C, (hipStream_t)stream);
}

int fu_op_upsample2(int precision, const void* src, const float* bn_a, const float* bn_b, void* dst, int B, int H,
                    int W, int C, int outH, int outW, fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  std::vector<void*> tables;
  UpTables t;
  int st = build_up_tables(&tables, H, W, &t);
  if (st == 0) st = launch_upsample2(p, src, bn_a, bn_b, dst, B, H, W, C, outH, outW, t, (hipStream_t)stream);
  (void)hipStreamSynchronize((hipStream_t)stream);
  for (void* q : tables) (void)hipFree(q);
  return st;
}

// ---- op-level test hooks of the decoder's resampling kernels: every argument check precedes the first HIP call, so a
// rejected call answers on a machine without a GPU ---------------------------------------------------------------------------
namespace {
int resample_args(const char* who, int precision, Prec* p, const void* a, const void* b, int vec, int B, int H, int W, int C,
                  int outH, int outW) {
  FU_TRY(prec_of(precision, p));
  FU_REQUIRE(a && b, "%s: null argument", who);
  FU_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: empty shape (B=%d H=%d W=%d C=%d)", who, B, H, W, C);
  FU_REQUIRE(C % vec == 0, "%s: C=%d is not a multiple of the %d channels of a vector", who, C, vec);
  FU_REQUIRE(outH >= 2 * H && outW >= 2 * W, "%s: target %dx%d smaller than 2x the source %dx%d", who, outH, outW, H, W);
  return 0;
}
}  // namespace

int fu_op_upsample2_bwd(int precision, const void* g_dst, void* g_src, int B, int H, int W, int C, int outH, int outW,
                        fu_stream stream) {
  Prec p;
  FU_TRY(resample_args("fu_op_upsample2_bwd", precision, &p, g_dst, g_src, 16 / fu_elem_size(precision), B, H, W, C, outH,
                       outW));
  std::vector<void*> tables;
  UpTables t;
  int st = build_up_tables(&tables, H, W, &t);
  if (st == 0) st = launch_upsample2_bwd(p, g_dst, g_src, B, H, W, C, outH, outW, t, (hipStream_t)stream);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  for (void* q : tables) (void)hipFree(q);
  if (st == 0 && e != hipSuccess) { set_error("fu_op_upsample2_bwd: %s", hipGetErrorString(e)); return FU_ERR_HIP; }
  return st;
}

int fu_op_depth_to_space(int precision, const void* y4, void* up, int B, int h, int w, int C, int outH, int outW,
                         fu_stream stream) {
  Prec p;
  FU_TRY(resample_args("fu_op_depth_to_space", precision, &p, y4, up, 4, B, h, w, C, outH, outW));
  FU_TRY(launch_depth_to_space(p, y4, up, B, h, w, C, outH, outW, (hipStream_t)stream));
  FU_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return FU_OK;
}

int fu_op_space_to_depth(int precision, const void* gup, void* g4, int B, int h, int w, int C, int outH, int outW,
                         fu_stream stream) {
  Prec p;
  FU_TRY(resample_args("fu_op_space_to_depth", precision, &p, gup, g4, 4, B, h, w, C, outH, outW));
  FU_TRY(launch_space_to_depth(p, gup, g4, B, h, w, C, outH, outW, (hipStream_t)stream));
  FU_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return FU_OK;
}

// ---- op-level test hooks for the code that only runs in the benched dispatch (fused BatchNorm-backward sums) ------------
namespace {
// [nTiles][C][2] partial rows -> per-channel sums, fp64 accumulation in tile order
int collapse_partials(const float* part, int nTiles, int C, float* s1, float* s2, hipStream_t s) {
  hipLaunchKernelGGL(k_stats_collapse, dim3(ceil_div(C, 64)), dim3(64), 0, s, part, nTiles, C, s1, s2);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("collapse launch failed: %s", hipGetErrorString(e)); return FU_ERR_HIP; }
  return 0;
}
}  // namespace

int fu_op_conv3x3_dgrad_bnsums(int precision, const void* dy, int Cout, const float* w_oihw, void* dx, int C0,
                               const void* y, const float* bn_a, const float* bn_b, const float* mean,
                               const float* invstd, float* sum_gm, float* sum_gmx, int B, int H, int W,
                               fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  FU_REQUIRE(p != PREC_F32, "fu_op_conv3x3_dgrad_bnsums: 16-bit precisions only (fp32 keeps the separate reduce pass)");
  FU_REQUIRE(dy && w_oihw && dx && y && bn_a && bn_b && mean && invstd && sum_gm && sum_gmx, "fu_op_conv3x3_dgrad_bnsums: null argument");
  hipStream_t s = (hipStream_t)stream;
  TmpBuf wd, part;
  FU_TRY(wd.get(conv3x3_pack_elems(p, C0, Cout) * fu_elem_size(precision)));
  FU_TRY(launch_pack_conv3x3(p, w_oihw, Cout, C0, C0, nullptr, wd.p, s));
  const int64_t cap = (int64_t)B * ceil_div(H, 16) * ceil_div(W, 16) * C0 * 2;
  FU_TRY(part.get((size_t)cap * sizeof(float)));
  int tiles = 0;
  const BnbFuse f = bnb_fuse(y, bn_a, bn_b, mean, invstd, (float*)part.p, cap, &tiles);
  ConvIn in{dy, Cout, nullptr, nullptr, nullptr, 0};
  in.opt.bnb = &f;
  FU_TRY(launch_conv3x3(p, in, wd.p, nullptr, dx, C0, nullptr, 0, nullptr, nullptr, B, H, W, s));
  if (tiles <= 0) {
    set_error("fu_op_conv3x3_dgrad_bnsums: the kernel that ran does not emit the sums for this shape / dispatch");
    return FU_ERR_UNSUPPORTED;
  }
  FU_TRY(perturb_bnb((float*)part.p, tiles, C0, s));
  FU_TRY(collapse_partials((const float*)part.p, tiles, C0, sum_gm, sum_gmx, s));
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

// ---- op-level test hooks of the 1x1 head: like the resampling hooks, every argument check precedes the first HIP call ------
namespace {
// precision, class count and the width rule of the head kernels (head_geometry, fu_head.hip): C = V * {1, 2, 4, 8, 16} lanes
// per pixel, V = 4 (fp32) or 8 (16-bit) channels per 16-byte vector
int head_args(const char* who, int precision, Prec* p, int C, int ncls) {
  FU_TRY(prec_of(precision, p));
  FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "%s: n_classes must be 1..%d (got %d)", who, HEAD_MAX_CLS, ncls);
  const int V = 16 / fu_elem_size(precision);
  const int lpp = C > 0 && C % V == 0 ? C / V : 0;
  FU_REQUIRE(lpp >= 1 && lpp <= 16 && (lpp & (lpp - 1)) == 0, "%s: C must be %d, %d, %d, %d or %d in this precision (got %d)", who,
             V, 2 * V, 4 * V, 8 * V, 16 * V, C);
  return 0;
}
}  // namespace

int fu_op_head_fwd(int precision, const void* y, const float* bn_a, const float* bn_b, const float* w, const float* bias,
                   int C, int ncls, int B, int H, int W, float* logits_nhwc, float* logits_nchw, fu_stream stream) {
  Prec p;
  FU_TRY(head_args("fu_op_head_fwd", precision, &p, C, ncls));
  FU_REQUIRE(y && w && bias && logits_nhwc, "fu_op_head_fwd: null argument");
  FU_REQUIRE(!bn_a == !bn_b, "fu_op_head_fwd: bn_a and bn_b go together (both or neither)");
  FU_REQUIRE(B > 0 && H > 0 && W > 0, "fu_op_head_fwd: empty shape (B=%d H=%d W=%d)", B, H, W);
  FU_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "fu_op_head_fwd: too many pixels per image");
  FU_TRY(launch_head_fwd(p, y, bn_a, bn_b, w, bias, C, ncls, B, H, W, logits_nhwc, logits_nchw, (hipStream_t)stream));
  FU_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return FU_OK;
}

int fu_op_head_bwd(int precision, const float* dlogits_nhwc, const void* y, const float* bn_a, const float* bn_b,
                   const float* w, int C, int ncls, int64_t npix, void* g, float* dw, float* db, const float* mean,
                   const float* invstd, float* sum_gm, float* sum_gmx, fu_stream stream) {
  Prec p;
  FU_TRY(head_args("fu_op_head_bwd", precision, &p, C, ncls));
  FU_REQUIRE(dlogits_nhwc && y && w && g && dw && db, "fu_op_head_bwd: null argument");
  FU_REQUIRE(!bn_a == !bn_b, "fu_op_head_bwd: bn_a and bn_b go together (both or neither)");
  FU_REQUIRE(npix > 0 && npix < ((int64_t)1 << 31), "fu_op_head_bwd: npix must be 1..2^31-1 (got %lld)", (long long)npix);
  const bool want = mean && invstd && sum_gm && sum_gmx;
  FU_REQUIRE(want || !(mean || invstd || sum_gm || sum_gmx),
             "fu_op_head_bwd: mean, invstd, sum_gm and sum_gmx go together (all or none)");
  FU_REQUIRE(!want || bn_a, "fu_op_head_bwd: the BatchNorm-backward sums need bn_a and bn_b");
  if (want && p == PREC_F32) {
    set_error("fu_op_head_bwd: the head-backward kernel does not emit the sums in this precision");
    return FU_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  TmpBuf part, bpart;
  FU_TRY(part.get((size_t)head_bwd_partial_elems(C, ncls) * sizeof(float)));
  const int64_t cap = (int64_t)2048 * C * 2;
  int tiles = 0;
  BnbFuse f;
  if (want) {
    FU_TRY(bpart.get((size_t)cap * sizeof(float)));
    f = bnb_fuse(y, bn_a, bn_b, mean, invstd, (float*)bpart.p, cap, &tiles);
  }
  FU_TRY(launch_head_bwd(p, dlogits_nhwc, y, bn_a, bn_b, w, C, ncls, npix, g, (float*)part.p, dw, db, nullptr, s,
                         want ? &f : nullptr));
  if (want) {
    if (tiles <= 0) {
      set_error("fu_op_head_bwd: the head-backward kernel did not emit the sums");
      return FU_ERR_UNSUPPORTED;
    }
    FU_TRY(perturb_bnb((float*)bpart.p, tiles, C, s));
    FU_TRY(collapse_partials((const float*)bpart.p, tiles, C, sum_gm, sum_gmx, s));
  }
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

// ---- op-level test hooks of the BatchNorm kernels (fu_bn.hip): every argument check precedes the first allocation or HIP call ----
namespace {
// rows [n][C] (fp32) -> out[c] = the rows added in fp64 in row order, rounded once
__global__ void k_rows_collapse(const float* part, int n, int C, float* out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0;
  for (int t = 0; t < n; ++t) s += part[(int64_t)t * C + c];
  out[c] = (float)s;
}
}  // namespace

int fu_op_bn_stats(const float* partials, int n_part, int C, int64_t count, const float* conv_bias, const float* gamma,
                   const float* beta, float eps, float momentum, float* mean, float* invstd, float* a, float* b,
                   float* rmean, float* rvar, int64_t* nbt, fu_stream stream) {
  FU_REQUIRE(partials && gamma && beta && mean && invstd && a && b, "fu_op_bn_stats: null argument");
  FU_REQUIRE(!rmean == !rvar, "fu_op_bn_stats: rmean and rvar go together (both or neither)");
  FU_REQUIRE(n_part >= 1 && C >= 1 && count >= 1, "fu_op_bn_stats: n_part, C and count must be >= 1 (got %d, %d, %lld)", n_part, C,
             (long long)count);
  hipStream_t s = (hipStream_t)stream;
  TmpBuf scr;
  FU_TRY(scr.get((size_t)reduce_scratch_elems(C) * sizeof(double)));
  const BnFwdOut o{conv_bias, gamma, beta, eps, momentum, mean, invstd, a, b, rmean, rvar, nbt};
  FU_TRY(launch_bn_finalize(o, partials, n_part, C, count, (double*)scr.p, nullptr, s));
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

int fu_op_bn_bwd_ex(int precision, void* g, const void* y, int C, int B, int H, int W, const float* bn_a,
                    const float* bn_b, const float* mean, const float* invstd, const void* g_pool, float* dgamma,
                    float* dbeta, const float* ext_sums, int ext_rows, const float* head_dl, const float* head_w, int ncls,
                    const float* unscale, float* db, float* coef, int two_level, fu_stream stream) {
  Prec p; FU_TRY(prec_of(precision, &p));
  FU_REQUIRE(g && y && bn_a && bn_b && mean && invstd && dgamma && dbeta, "fu_op_bn_bwd: null argument");
  FU_REQUIRE(ext_rows >= 0 && !ext_sums == (ext_rows == 0), "fu_op_bn_bwd: external sums and their row count go together");
  FU_REQUIRE(!head_dl == !head_w, "fu_op_bn_bwd: head_dl and head_w go together (both or neither)");
  FU_REQUIRE(B > 0 && H > 0 && W > 0, "fu_op_bn_bwd: empty shape (B=%d H=%d W=%d)", B, H, W);
  FU_REQUIRE(C >= 4 && C <= 1024 && C % 4 == 0, "fu_op_bn_bwd: channels must be a multiple of 4 in 4..1024 (got %d)", C);
  const int64_t npix = (int64_t)B * H * W;
  if (g_pool) {
    FU_REQUIRE(BNB_THREADS % (C / 4) == 0, "fu_op_bn_bwd (pooled): C / 4 must divide %d (got C=%d)", BNB_THREADS, C);
    FU_REQUIRE(!ext_sums && !head_dl, "fu_op_bn_bwd (pooled): neither external sums nor a recomputed head gradient");
    FU_REQUIRE(npix < ((int64_t)1 << 31), "fu_op_bn_bwd (pooled): too many pixels");
  }
  if (head_dl) {
    FU_REQUIRE(p != PREC_F32, "fu_op_bn_bwd (head): 16-bit precisions only");
    FU_REQUIRE(C % 8 == 0 && BNB_THREADS % (C / 8) == 0, "fu_op_bn_bwd (head): C / 8 must divide %d (got C=%d)", BNB_THREADS, C);
    FU_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "fu_op_bn_bwd (head): n_classes must be 1..%d (got %d)", HEAD_MAX_CLS, ncls);
    FU_REQUIRE(ext_sums, "fu_op_bn_bwd (head): the recomputed head gradient needs the external sums");
  }
  hipStream_t s = (hipStream_t)stream;
  TmpBuf part, coefb, dbp, scr;
  if (!ext_sums) FU_TRY(part.get((size_t)bn_bwd_partial_elems(C, npix) * sizeof(float)));
  if (!coef) FU_TRY(coefb.get((size_t)C * 2 * sizeof(float)));
  FU_TRY(dbp.get((size_t)bn_bwd_partial_elems(C, npix) * sizeof(float)));
  FU_TRY(scr.get((size_t)reduce_scratch_elems(std::max(C, 64)) * sizeof(double)));
  int ndb = 0;
  const HeadGrad hg{head_dl, head_w, ncls};
  BnBwdArgs A;
  A.g = g; A.y = y; A.C = C; A.npix = npix;
  A.a = bn_a; A.b = bn_b; A.mean = mean; A.invstd = invstd;
  A.dgamma = dgamma; A.dbeta = dbeta;
  A.partials = ext_sums ? const_cast<float*>(ext_sums) : (float*)part.p;      // read only when the rows are the caller's
  A.coef = coef ? coef : (float*)coefb.p; A.db_partials = (float*)dbp.p; A.n_db_partials = &ndb;
  A.dscratch = (double*)scr.p;
  A.g_pool = g_pool; A.B = B; A.H = H; A.W = W;
  A.ext_partials = ext_rows;
  A.head = head_dl ? &hg : nullptr;
  A.two_level = two_level != 0;
  A.unscale = unscale;
  FU_TRY(launch_bn_bwd(p, A, s));
  if (db) {
    hipLaunchKernelGGL(k_rows_collapse, dim3(ceil_div(C, 64)), dim3(64), 0, s, (const float*)dbp.p, ndb, C, db);
    FU_LAUNCH_CHECK();
  }
  FU_HIP_CHECK(hipStreamSynchronize(s));
  return FU_OK;
}

int fu_op_bn_bwd(int precision, void* g, const void* y, int C, int B, int H, int W, const float* bn_a,
                 const float* bn_b, const float* mean, const float* invstd, const void* g_pool, float* dgamma,
                 float* dbeta, fu_stream stream) {
  return fu_op_bn_bwd_ex(precision, g, y, C, B, H, W, bn_a, bn_b, mean, invstd, g_pool, dgamma, dbeta, nullptr, 0, nullptr,
                         nullptr, 0, nullptr, nullptr, nullptr, 0, stream);
}

// ---- op-level test hooks of the fp16 loss scale and overflow guard (fu_loss.hip, fu_optim.hip) ---------------------------
int fu_op_loss_grad_eff(const float* dlogits, float* out, int64_t n, const float* up_dev, float* partials, float* scale,
                        const int* guard, fu_stream stream) {
  FU_REQUIRE(dlogits && out && partials, "fu_op_loss_grad_eff: null argument");
  FU_REQUIRE(n >= 1, "fu_op_loss_grad_eff: n must be >= 1 (got %lld)", (long long)n);
  return launch_loss_grad_eff(dlogits, out, n, up_dev, partials, scale, (hipStream_t)stream, guard);
}

int fu_op_fp16_guard(const float* g, int64_t n, int* guard, int book, fu_stream stream) {
  FU_REQUIRE(g && guard, "fu_op_fp16_guard: null argument");
  FU_REQUIRE(n >= 1, "fu_op_fp16_guard: n must be >= 1 (got %lld)", (long long)n);
  FU_TRY(launch_grad_finite_check(g, n, guard, (hipStream_t)stream));
  if (book) FU_TRY(launch_guard_book(guard, (hipStream_t)stream));
  return FU_OK;
}

int fu_test_fp16_state(fu_ctx* c, float scale[2], int32_t guard[4]) {
  FU_REQUIRE(c && scale && guard, "fu_test_fp16_state: null argument");
  scale[0] = scale[1] = 0.f;
  guard[0] = guard[1] = guard[2] = guard[3] = 0;
  if (c->prec != PREC_F16) return FU_OK;
  FU_HIP_CHECK(hipSetDevice(c->cfg.device));
  FU_HIP_CHECK(hipDeviceSynchronize());                  // every stream: the step may run on a non-blocking one
  FU_HIP_CHECK(hipMemcpy(scale, c->loss_scale, 2 * sizeof(float), hipMemcpyDeviceToHost));
  FU_HIP_CHECK(hipMemcpy(guard, c->guard, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return FU_OK;
}

int fu_test_set_fp16_backoff(fu_ctx* c, int exponent, int clean_steps, fu_stream stream) {
  FU_REQUIRE(c, "fu_test_set_fp16_backoff: null context");
  FU_REQUIRE(c->prec == PREC_F16, "fu_test_set_fp16_backoff: the context is not fp16");
  FU_REQUIRE(exponent >= 0 && exponent <= 14, "fu_test_set_fp16_backoff: exponent %d outside 0..14", exponent);
  FU_REQUIRE(clean_steps >= 0 && clean_steps <= 63, "fu_test_set_fp16_backoff: clean_steps %d outside 0..63", clean_steps);
  FU_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(c->guard + 2), exponent, 1, (hipStream_t)stream));
  FU_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(c->guard + 3), clean_steps, 1, (hipStream_t)stream));
  return FU_OK;
}

int fu_test_get_buffer(fu_ctx* c, int block, int which, void** ptr, int64_t* elems) {
  FU_REQUIRE(c && ptr && elems, "fu_test_get_buffer: null argument");
  FU_REQUIRE(block >= 0 && block < c->nb, "fu_test_get_buffer: block %d outside 0..%d", block, c->nb - 1);
  const Block& K = c->blk[block];
  const int B = c->cfg.max_batch;
  auto act = [&](int level, int C) { return (int64_t)B * c->Hs[level] * c->Ws[level] * C; };
  switch (which) {
    case 0: *ptr = K.c[0].y; *elems = act(K.c[0].level, K.c[0].cout); break;
    case 1: *ptr = K.c[0].gy; *elems = act(K.c[0].level, K.c[0].cout); break;
    case 2: *ptr = K.c[1].y; *elems = act(K.c[1].level, K.c[1].cout); break;
    case 3: *ptr = K.c[1].gy; *elems = act(K.c[1].level, K.c[1].cout); break;
    case 4: *ptr = K.g_pooled; *elems = K.kind == BK_DOWN ? act(K.level, K.c[0].cin_real) : 0; break;
    case 5: *ptr = K.g_up; *elems = K.kind == BK_UP ? act(K.level, K.c[0].cin_real - c->ch[K.skip]) : 0; break;
    default: set_error("fu_test_get_buffer: which must be 0..5"); return FU_ERR_INVALID;
  }
  return FU_OK;
}

int fu_test_loss_buffers(fu_ctx* c, float** logits, float** dlogits, int64_t* elems) {
  FU_REQUIRE(c && logits && dlogits && elems, "fu_test_loss_buffers: null argument");
  const fu_config& f = c->cfg;
  *logits = c->logits;
  *dlogits = c->dlogits;
  *elems = (int64_t)f.max_batch * f.height * f.width * f.n_classes;
  return FU_OK;
}

int fu_test_get_pack(fu_ctx* c, int kind, int index, int which, fu_test_pack* out) {
  FU_REQUIRE(c && out, "fu_test_get_pack: null argument");
  fu_test_pack r = {};
  r.p_weight = r.p_bias = r.bn = -1;
  if (kind == 0) {
    FU_REQUIRE(index >= 0 && index < c->nb, "fu_test_get_pack: block %d outside 0..%d", index, c->nb - 1);
    FU_REQUIRE(which == 0 || which == 1, "fu_test_get_pack: conv %d of a double conv (0 or 1)", which);
    const Conv& v = c->blk[index].c[which];
    r.present = 1;
    r.wf = v.wf; r.wd = v.wd;
    r.fold_scale = v.fold_scale; r.fold_bias = v.fold_bias; r.a = v.a; r.b = v.b;
    r.cout = v.cout; r.cin_real = v.cin_real; r.cin_pad = v.cin_pad;
    r.p_weight = v.p_w; r.p_bias = v.p_b; r.bn = v.bn;
  } else if (kind == 1) {
    FU_REQUIRE(index >= 0 && index < 5, "fu_test_get_pack: fusion level %d outside 0..4", index);
    FU_REQUIRE(which == 0, "fu_test_get_pack: which must be 0 for a fusion conv");
    if (c->fusion) {
      const Fuse& F = c->fuse[index];
      r.present = 1;
      r.wf = F.wf; r.wd = F.wd;
      r.cout = F.C; r.cin_real = r.cin_pad = c->nE * F.C;
      r.p_weight = F.p_w; r.p_bias = F.p_b;
    }
  } else if (kind == 2) {
    FU_REQUIRE(index >= 5 * c->nE && index < c->nb, "fu_test_get_pack: block %d is not an up block (%d..%d)", index,
               5 * c->nE, c->nb - 1);
    FU_REQUIRE(which == 0, "fu_test_get_pack: which must be 0 for a transposed conv");
    if (!c->cfg.bilinear) {
      const Block& K = c->blk[index];
      r.present = 1;
      r.wf = K.ct_wf; r.wd = K.ct_wd; r.bias4 = K.ct_b4;
      r.cout = 4 * K.ct_cout; r.cin_real = r.cin_pad = K.ct_cin;
      r.p_weight = K.ct_w; r.p_bias = K.ct_b;
    }
  } else {
    set_error("fu_test_get_pack: kind must be 0 (double conv), 1 (fusion conv) or 2 (transposed conv)");
    return FU_ERR_INVALID;
  }
  *out = r;
  return FU_OK;
}

}  // extern "C"
