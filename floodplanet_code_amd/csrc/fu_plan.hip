// The static execution plan of a context: the canonical parameter table (reference state_dict order), the workspace
// arena, the bilinear tables, and the packed per-tap weight copies (repack: plain for training, BatchNorm folded in
// for eval) with the kernels that write them.
#include "fu_ctx.h"

namespace fu {

namespace {

// fp32 -> raw 16-bit storage of the context's element type
template <bool HALF> __device__ __forceinline__ unsigned short cvt16(float v) { return HALF ? f2h(v) : f2bf(v); }

template <typename T, bool BF16_LAYOUT, bool HALF = false>
__global__ void k_pack_all(const float* __restrict__ params, PackTable tab, int use_scale) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tab.total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int l = 0;
#pragma unroll 1
    for (int k = 1; k < tab.n; ++k) l = idx >= tab.d[k].start ? k : l;
    const PackDesc& D = tab.d[l];
    const int64_t e = idx - D.start;
    const float* w = params + D.w_off;
    int co, ci, tap;
    if (BF16_LAYOUT) {            // element order [tap][co][ci]
      ci = (int)(e % D.cin_pad);
      const int64_t r = e / D.cin_pad;
      co = (int)(r % D.cout);
      tap = (int)(r / D.cout);
    } else {                      // element order [tap][ci][co]
      co = (int)(e % D.cout);
      const int64_t r = e / D.cout;
      ci = (int)(r % D.cin_pad);
      tap = (int)(r / D.cin_pad);
    }
    float v = ci < D.cin_real ? w[((int64_t)co * D.cin_real + ci) * 9 + tap] : 0.f;
    if (use_scale && ci < D.cin_real) v *= D.scale[co];   // (the channel padding stays +0.0 under a negative scale)
    T* wf = (T*)D.wf;
    T* wd = (T*)D.wd;
    if (BF16_LAYOUT) {
      wf[e] = (T)cvt16<HALF>(v);
      if (wd) wd[((int64_t)(8 - tap) * D.cin_pad + ci) * D.cout + co] = (T)cvt16<HALF>(v);
    } else {
      ElemIO<T>::store1(wf + e, v);
      if (wd) ElemIO<T>::store1(wd + ((int64_t)(8 - tap) * D.cout + co) * D.cin_pad + ci, v);
    }
  }
}

// bf16 layouts, tiled: one workgroup converts a 32 (c_out) x 32 (c_in) x 9 block.  OIHW rows are read as contiguous
// 1152-byte runs, both packed layouts are written as 16-byte vectors along their fastest dimension (wf: c_in,
// wd: c_out); the element-wise kernel above reads with a 36-byte stride and writes 2-byte values 2*cout bytes apart
// (142 us per step for the 17M-parameter UNet, 8x its HBM time).  Needs cout % 8 == 0 and cin_pad % 8 == 0.
template <bool HALF>
__global__ __launch_bounds__(256) void k_pack_tiles_16(const float* __restrict__ params, PackTable tab, int use_scale) {
  constexpr int PITCH = 34;
  __shared__ unsigned short sT[9][32][PITCH];
  int l = 0;
  for (int k = 1; k < tab.n; ++k) l = (int)blockIdx.x >= tab.d[k].tile_start ? k : l;
  const PackDesc& D = tab.d[l];
  const int local = blockIdx.x - D.tile_start;
  const int tco = local / D.tiles_ci, tci = local - tco * D.tiles_ci;
  const int co0 = tco * 32, ci0 = tci * 32;
  const float* w = params + D.w_off;
  // A block's 32 OIHW rows are 32 runs of (up to) 288 contiguous floats.  Where they are 16-byte aligned, a thread fetches its 9
  // float4 pieces back to back (round 4: the scalar loop below issued 36 dependent 4-byte loads per thread, one memory latency
  // each -- 50 us per step at the head of every forward for 138 MB of traffic).
  const int run = min(32, max(D.cin_real - ci0, 0)) * 9;             // valid floats of a row of this tile
  if ((D.w_off & 3) == 0 && (D.cin_real & 3) == 0) {
    float4 v4[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int u = threadIdx.x + k * 256, co_l = u / 72, q = u - co_l * 72;
      const int co = co0 + co_l;
      v4[k] = (co < D.cout && 4 * q < run) ? *reinterpret_cast<const float4*>(w + ((size_t)co * D.cin_real + ci0) * 9 + 4 * q)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);      // (run % 4 == 0: whole pieces)
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int u = threadIdx.x + k * 256, co_l = u / 72, q = u - co_l * 72;
      // (a piece outside the tile's real channels keeps its +0.0: times a negative scale it would be -0.0)
      const float sc = (use_scale && co0 + co_l < D.cout && 4 * q < run) ? D.scale[co0 + co_l] : 1.f;
      const float vv[4] = {v4[k].x, v4[k].y, v4[k].z, v4[k].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * q + j, ci_l = f / 9, tap = f - ci_l * 9;
        sT[tap][co_l][ci_l] = cvt16<HALF>(use_scale ? vv[j] * sc : vv[j]);
      }
    }
  } else {
    for (int e = threadIdx.x; e < 32 * 288; e += 256) {
      const int co_l = e / 288, r = e - co_l * 288;
      const int ci_l = r / 9, tap = r - ci_l * 9;
      const int co = co0 + co_l, ci = ci0 + ci_l;
      float v = (co < D.cout && ci < D.cin_real) ? w[((size_t)co * D.cin_real + ci) * 9 + tap] : 0.f;
      if (use_scale && co < D.cout && ci < D.cin_real) v *= D.scale[co];
      sT[tap][co_l][ci_l] = cvt16<HALF>(v);
    }
  }
  __syncthreads();
  bf16_t* wf = (bf16_t*)D.wf;
  bf16_t* wd = (bf16_t*)D.wd;
  for (int it = threadIdx.x; it < 9 * 32 * 4; it += 256) {
    const int oct = it & 3, row = (it >> 2) & 31, tap = it >> 7;
    {   // wf[tap][co][ci]: row = c_out, 8 consecutive c_in
      const int co = co0 + row, ci = ci0 + oct * 8;
      if (co < D.cout && ci < D.cin_pad) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&sT[tap][row][oct * 8]);
        *reinterpret_cast<uint4*>(wf + ((size_t)tap * D.cout + co) * D.cin_pad + ci) =
            make_uint4(src[0], src[1], src[2], src[3]);
      }
    }
    if (wd) {   // wd[8 - tap][ci][co]: row = c_in, 8 consecutive c_out
      const int ci = ci0 + row, co = co0 + oct * 8;
      if (ci < D.cin_pad && co < D.cout) {
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (unsigned)sT[tap][oct * 8 + 2 * j][row] | ((unsigned)sT[tap][oct * 8 + 2 * j + 1][row] << 16);
        *reinterpret_cast<uint4*>(wd + ((size_t)(8 - tap) * D.cin_pad + ci) * D.cout + co) =
            make_uint4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

// Eval mode (water_seg_model.py:92-96, 138-158: BatchNorm on its running statistics): bn(conv(x)) is affine per output
// channel, so it is folded into the conv once per parameter change -- packed weights times scale = gamma / sqrt(rv + eps),
// bias' = scale * bias + (beta - rm * scale) -- and every consumer's activation prologue becomes relu(1 * y + 0).
__global__ void k_bn_fold_eval(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ rm, const float* __restrict__ rv, const float* __restrict__ bias,
                               float eps, float* __restrict__ scale, float* __restrict__ fbias, float* __restrict__ a,
                               float* __restrict__ b) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  float shift;   // beta - rm * scale: a product and a difference, each rounded (left to -ffp-contract=fast they became one fma,
  {              // up to 32 ulp off in fold_bias where the two terms cancel: tests/test_gpu_weight_pack.py)
#pragma clang fp contract(off)
    const float p = rm[c] * sc;
    shift = beta[c] - p;
  }
  fbias[c] = fmaf(sc, bias[c], shift);
  a[c] = 1.f;
  b[c] = 0.f;
}

}  // namespace

static std::string dc_prefix(int i) {   // i = block role
  if (i == 0) return "inc.double_conv";
  if (i <= 4) return "down" + std::to_string(i) + ".maxpool_conv.1.double_conv";
  return "up" + std::to_string(i - 4) + ".conv.double_conv";
}

static int add_param(fu_ctx* c, const std::string& name, std::initializer_list<int64_t> shape) {
  ParamInfo p;
  p.name = name;
  p.ndim = (int)shape.size();
  p.numel = 1;
  int k = 0;
  for (auto d : shape) { p.shape[k++] = d; p.numel *= d; }
  for (; k < 4; ++k) p.shape[k] = 1;
  p.off = c->total_params;
  c->total_params += p.numel;
  c->params.push_back(p);
  return (int)c->params.size() - 1;
}

static void build_axis(int in, std::vector<int>& i0, std::vector<int>& i1, std::vector<float>& w1, std::vector<int>& bo,
                std::vector<float>& bw, bool* ok) {
  const int out = 2 * in;
  // ATen area_pixel_compute_scale<float>(align_corners=True) and compute_source_index_and_lambda
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  i0.resize(out); i1.resize(out); w1.resize(out);
  bo.assign((size_t)in * UP_BWD_MAX, -1);
  bw.assign((size_t)in * UP_BWD_MAX, 0.f);
  std::vector<int> cnt(in, 0);
  auto push = [&](int i, int o, float w) {
    if (w == 0.f) return;
    for (int j = 0; j < cnt[i]; ++j)
      if (bo[(size_t)i * UP_BWD_MAX + j] == o) { bw[(size_t)i * UP_BWD_MAX + j] += w; return; }
    if (cnt[i] >= UP_BWD_MAX) { *ok = false; return; }
    bo[(size_t)i * UP_BWD_MAX + cnt[i]] = o;
    bw[(size_t)i * UP_BWD_MAX + cnt[i]] = w;
    cnt[i]++;
  };
  for (int o = 0; o < out; ++o) {
    const float src = scale * (float)o;
    const int a = (int)src;
    const int off = a < in - 1 ? 1 : 0;
    float l1 = src - (float)a;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    i0[o] = a; i1[o] = a + off; w1[o] = l1;
    push(a, o, 1.f - l1);
    push(a + off, o, l1);
  }
}

template <typename T>
static int upload(std::vector<void*>* allocs, const std::vector<T>& v, const T** out) {
  void* d = nullptr;
  FU_HIP_CHECK(hipMalloc(&d, v.size() * sizeof(T) + 16));
  FU_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  allocs->push_back(d);
  *out = (const T*)d;
  return 0;
}

int build_up_tables(std::vector<void*>* allocs, int H, int W, UpTables* t) {
  std::vector<int> yi0, yi1, xi0, xi1, ybo, xbo;
  std::vector<float> yw1, xw1, ybw, xbw;
  bool ok = true;
  build_axis(H, yi0, yi1, yw1, ybo, ybw, &ok);
  build_axis(W, xi0, xi1, xw1, xbo, xbw, &ok);
  FU_REQUIRE(ok, "bilinear backward table overflow (H=%d W=%d)", H, W);
  t->scale_y = 2 * H > 1 ? (float)(H - 1) / (float)(2 * H - 1) : 0.f;
  t->scale_x = 2 * W > 1 ? (float)(W - 1) / (float)(2 * W - 1) : 0.f;
  FU_TRY(upload(allocs, yi0, &t->y_i0)); FU_TRY(upload(allocs, yi1, &t->y_i1)); FU_TRY(upload(allocs, yw1, &t->y_w1));
  FU_TRY(upload(allocs, xi0, &t->x_i0)); FU_TRY(upload(allocs, xi1, &t->x_i1)); FU_TRY(upload(allocs, xw1, &t->x_w1));
  FU_TRY(upload(allocs, ybo, &t->yb_o)); FU_TRY(upload(allocs, ybw, &t->yb_w));
  FU_TRY(upload(allocs, xbo, &t->xb_o)); FU_TRY(upload(allocs, xbw, &t->xb_w));
  return 0;
}

int build_plan(fu_ctx* c) {
  const fu_config& f = c->cfg;
  const int base = f.base_channels;
  const int factor = f.bilinear ? 2 : 1;
  c->ch[0] = base; c->ch[1] = base * 2; c->ch[2] = base * 4; c->ch[3] = base * 8; c->ch[4] = base * 16 / factor;
  c->Hs[0] = f.height; c->Ws[0] = f.width;
  for (int l = 1; l < 5; ++l) { c->Hs[l] = c->Hs[l - 1] / 2; c->Ws[l] = c->Ws[l - 1] / 2; }
  FU_REQUIRE(c->Hs[4] >= 1 && c->Ws[4] >= 1, "tile %dx%d is too small for four 2x poolings", f.height, f.width);
  c->fusion = f.n_encoders >= 1;
  c->nE = c->fusion ? f.n_encoders : 1;
  c->nb = 5 * c->nE + 4;
  c->blk.assign(c->nb, Block());
  for (int e = 0, off = 0; e < c->nE; ++e) {
    c->enc_ch[e] = c->fusion ? f.enc_channels[e] : f.n_channels;
    c->enc_coff[e] = off;
    off += c->enc_ch[e];
    c->cin_pad0[e] = round_up(c->enc_ch[e], c->prec == PREC_F32 ? 4 : 8);
  }
  const int outs[4] = {base * 8 / factor, base * 4 / factor, base * 2 / factor, base};

  int low = c->ch[4];
  for (int i = 0; i < c->nb; ++i) {
    Block& K = c->blk[i];
    int cin, cmid, cout;
    const bool is_enc = i < 5 * c->nE;
    K.enc = is_enc ? i / 5 : 0;
    K.role = is_enc ? i % 5 : 5 + (i - 5 * c->nE);
    const int r = K.role;
    if (r == 0) { K.kind = BK_INC; K.level = 0; cin = c->enc_ch[K.enc]; cmid = cout = c->ch[0]; }
    else if (r <= 4) { K.kind = BK_DOWN; K.level = r; cin = c->ch[r - 1]; cmid = cout = c->ch[r]; }
    else {
      const int k = r - 5;
      K.kind = BK_UP; K.skip = 3 - k; K.level = 3 - k;
      if (f.bilinear) { cin = low + c->ch[3 - k]; cmid = cin / 2; cout = outs[k]; }
      else { K.ct_cin = low; K.ct_cout = low / 2; cin = low / 2 + c->ch[3 - k]; cmid = cout = outs[k]; }
      low = cout;
    }
    if (c->fusion && r == 5) {   // between the encoders and the decoder in the flat buffers (backward order stays adjacent)
      for (int l = 0; l < 5; ++l) {
        Fuse& F = c->fuse[l];
        F.C = c->ch[l];
        const std::string cn = "concat_convs." + std::to_string(l);
        F.p_w = add_param(c, cn + ".weight", {F.C, (int64_t)c->nE * F.C, 1, 1});
        F.p_b = add_param(c, cn + ".bias", {F.C});
      }
    }
    const std::string scope = !c->fusion ? "" : (is_enc ? "encoders." + std::to_string(K.enc) + "." : "decoder.");
    K.first_param = (int)c->params.size();
    if (K.kind == BK_UP && !f.bilinear) {
      const std::string up = scope + "up" + std::to_string(r - 4) + ".up";
      K.ct_w = add_param(c, up + ".weight", {K.ct_cin, K.ct_cout, 2, 2});
      K.ct_b = add_param(c, up + ".bias", {K.ct_cout});
    }
    const std::string pre = scope + dc_prefix(r);
    for (int j = 0; j < 2; ++j) {
      Conv& v = K.c[j];
      v.level = K.level;
      v.cin_real = j == 0 ? cin : cmid;
      v.cin_pad = (r == 0 && j == 0) ? c->cin_pad0[K.enc] : v.cin_real;
      v.cout = j == 0 ? cmid : cout;
      const std::string cn = pre + "." + std::to_string(j == 0 ? 0 : 3);
      const std::string bn = pre + "." + std::to_string(j == 0 ? 1 : 4);
      v.p_w = add_param(c, cn + ".weight", {v.cout, v.cin_real, 3, 3});
      v.p_b = add_param(c, cn + ".bias", {v.cout});
      v.p_g = add_param(c, bn + ".weight", {v.cout});
      v.p_beta = add_param(c, bn + ".bias", {v.cout});
      v.bn = (int)c->bns.size();
      c->bns.push_back({bn, v.cout, c->total_bn});
      c->total_bn += v.cout;
    }
    K.num_params = (int)c->params.size() - K.first_param;
  }
  const std::string dscope = c->fusion ? "decoder." : "";
  c->p_outw = add_param(c, dscope + "outc.conv.weight", {f.n_classes, base, 1, 1});
  c->p_outb = add_param(c, dscope + "outc.conv.bias", {f.n_classes});
  return 0;
}

int alloc_workspace(fu_ctx* c) {
  const fu_config& f = c->cfg;
  const int B = f.max_batch;
  Arena& A = c->arena;
  const size_t es = c->esize;
  auto act = [&](int level, int C) { return (size_t)B * c->Hs[level] * c->Ws[level] * C * es; };
  for (int e = 0; e < c->nE; ++e) A.want(&c->xin[e], act(0, c->cin_pad0[e]));
  int64_t max_stats = 0, max_bnb = 0, max_slab = 0, max_dbp = 0;
  int max_c = 0;
  for (int i = 0; i < c->nb; ++i) {
    Block& K = c->blk[i];
    for (int j = 0; j < 2; ++j) {
      Conv& v = K.c[j];
      const int H = c->Hs[v.level], W = c->Ws[v.level];
      const int64_t npix = (int64_t)B * H * W;
      A.want(&v.y, act(v.level, v.cout));
      A.want(&v.gy, act(v.level, v.cout));
      A.want(&v.mean, v.cout * sizeof(float));
      A.want(&v.invstd, v.cout * sizeof(float));
      A.want(&v.a, v.cout * sizeof(float));
      A.want(&v.b, v.cout * sizeof(float));
      A.want(&v.coef, v.cout * 2 * sizeof(float));
      A.want(&v.fold_scale, v.cout * sizeof(float));
      A.want(&v.fold_bias, v.cout * sizeof(float));
      A.want(&v.wf, conv3x3_pack_elems(c->prec, v.cin_pad, v.cout) * es);
      if (!(K.role == 0 && j == 0)) A.want(&v.wd, conv3x3_pack_elems(c->prec, v.cin_pad, v.cout) * es);
      max_stats = std::max<int64_t>(max_stats, (int64_t)conv3x3_num_stat_tiles(c->prec, B, H, W) * v.cout * 2);
      max_bnb = std::max<int64_t>(max_bnb, bn_bwd_partial_elems(v.cout, npix));
      // one row of c_out bias-gradient partials per BN-backward workgroup, per conv (0.5 - 2 MB each, 19.5 MB over the 18
      // convs of the base-64 net at B = 16, 256 x 256, against 4 MB for the two alternating buffers they replace): nothing inside one backward reuses such a buffer (backward_conv)
      A.want(&v.db_part, bn_bwd_partial_elems(v.cout, npix) / 2 * sizeof(float));
      max_slab = std::max<int64_t>(max_slab, conv3x3_wgrad_slab_elems(c->prec, v.cin_pad, v.cout, B, H, W));
      max_c = std::max(max_c, v.cout);
    }
    if (K.kind == BK_DOWN) {
      A.want(&K.pooled, act(K.level, K.c[0].cin_real));
      A.want(&K.g_pooled, act(K.level, K.c[0].cin_real));
    } else if (K.kind == BK_UP) {
      const int clow = K.c[0].cin_real - c->ch[K.skip];
      A.want(&K.up, act(K.level, clow));
      A.want(&K.g_up, act(K.level, clow));
      if (!f.bilinear) {
        const int H = c->Hs[K.level], W = c->Ws[K.level];
        A.want(&K.u, act(K.level, K.ct_cout));            // = B h w (4 ct_cout)
        A.want(&K.g_u, act(K.level, K.ct_cout));
        A.want(&K.ct_w3, (size_t)9 * K.ct_cin * 4 * K.ct_cout * sizeof(float));
        A.want(&K.ct_dw3, (size_t)9 * K.ct_cin * 4 * K.ct_cout * sizeof(float));
        A.want(&K.ct_b4, (size_t)4 * K.ct_cout * sizeof(float));
        A.want(&K.ct_wf, conv3x3_pack_elems(c->prec, K.ct_cin, 4 * K.ct_cout) * es);
        A.want(&K.ct_wd, conv3x3_pack_elems(c->prec, K.ct_cin, 4 * K.ct_cout) * es);
        max_slab = std::max<int64_t>(max_slab, conv3x3_wgrad_slab_elems(c->prec, K.ct_cin, 4 * K.ct_cout, B, H / 2, W / 2));
        max_dbp = std::max<int64_t>(max_dbp, (int64_t)2048 * K.ct_cout);
      }
    }
  }
  for (int l = 0; l < 5 && c->fusion; ++l) {
    Fuse& F = c->fuse[l];
    const int Ccat = c->nE * F.C, H = c->Hs[l], W = c->Ws[l];
    A.want(&F.cat, act(l, Ccat));
    A.want(&F.gcat, act(l, Ccat));
    A.want(&F.y, act(l, F.C));
    A.want(&F.gy, act(l, F.C));
    A.want(&F.w3, (size_t)9 * Ccat * F.C * sizeof(float));
    A.want(&F.dw3, (size_t)9 * Ccat * F.C * sizeof(float));
    A.want(&F.wf, conv3x3_pack_elems(c->prec, Ccat, F.C) * es);
    A.want(&F.wd, conv3x3_pack_elems(c->prec, Ccat, F.C) * es);
    max_slab = std::max<int64_t>(max_slab, conv3x3_wgrad_slab_elems(c->prec, Ccat, F.C, B, H, W));
    max_dbp = std::max<int64_t>(max_dbp, (int64_t)2048 * F.C);
  }
  const int64_t npix0 = (int64_t)B * f.height * f.width;
  A.want(&c->logits, npix0 * f.n_classes * sizeof(float));
  A.want(&c->dlogits, npix0 * f.n_classes * sizeof(float));
  A.want(&c->dlogits_eff, npix0 * f.n_classes * sizeof(float));
  A.want(&c->up_scale, 256);
  A.want(&c->stats, max_stats * sizeof(float));
  A.want(&c->bnb_part, max_bnb * sizeof(float));
  c->bnb_cap = max_bnb;
  A.want(&c->db_part, max_dbp * sizeof(float));   // (the fusion convs and the ConvTranspose path only)
  A.want(&c->dscratch, reduce_scratch_elems(std::max(max_c, 64)) * sizeof(double));
  A.want(&c->slab, max_slab * sizeof(float));
  A.want(&c->ce_part, LOSS_PART_FLOATS * sizeof(float));
  A.want(&c->ce_wsum, 256);
  A.want(&c->region_coef, REGION_COEF_BYTES);
  A.want(&c->hb_part, head_bwd_partial_elems(f.base_channels, f.n_classes) * sizeof(float));
  A.want(&c->loss_dev, 256);
  A.want(&c->loss_scale, 256);
  A.want(&c->guard, 256);
  A.want(&c->conf_tmp, 64 * sizeof(unsigned long long));
  A.want(&c->n_valid, 256);
  FU_TRY(A.commit());
  for (int i = 5 * c->nE; i < c->nb && f.bilinear; ++i) {
    Block& K = c->blk[i];
    const int lowlvl = K.level + 1;
    FU_TRY(build_up_tables(&c->extra_allocs, c->Hs[lowlvl], c->Ws[lowlvl], &K.upt));
  }
  return 0;
}

int repack(fu_ctx* c, hipStream_t s, bool eval) {
  const int use_scale = eval ? 1 : 0;
  if (eval) {
    for (int i = 0; i < c->nb; ++i)
      for (int j = 0; j < 2; ++j) {
        Conv& v = c->blk[i].c[j];
        const int64_t off = c->bns[v.bn].off;
        hipLaunchKernelGGL(k_bn_fold_eval, dim3(fu::ceil_div(v.cout, 64)), dim3(64), 0, s, v.cout, P(c, v.p_g),
                           P(c, v.p_beta), c->RM + off, c->RV + off, P(c, v.p_b), BN_EPS, v.fold_scale, v.fold_bias, v.a,
                           v.b);
      }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("eval fold launch failed: %s", hipGetErrorString(e)); return FU_ERR_HIP; }
  }
  if (c->pack_tabs.empty()) {
    bool tiled_ok = true;
    for (int i = 0; i < c->nb; ++i)
      for (int j = 0; j < 2; ++j) {
        const Conv& v = c->blk[i].c[j];
        if (v.cout % 8 != 0 || v.cin_pad % 8 != 0) tiled_ok = false;
      }
    int64_t start = 0;
    for (int i = 0; i < c->nb; ++i)
      for (int j = 0; j < 2; ++j) {
        Conv& v = c->blk[i].c[j];
        if (c->pack_tabs.empty() || c->pack_tabs.back().n == MAX_PACK) {   // one launch per MAX_PACK layers
          PackTable nt;
          nt.n = 0; nt.total = 0; nt.tiles = 0;
          c->pack_tabs.push_back(nt);
          start = 0;
        }
        PackTable& t = c->pack_tabs.back();
        PackDesc& d = t.d[t.n++];
        d.start = start;
        d.w_off = c->params[v.p_w].off;
        d.cout = v.cout; d.cin_real = v.cin_real; d.cin_pad = v.cin_pad; d.pad_ = 0;
        d.wf = v.wf; d.wd = v.wd;
        d.scale = v.fold_scale;
        start += (int64_t)9 * v.cin_pad * v.cout;
        d.tile_start = t.tiles;
        d.tiles_ci = fu::ceil_div(v.cin_pad, 32);
        t.tiles += fu::ceil_div(v.cout, 32) * d.tiles_ci;
        t.total = start;
      }
    if (!tiled_ok) for (PackTable& t : c->pack_tabs) t.tiles = 0;
  }
  const int grid = 2048;
  for (const PackTable& t : c->pack_tabs) {
    if (c->prec == PREC_F32)
      hipLaunchKernelGGL((k_pack_all<float, false>), dim3(grid), dim3(256), 0, s, c->P, t, use_scale);
    else if (t.tiles > 0 && c->prec == PREC_BF16)
      hipLaunchKernelGGL(k_pack_tiles_16<false>, dim3(t.tiles), dim3(256), 0, s, c->P, t, use_scale);
    else if (t.tiles > 0)
      hipLaunchKernelGGL(k_pack_tiles_16<true>, dim3(t.tiles), dim3(256), 0, s, c->P, t, use_scale);
    else if (c->prec == PREC_BF16)
      hipLaunchKernelGGL((k_pack_all<bf16_t, true, false>), dim3(grid), dim3(256), 0, s, c->P, t, use_scale);
    else
      hipLaunchKernelGGL((k_pack_all<bf16_t, true, true>), dim3(grid), dim3(256), 0, s, c->P, t, use_scale);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("pack launch failed: %s", hipGetErrorString(e)); return FU_ERR_HIP; }
  }
  for (int l = 0; l < 5 && c->fusion; ++l) {
    Fuse& F = c->fuse[l];
    const int Ccat = c->nE * F.C;
    FU_TRY(launch_center_to_w3(P(c, F.p_w), (int64_t)F.C * Ccat, F.w3, s));
    FU_TRY(launch_pack_conv3x3(c->prec, F.w3, F.C, Ccat, Ccat, F.wf, F.wd, s));
  }
  if (!c->cfg.bilinear) {
    for (int i = 5 * c->nE; i < c->nb; ++i) {
      Block& K = c->blk[i];
      FU_TRY(launch_convT_to_w3(P(c, K.ct_w), P(c, K.ct_b), K.ct_cin, K.ct_cout, K.ct_w3, K.ct_b4, s));
      FU_TRY(launch_pack_conv3x3(c->prec, K.ct_w3, 4 * K.ct_cout, K.ct_cin, K.ct_cin, K.ct_wf, K.ct_wd, s));
    }
  }
  c->packed_dirty = false;
  c->packed_eval = eval;
  return 0;
}

}  // namespace fu
