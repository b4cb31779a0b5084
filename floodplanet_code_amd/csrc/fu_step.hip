// One training / inference step over the plan of a context (fu_ctx.h): the forward pass, the backward pass block by
// block with the weight-gradient chains on the side stream, the late-fusion convs, the per-launch profiler slots and
// the FLOP count.  The entry points of fu_api.hip check their arguments and call forward_impl / backward_block_impl.
#include "fu_ctx.h"

namespace fu {

// the event pair for ONE conv / wgrad launch (empty when profiling is off): goes into that launch's ConvIn::opt.prof
static ProfSlot prof_arm(fu_ctx* c, int cls, double flops) {
  Profiler& pr = c->prof;
  ProfSlot ps;
  if (!pr.on) return ps;
  if (pr.next + 2 > pr.pool.size()) { pr.overflow = true; return ps; }
  ProfRec r{cls, flops, pr.pool[pr.next], pr.pool[pr.next + 1]};
  pr.next += 2;
  pr.recs.push_back(r);
  ps.start = r.e0;
  ps.stop = r.e1;
  return ps;
}

// decoder inputs: the feature of `level` (skip connection) and the low-resolution input of up block i
static Feat level_feat(fu_ctx* c, int level) {
  if (c->fusion) { Fuse& F = c->fuse[level]; return Feat{F.y, nullptr, nullptr, F.gy, F.C}; }
  Conv& v = c->blk[level].c[1];
  return Feat{v.y, v.a, v.b, v.gy, v.cout};
}
static Feat low_feat(fu_ctx* c, int i) {
  if (i == 5 * c->nE) return level_feat(c, 4);
  Conv& v = c->blk[i - 1].c[1];
  return Feat{v.y, v.a, v.b, v.gy, v.cout};
}

static ConvIn conv_input(fu_ctx* c, int i, int j) {
  Block& K = c->blk[i];
  ConvIn in;
  in.src1 = nullptr; in.C1 = 0; in.a0 = nullptr; in.b0 = nullptr;
  if (j == 1) {
    in.src0 = K.c[0].y; in.C0 = K.c[0].cout; in.a0 = K.c[0].a; in.b0 = K.c[0].b;
  } else if (K.kind == BK_INC) {
    in.src0 = c->xin[K.enc]; in.C0 = c->cin_pad0[K.enc];
  } else if (K.kind == BK_DOWN) {
    in.src0 = K.pooled; in.C0 = K.c[0].cin_real;
  } else {
    const Feat sk = level_feat(c, K.skip);
    in.src0 = sk.y; in.C0 = sk.C; in.a0 = sk.a; in.b0 = sk.b;
    in.src1 = K.up; in.C1 = K.c[0].cin_real - sk.C;
  }
  return in;
}

static int conv_fwd(fu_ctx* c, int i, int j, int B, bool training, hipStream_t s) {
  Conv& v = c->blk[i].c[j];
  const int H = c->Hs[v.level], W = c->Ws[v.level];
  ConvIn in = conv_input(c, i, j);
  int nt = 0;
  const double fl = 2.0 * 9 * v.cin_real * v.cout * (double)B * H * W;
  in.opt.prof = prof_arm(c, FU_K_CONV3X3, fl);
  // eval: the packed weights and v.fold_bias already contain the BatchNorm (repack(eval)); y IS bn(conv(x)), v.a / v.b = 1 / 0
  FU_TRY(launch_conv3x3(c->prec, in, v.wf, training ? P(c, v.p_b) : v.fold_bias, v.y, v.cout, nullptr, 0,
                        training ? c->stats : nullptr, &nt, B, H, W, s));
  const int64_t off = c->bns[v.bn].off;
  if (training) {
    BnFwdOut o;
    o.conv_bias = P(c, v.p_b); o.gamma = P(c, v.p_g); o.beta = P(c, v.p_beta);
    o.eps = BN_EPS; o.momentum = BN_MOMENTUM;
    o.mean = v.mean; o.invstd = v.invstd; o.a = v.a; o.b = v.b;
    o.rmean = c->RM + off; o.rvar = c->RV + off; o.nbt = c->NBT + v.bn;
    FU_TRY(launch_bn_finalize(o, c->stats, nt, v.cout, (int64_t)B * H * W, c->dscratch, active_sync(c, training), s));
  }
  return 0;
}

// Late fusion, all five levels (lf_model.py:78-90).  forward: cat <- [relu(bn(x_e))]_e ; fused = W * cat + bias.
static int fuse_forward(fu_ctx* c, int B, hipStream_t s) {
  for (int l = 0; l < 5; ++l) {
    Fuse& F = c->fuse[l];
    const int Ccat = c->nE * F.C, H = c->Hs[l], W = c->Ws[l];
    const int64_t npix = (int64_t)B * H * W;
    for (int e = 0; e < c->nE; ++e) {
      Conv& v = c->blk[5 * e + l].c[1];
      FU_TRY(launch_copy_channels(c->prec, v.y, v.cout, 0, v.a, v.b, F.cat, Ccat, e * F.C, F.C, npix, s));
    }
    ConvIn in{F.cat, Ccat, nullptr, nullptr, nullptr, 0, true};   // 1x1: only the centre tap of wf is non-zero
    FU_TRY(launch_conv3x3(c->prec, in, F.wf, P(c, F.p_b), F.y, F.C, nullptr, 0, nullptr, nullptr, B, H, W, s));
  }
  return 0;
}

// backward of the five fusion convs: needs every F.gy (complete after up1's backward); writes dL/d(activated feature)
// of every encoder level ("=": the encoders' pool backward accumulates into it afterwards, as the skip gradient of
// the plain UNet) and the fusion parameters' gradients
static int fuse_backward(fu_ctx* c, int B, hipStream_t s) {
  for (int l = 4; l >= 0; --l) {
    Fuse& F = c->fuse[l];
    const int Ccat = c->nE * F.C, H = c->Hs[l], W = c->Ws[l];
    const int64_t npix = (int64_t)B * H * W;
    int ndbp = 0;
    FU_TRY(launch_channel_partial_sums(c->prec, F.gy, F.C, npix, c->db_part, &ndbp, s));
    ConvIn in{F.cat, Ccat, nullptr, nullptr, nullptr, 0, true};   // only the centre tap of dw3 is computed (and read)
    in.opt.unscale = grad_unscale(c);
    FU_TRY(launch_conv3x3_wgrad(c->prec, in, F.gy, F.C, c->slab, F.dw3, Ccat, c->db_part, ndbp, G(c, F.p_b), B, H, W,
                                s));
    FU_TRY(launch_center_from_w3(F.dw3, (int64_t)F.C * Ccat, G(c, F.p_w), s));
    ConvIn gin{F.gy, F.C, nullptr, nullptr, nullptr, 0, true};    // the flipped 3x3 of a centre tap is a centre tap
    if (c->nE == 2 && F.C % 64 == 0) {
      // two encoders: the conv kernels' two destinations ARE the encoders' skip gradients (no concat gradient, no split)
      FU_TRY(launch_conv3x3(c->prec, gin, F.wd, nullptr, c->blk[l].c[1].gy, F.C, c->blk[5 + l].c[1].gy, F.C, nullptr,
                            nullptr, B, H, W, s));
    } else {
      FU_TRY(launch_conv3x3(c->prec, gin, F.wd, nullptr, F.gcat, Ccat, nullptr, 0, nullptr, nullptr, B, H, W, s));
      for (int e = 0; e < c->nE; ++e) {
        Conv& v = c->blk[5 * e + l].c[1];
        FU_TRY(launch_copy_channels(c->prec, F.gcat, Ccat, e * F.C, nullptr, nullptr, v.gy, v.cout, 0, F.C, npix, s));
      }
    }
  }
  return 0;
}

int forward_impl(fu_ctx* c, const float* x, const SrcList* srcs, int B, bool training, float* logits_out,
                 hipStream_t s, int n_views, unsigned view_codes) {
  const fu_config& f = c->cfg;
  c->view_n = 0;
  if (c->packed_dirty || c->packed_eval != !training) FU_TRY(repack(c, s, !training));
  for (int e = 0; e < c->nE; ++e) {
    if (n_views > 0)   // test-time augmentation (fu_forward_views): sample v * (B / n_views) + b = view v of crop b
      FU_TRY(launch_gather_views_nchw_to_nhwc(c->prec, *srcs, c->xin[e], B / n_views, n_views, view_codes, c->enc_ch[e],
                                              f.height, f.width, c->cin_pad0[e], c->enc_coff[e], s));
    else if (srcs)     // several input tensors side by side (fu_forward_srcs): the concat happens inside the layout conversion
      FU_TRY(launch_gather_nchw_to_nhwc(c->prec, *srcs, c->xin[e], B, c->enc_ch[e], f.height, f.width, c->cin_pad0[e],
                                        c->enc_coff[e], s));
    else
      FU_TRY(launch_nchw_to_nhwc(c->prec, x, c->xin[e], B, c->enc_ch[e], f.height, f.width, c->cin_pad0[e], s,
                                 f.n_channels, c->enc_coff[e]));
  }
  for (int i = 0; i < c->nb; ++i) {
    Block& K = c->blk[i];
    if (c->fusion && i == 5 * c->nE) FU_TRY(fuse_forward(c, B, s));
    if (K.kind == BK_DOWN) {
      Conv& pv = c->blk[i - 1].c[1];
      FU_TRY(launch_maxpool2(c->prec, pv.y, pv.a, pv.b, K.pooled, B, c->Hs[pv.level], c->Ws[pv.level], pv.cout, s));
    } else if (K.kind == BK_UP) {
      const Feat pv = low_feat(c, i);
      const int h = c->Hs[K.level + 1], w = c->Ws[K.level + 1], H = c->Hs[K.level], W = c->Ws[K.level];
      if (c->cfg.bilinear) {
        FU_TRY(launch_upsample2(c->prec, pv.y, pv.a, pv.b, K.up, B, h, w, pv.C, H, W, K.upt, s));
      } else {
        // ConvTranspose2d(k2,s2) (unet.py:48-51): the four phase GEMMs as one 1x1 conv of relu(bn(low)) with 4 ct_cout
        // output channels at the low resolution, then depth-to-space + F.pad (unet.py:57-62)
        ConvIn lin{pv.y, pv.C, pv.a, pv.b, nullptr, 0, true};
        FU_TRY(launch_conv3x3(c->prec, lin, K.ct_wf, K.ct_b4, K.u, 4 * K.ct_cout, nullptr, 0, nullptr, nullptr, B, h, w, s));
        FU_TRY(launch_depth_to_space(c->prec, K.u, K.up, B, h, w, K.ct_cout, H, W, s));
      }
    }
    FU_TRY(conv_fwd(c, i, 0, B, training, s));
    FU_TRY(conv_fwd(c, i, 1, B, training, s));
  }
  Conv& last = c->blk[c->nb - 1].c[1];
  FU_TRY(launch_head_fwd(c->prec, last.y, last.a, last.b, P(c, c->p_outw), P(c, c->p_outb), f.base_channels,
                         f.n_classes, B, f.height, f.width, c->logits, logits_out, s));
  c->last_batch = B;
  c->view_n = n_views;
  c->view_batch = n_views > 0 ? B / n_views : 0;
  c->view_codes = view_codes;
  c->fwd_training = training;
  c->have_loss = false;
  c->have_up_scale = false;
  return 0;
}

// testing hook (fu_test_bnb_separate): 1 = BatchNorm-backward sums always by their own reduce pass, never from the
// producer of the gradient (BnbFuse, fu_common.h)
static int g_bnb_separate = 0;
static int g_head_store_g = 0;   // testing hook (fu_test_head_store_g): the head backward stores its data gradient even where the apply pass could recompute it
// testing hook (fu_test_perturb_bnb_sums): the fused sums are multiplied by this factor after the kernel that emitted
// them -- the negative control of the parity tests (a wrong fused sum must make them fail); 1 = off, no launch
static float g_test_perturb_bnb = 1.f;
static __global__ void k_scale_floats(float* x, int64_t n, float f) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= f;
}
int perturb_bnb(float* part, int tiles, int C, hipStream_t s) {
  if (g_test_perturb_bnb == 1.f || tiles <= 0) return 0;
  hipLaunchKernelGGL(k_scale_floats, dim3(256), dim3(256), 0, s, part, (int64_t)tiles * C * 2, g_test_perturb_bnb);
  return hipGetLastError() == hipSuccess ? 0 : FU_ERR_HIP;
}

static int backward_conv(fu_ctx* c, int i, int j, int B, hipStream_t s) {
  Block& K = c->blk[i];
  Conv& v = K.c[j];
  const int H = c->Hs[v.level], W = c->Ws[v.level];
  const int64_t npix = (int64_t)B * H * W;
  int ndb = 0;
  // BN + ReLU backward: gy <- dL/dy ; dgamma, dbeta
  // The weight-gradient chain of this conv (wgrad, slab reduce, transpose) depends only on gy and on saved activations
  // and nothing in the rest of backward depends on it: it runs on a side stream, concurrently with this conv's dgrad
  // and the next BN backward (its 8-wave workgroups spend more than half of every stage staging with the MFMA pipe
  // idle, measured with s_memtime stamps; the dgrad workgroups that fit beside them on a CU use it).
  // The main stream never waits for that chain inside a backward.  The one buffer the two share, the bias-gradient partials
  // (written by launch_bn_bwd here, read by the slab reduce there), is this conv's own (Conv::db_part), so nothing inside
  // one backward reuses it.  Its next writer is the launch_bn_bwd of the SAME conv in the next backward, and every way there
  // passes a join_side behind this conv's reduce, in the order of the stream that then writes:
  //   fu_backward                    joins after its last block;
  //   fu_backward_block, mode 1      joins at the end of this very block;
  //   fu_backward_block, mode 2      the caller's fu_backward_join after the last block (the optimizer step needs it); a
  //                                  caller that left it out is caught by the join at block 0 below (side_open);
  //   mode 0                         there is no second stream;
  //   a repeated backward of one loss is one of the above twice: the first one's join is in front of the second one's block 0;
  //   fuse_backward                  joins first and then uses the context's buffer (c->db_part), like the ConvTranspose path,
  //                                  which exists only without a side stream;
  //   the last chain of a backward   (`tail` below) runs on the caller's stream itself, behind this launch_bn_bwd: the next
  //                                  writer of its db_part is a launch on that same stream, ordered by the stream with no join
  //                                  at all -- and so is its private workspace (slab_tail), which no other chain touches.
  // (A backward on another stream than the one that joined is ordered by the caller, as for every other buffer of the context.)
  const bool side = c->side != nullptr && c->side_mode != 0;
  float* dbp = v.db_part;
  BnBwdArgs A;
  A.g = v.gy; A.y = v.y; A.C = v.cout; A.npix = npix;
  A.a = v.a; A.b = v.b; A.mean = v.mean; A.invstd = v.invstd;
  A.dgamma = G(c, v.p_g); A.dbeta = G(c, v.p_beta);
  A.partials = c->bnb_part; A.coef = v.coef; A.db_partials = dbp; A.n_db_partials = &ndb; A.dscratch = c->dscratch;
  A.sync = active_sync(c, true); A.unscale = grad_unscale(c);
  A.g_pool = v.pool_g; A.B = B; A.H = H; A.W = W;
  A.ext_partials = v.bnb_tiles;
  A.head = v.head.dl ? &v.head : nullptr;
  FU_TRY(launch_bn_bwd(c->prec, A, s));
  v.pool_g = nullptr;
  v.bnb_tiles = 0;
  v.head = HeadGrad{};
  // weight (and bias) gradient
  ConvIn in = conv_input(c, i, j);
  const double fl = 2.0 * 9 * v.cin_real * v.cout * (double)B * H * W;
  // The last chain of a backward (the first conv of the encoder that is processed last: no data gradient, so nothing is left
  // on the caller's stream to run beside it) stays on the caller's stream: the hop to the side stream and back would only add
  // its hand-off latency in front of the optimiser step.  The chain before it may still be reducing out of c->slab on the
  // side stream, so this one has a workspace of its own.
  const bool tail = side && c->slab_tail != nullptr && i == 0 && j == 0;
  hipStream_t ws = s;
  if (side && !tail) {
    FU_HIP_CHECK(hipEventRecord(c->ev_gy, s));
    FU_HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_gy, 0));
    ws = c->side;
    c->side_open = true;
  }
  in.opt.prof = prof_arm(c, FU_K_WGRAD, fl);
  in.opt.unscale = A.unscale;
  FU_TRY(launch_conv3x3_wgrad(c->prec, in, v.gy, v.cout, tail ? c->slab_tail : c->slab, G(c, v.p_w), v.cin_real, dbp, ndb,
                              G(c, v.p_b), B, H, W, ws));
  // data gradient
  ConvIn din{v.gy, v.cout, nullptr, nullptr, nullptr, 0};
  if (!(K.role == 0 && j == 0)) din.opt.prof = prof_arm(c, FU_K_CONV3X3, fl);
  if (j == 1) {
    // this dgrad's destination is dL/d relu(bn(y)) of the block's first conv: a kernel that can (the row-stationary 16-bit
    // one) also leaves that BatchNorm's backward sums in bnb_part, consumed by the very next launch_bn_bwd on this stream
    Conv& v0 = K.c[0];
    const bool separate = g_bnb_separate != 0;      // testing hook: always the separate reduce pass
    int tiles = 0;
    BnbFuse f;
    if (c->prec != PREC_F32 && !A.sync && !separate) {
      f = bnb_fuse(v0.y, v0.a, v0.b, v0.mean, v0.invstd, c->bnb_part, c->bnb_cap, &tiles);
      din.opt.bnb = &f;
    }
    FU_TRY(launch_conv3x3(c->prec, din, v.wd, nullptr, v0.gy, v0.cout, nullptr, 0, nullptr, nullptr, B, H, W, s));
    v0.bnb_tiles = tiles;
    FU_TRY(perturb_bnb(c->bnb_part, tiles, v0.cout, s));
  } else if (K.kind == BK_DOWN) {
    FU_TRY(launch_conv3x3(c->prec, din, v.wd, nullptr, K.g_pooled, v.cin_real, nullptr, 0, nullptr, nullptr, B, H, W,
                          s));
    // the pool's backward (route g_pooled to the first argmax of every window, add to the skip gradient) is folded into
    // the BN backward of the pooled tensor: the next backward block on this stream (k_bn_bwd_pool)
    Conv& pv = c->blk[i - 1].c[1];
    pv.pool_g = K.g_pooled;
  } else if (K.kind == BK_UP) {
    const Feat sk = level_feat(c, K.skip);
    const Feat pv = low_feat(c, i);
    FU_TRY(launch_conv3x3(c->prec, din, v.wd, nullptr, sk.gy, sk.C, K.g_up, v.cin_real - sk.C, nullptr, nullptr,
                          B, H, W, s));
    const int h = c->Hs[K.level + 1], w = c->Ws[K.level + 1];
    if (c->cfg.bilinear) {
      FU_TRY(launch_upsample2_bwd(c->prec, K.g_up, pv.gy, B, h, w, pv.C, H, W, K.upt, s));
    } else {
      // g4 = space-to-depth of dL/d(up) (the F.pad region carries no gradient: it is simply not gathered); the 1x1 conv's
      // bias gradient is the sum of g4 over pixels and phases, its weight gradient a one-tap wgrad, its data gradient a
      // 1x1 conv with the transposed weights
      FU_TRY(launch_space_to_depth(c->prec, K.g_up, K.g_u, B, h, w, K.ct_cout, H, W, s));
      int ndbp = 0;
      FU_TRY(launch_channel_partial_sums(c->prec, K.g_u, K.ct_cout, (int64_t)B * h * w * 4, c->db_part, &ndbp, s));
      FU_TRY(launch_colsum_partials(c->db_part, ndbp, K.ct_cout, A.unscale, G(c, K.ct_b), s));
      ConvIn lin{pv.y, pv.C, pv.a, pv.b, nullptr, 0, true};
      lin.opt.unscale = A.unscale;
      FU_TRY(launch_conv3x3_wgrad(c->prec, lin, K.g_u, 4 * K.ct_cout, c->slab, K.ct_dw3, K.ct_cin, nullptr, 0, nullptr, B, h,
                                  w, s));
      FU_TRY(launch_convT_grad_from_w3(K.ct_dw3, K.ct_cin, K.ct_cout, G(c, K.ct_w), s));
      ConvIn gin{K.g_u, 4 * K.ct_cout, nullptr, nullptr, nullptr, 0, true};
      FU_TRY(launch_conv3x3(c->prec, gin, K.ct_wd, nullptr, pv.gy, K.ct_cin, nullptr, 0, nullptr, nullptr, B, h, w, s));
    }
  }
  return 0;
}

int join_side(fu_ctx* c, hipStream_t s) {
  if (c->side && c->side_mode != 0) {
    FU_HIP_CHECK(hipEventRecord(c->ev_blk, c->side));
    FU_HIP_CHECK(hipStreamWaitEvent(s, c->ev_blk, 0));
    c->side_open = false;
  }
  return 0;
}

// backward order: 0 = head, 1..4 = up4..up1, [5 = the fusion convs], then down4..inc of the last encoder ... the first
int num_backward_blocks(const fu_ctx* c) { return 5 + (c->fusion ? 1 : 0) + 5 * c->nE; }
int backward_block_index(const fu_ctx* c, int block) {
  if (block <= 4) return c->nb - block;                       // nb-1 (up4) ... nb-4 (up1)
  const int k = block - 5 - (c->fusion ? 1 : 0);              // 0 .. 5*nE-1 over the encoders, last encoder first
  return 5 * c->nE - 1 - k;
}

int backward_block_impl(fu_ctx* c, int block, const float* dlogits_ext, hipStream_t s, bool join) {
  const fu_config& f = c->cfg;
  const int B = c->last_batch;
  if (block == 0) {
    // a mode-2 caller that started over without fu_backward_join: the chains of the last backward still read the
    // per-conv bias-gradient partials that this one is about to write (backward_conv)
    if (c->side_open) FU_TRY(join_side(c, s));
    if (dlogits_ext) {
      FU_TRY(launch_dlogits_from_nchw(dlogits_ext, c->dlogits, f.n_classes, B, f.height, f.width, s));
      c->have_up_scale = false;     // the caller's dlogits IS the whole upstream gradient
    } else {
      FU_REQUIRE(c->have_loss, "fu_backward: no dlogits given and no fu_loss_* call since the last forward");
    }
    // What the head backward reads: the stored gradient itself, or -- out of place, so that a repeated backward of the same
    // loss starts from the same input -- times the upstream gradient of loss.backward() and, for fp16 gradient maps, the
    // power-of-two loss scale chosen from max|dL/dlogits| (grad_unscale: taken out again where parameter gradients are written)
    const float* dl = c->dlogits;
    if (c->prec == PREC_F16 || c->have_up_scale) {
      FU_TRY(launch_loss_grad_eff(c->dlogits, c->dlogits_eff, (int64_t)B * f.height * f.width * f.n_classes,
                                  c->have_up_scale ? c->up_scale : nullptr, c->ce_part,
                                  c->prec == PREC_F16 ? c->loss_scale : nullptr, s,
                                  c->prec == PREC_F16 ? c->guard : nullptr));
      dl = c->dlogits_eff;
    }
    Conv& last = c->blk[c->nb - 1].c[1];
    // the head's data gradient is dL/d relu(bn(y)) of the last conv: it can leave that BatchNorm's backward sums behind
    BnbFuse fz;
    int tiles = 0;
    const bool want = c->prec != PREC_F32 && !active_sync(c, true) && !g_bnb_separate;
    if (want) {
      fz = bnb_fuse(last.y, last.a, last.b, last.mean, last.invstd, c->bnb_part, c->bnb_cap, &tiles);
      // ... and then g = dl . w need not be stored at all: the apply pass of that BatchNorm recomputes it (HeadGrad)
      fz.skip_g = last.cout % 8 == 0 && 2048 % last.cout == 0 && !g_head_store_g;
    }
    FU_TRY(launch_head_bwd(c->prec, dl, last.y, last.a, last.b, P(c, c->p_outw), f.base_channels, f.n_classes,
                           (int64_t)B * f.height * f.width, last.gy, c->hb_part, G(c, c->p_outw), G(c, c->p_outb),
                           grad_unscale(c), s, want ? &fz : nullptr));
    last.bnb_tiles = tiles;
    FU_REQUIRE(!(want && fz.skip_g) || tiles > 0, "head backward: the fused BatchNorm sums were refused (partials %lld floats)",
               (long long)c->bnb_cap);
    last.head = HeadGrad{};
    if (want && fz.skip_g) { last.head.dl = dl; last.head.w = P(c, c->p_outw); last.head.ncls = f.n_classes; }
    FU_TRY(perturb_bnb(c->bnb_part, tiles, last.cout, s));
    return 0;
  }
  if (c->fusion && block == 5) {
    // shares the slab and the bias-gradient partials with the side stream's weight-gradient chain: join it first (the
    // encoders' chains that follow are ordered behind this block by their ev_gy events)
    FU_TRY(join_side(c, s));
    return fuse_backward(c, B, s);
  }
  const int i = backward_block_index(c, block);
  FU_TRY(backward_conv(c, i, 1, B, s));
  FU_TRY(backward_conv(c, i, 0, B, s));
  if (join) FU_TRY(join_side(c, s));   // the block's gradients are complete (for the caller's all-reduce / Adam) once the side stream is
  return 0;
}

double conv_flops(fu_ctx* c, bool train) {
  double fwd = 0.0, first = 0.0;
  for (int i = 0; i < c->nb; ++i)
    for (int j = 0; j < 2; ++j) {
      const Conv& v = c->blk[i].c[j];
      const double fl = 2.0 * 9 * v.cin_real * v.cout * c->Hs[v.level] * c->Ws[v.level];
      if (c->blk[i].role == 0 && j == 0) first += fl;      // the encoders' first convs have no data gradient
      fwd += fl;
    }
  for (int l = 0; l < 5 && c->fusion; ++l)                   // the 1x1 fusion convs (the MACs they need, not the 3x3 run)
    fwd += 2.0 * c->nE * c->fuse[l].C * c->fuse[l].C * c->Hs[l] * c->Ws[l];
  if (!c->cfg.bilinear)
    for (int i = 5 * c->nE; i < c->nb; ++i) {
      const Block& K = c->blk[i];
      fwd += 2.0 * 4 * K.ct_cin * K.ct_cout * c->Hs[K.level + 1] * c->Ws[K.level + 1];
    }
  fwd += 2.0 * c->cfg.base_channels * c->cfg.n_classes * c->cfg.height * c->cfg.width;
  return train ? 3.0 * fwd - first : fwd;
}

}  // namespace fu

extern "C" void fu_test_bnb_separate(int on) { fu::g_bnb_separate = on ? 1 : 0; }
extern "C" void fu_test_head_store_g(int on) { fu::g_head_store_g = on ? 1 : 0; }
extern "C" void fu_test_perturb_bnb_sums(float factor) { fu::g_test_perturb_bnb = factor; }
