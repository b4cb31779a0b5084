// Private to the library (never installed): the context behind the opaque fu_ctx of include/floodunet.h, the static
// execution plan it holds, and the functions of fu_plan.hip / fu_step.hip that other files call.  (The layout of the
// data in HBM is described at the top of fu_api.hip.)
#pragma once
#include "../../include/floodunet.h"
#include "fu_common.h"
#include "fu_optim.h"

#include <string>
#include <vector>

namespace fu {

// one launch packs every conv layer: device table of layers, element ranges by prefix sum
struct PackDesc {
  int64_t start;      // first packed element of this layer in the global element numbering
  int64_t w_off;      // offset of the OIHW weight in the flat parameter buffer
  int cout, cin_real, cin_pad, pad_;
  void* wf;
  void* wd;
  int tile_start, tiles_ci;   // bf16 tiled pack: first 32x32 (co x ci) tile of this layer, tiles along ci
  const float* scale;         // eval pack: per-output-channel factor gamma * invstd of the BatchNorm behind the conv
};
constexpr int MAX_PACK = 32;
struct PackTable { PackDesc d[MAX_PACK]; int n; int64_t total; int tiles; };

constexpr float BN_EPS = 1e-5f;
constexpr float BN_MOMENTUM = 0.1f;

struct ParamInfo {
  std::string name;
  int ndim;
  int64_t shape[4];
  int64_t off, numel;
};
struct BnInfo {
  std::string name;
  int C;
  int64_t off;
};

struct Conv {
  int cin_real = 0, cin_pad = 0, cout = 0, level = 0;
  int p_w = -1, p_b = -1, p_g = -1, p_beta = -1, bn = -1;
  void* wf = nullptr;
  void* wd = nullptr;
  float *mean = nullptr, *invstd = nullptr, *a = nullptr, *b = nullptr, *coef = nullptr;
  float *fold_scale = nullptr, *fold_bias = nullptr;   // eval pack (k_bn_fold_eval)
  void* y = nullptr;
  void* gy = nullptr;
  float* db_part = nullptr;       // backward: this conv's OWN bias-gradient partials (written by its BN backward on the caller's
                                  // stream, read by its slab reduce on a side stream; see backward_conv for the reuse order)
  const void* pool_g = nullptr;   // backward: dL/d(maxpool(this output)), to be folded into this conv's BN backward
  int bnb_tiles = 0;              // backward: > 0 = the producer of gy left this many rows of BN-backward sums in bnb_part
  HeadGrad head;                  // backward, last conv only: gy was not stored, the BN-backward apply recomputes it (dl != null)
};

enum BlockKind { BK_INC = 0, BK_DOWN = 1, BK_UP = 2 };

struct Block {
  Conv c[2];
  int kind = BK_INC, level = 0;
  int enc = 0;                // BK_INC / BK_DOWN: encoder this block belongs to
  int role = 0;               // 0..8 = inc, down1..4, up1..4 (names, flops)
  int skip = -1;              // BK_UP: level whose feature is concatenated first
  void* pooled = nullptr;     // BK_DOWN: maxpool output (input of c[0])
  void* g_pooled = nullptr;
  void* up = nullptr;         // BK_UP: upsampled + padded low-resolution input
  void* g_up = nullptr;
  UpTables upt;
  // bilinear=False: ConvTranspose2d(ct_cin, ct_cout, 2, 2) = one 1x1 conv ct_cin -> 4 ct_cout (phase-major) at the low
  // resolution + depth-to-space
  int ct_w = -1, ct_b = -1, ct_cin = 0, ct_cout = 0;
  void* u = nullptr;          // y4: the 1x1 conv's output [B, h, w, 4 ct_cout]
  void* g_u = nullptr;        // g4: its gradient (space-to-depth of dL/d up)
  float* ct_w3 = nullptr;     // embedded OIHW weight [4 ct_cout][ct_cin][3][3] (fp32, centre tap only)
  float* ct_dw3 = nullptr;    // its gradient
  float* ct_b4 = nullptr;     // bias repeated per phase [4 ct_cout]
  void* ct_wf = nullptr;      // packed forward / dgrad copies
  void* ct_wd = nullptr;
  int first_param = 0, num_params = 0;  // contiguous range in the canonical parameter table
};

// Late fusion, one per level (lf_model.py:40-45, 78-90): fused = Conv2d(nE*C, C, 1)(cat_e relu(bn(x_e)))
struct Fuse {
  int p_w = -1, p_b = -1, C = 0;
  void* cat = nullptr;        // [pixels][nE*C]: activated encoder features side by side
  void* gcat = nullptr;       // its gradient
  void* y = nullptr;          // fused feature (plain: no BN / ReLU follows)
  void* gy = nullptr;         // its gradient (written by the decoder's backward)
  float* w3 = nullptr;        // the 1x1 weight as the centre tap of a 3x3 one, OIHW fp32
  float* dw3 = nullptr;
  void* wf = nullptr;         // packed forward / dgrad copies
  void* wd = nullptr;
};

// what the decoder reads at one level: the encoder's own conv output (plain UNet) or the fused feature
struct Feat { void* y; float* a; float* b; void* gy; int C; };

struct ProfRec { int cls; double flops; hipEvent_t e0, e1; };
struct Profiler {
  bool on = false;
  std::vector<hipEvent_t> pool;   // pairs
  size_t next = 0;
  std::vector<ProfRec> recs;
  bool overflow = false;
};

struct Arena {
  struct Req { void** slot; size_t bytes; };
  std::vector<Req> reqs;
  char* base = nullptr;
  size_t total = 0;
  template <typename T> void want(T** slot, size_t bytes) {
    reqs.push_back({reinterpret_cast<void**>(slot), bytes});
  }
  int commit() {
    size_t off = 0;
    for (auto& r : reqs) off += (r.bytes + 255) & ~(size_t)255;
    total = off ? off : 256;
    FU_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&base), total));
    FU_HIP_CHECK(hipMemset(base, 0, total));
    off = 0;
    for (auto& r : reqs) {
      *r.slot = base + off;
      off += (r.bytes + 255) & ~(size_t)255;
    }
    return 0;
  }
};

// The optimiser's state in a context: what fu_optim_api.hip's entry points bind, arm and read
struct OptimState {
  float* adam_m = nullptr;        // bound (caller-owned, fu_bind_adam_state): the moments outlive the context
  float* adam_v = nullptr;
  float* ema_p = nullptr;         // bound (caller-owned, fu_bind_ema_state): the weight EMA and the EMA of the running statistics
  float* ema_rm = nullptr;
  float* ema_rv = nullptr;
  double clip_max_norm = 0.0;     // fu_set_grad_clip: > 0 = the optimiser step clips the global gradient norm to it
  GradClip clip;                  // its chunk table, partials, state block and scalars (made at the first use; extra_allocs)
  double weight_decay = 0.0;      // fu_set_weight_decay: > 0 = the optimiser step decays the flagged tensors (AdamW)
  std::vector<uint8_t> wd_mask;   // its per-tensor flags in parameter order (empty: never armed)
  int64_t* wd_bounds = nullptr;   // device: the sorted bounds of the decayed ranges (AdamDecay; extra_allocs, made once)
  int wd_nb = 0;                  // bounds in use (0: no tensor decays -- the plain kernels run)
};

}  // namespace fu

struct Dp;   // fu_dp.hip
struct fu_ctx {
  fu_config cfg;
  fu::Prec prec;
  size_t esize;
  int Hs[5], Ws[5], ch[5];
  int nE = 1;                  // encoders (1 for the plain UNet)
  bool fusion = false;         // late fusion: nE encoders -> 5 fusion convs -> decoder
  int nb = 9;                  // blocks: 5 per encoder (inc, down1..4), then up1..4
  int enc_ch[FU_MAX_ENCODERS] = {0}, enc_coff[FU_MAX_ENCODERS] = {0}, cin_pad0[FU_MAX_ENCODERS] = {0};
  void* xin[FU_MAX_ENCODERS] = {nullptr};
  std::vector<fu::ParamInfo> params;
  std::vector<fu::BnInfo> bns;
  int64_t total_params = 0, total_bn = 0;
  std::vector<fu::Block> blk;
  fu::Fuse fuse[5];
  int p_outw = -1, p_outb = -1;
  // bound (caller-owned)
  float* P = nullptr;
  float* G = nullptr;
  float* RM = nullptr;
  float* RV = nullptr;
  int64_t* NBT = nullptr;
  bool packed_dirty = true;
  bool packed_eval = false;       // the packed copies hold the eval-folded weights (BatchNorm inside) rather than the plain ones
  // owned
  fu::Arena arena;
  std::vector<void*> extra_allocs;
  float* logits = nullptr;
  float* dlogits = nullptr;        // dL/dlogits as fu_loss_* (or the caller) left it: never modified by a backward
  float* dlogits_eff = nullptr;    // times the upstream gradient / the fp16 loss scale (launch_loss_grad_eff)
  float* up_scale = nullptr;       // device scalar: upstream gradient of the loss (fu_scale_loss_grad)
  bool have_up_scale = false;
  float* stats = nullptr;
  float* bnb_part = nullptr;
  int64_t bnb_cap = 0;         // floats
  float* db_part = nullptr;       // bias-gradient partials of the launches that run on the caller's stream behind a join: the
                                  // fusion convs and the ConvTranspose path (every 3x3 conv of the plan has its own: Conv::db_part)
  hipStream_t side = nullptr;     // side stream for the weight-gradient chain (wgrad + slab reduce + transpose): one of ...
  hipStream_t side_lo = nullptr;  // ... lowest priority (mode 1: nothing but the final join waits for that chain; the main chain
                                  //     conv -> BN backward -> conv is the critical path and gets the CUs first: measured
                                  //     5.66 -> 5.64 ms per step and 0.338 -> 0.350 of peak for the conv launches in the step)
  hipStream_t side_def = nullptr; // ... the default priority (mode 2: an all-reduce bucket waits for its weight gradients)
  hipEvent_t ev_gy = nullptr, ev_blk = nullptr;
  hipEvent_t ev_fence[2] = {nullptr, nullptr};   // fu_backward_fence: compute stream / side stream (created on first use)
  int side_mode = 1;              // fu_set_side_stream: 0 off, 1 on (blocks join), 2 on (the caller joins: fu_backward_join)
  bool side_open = false;         // weight-gradient chains were queued on the side stream since the last join_side
  double* dscratch = nullptr;
  fu::SyncDesc sync;           // exact data-parallel mode (fu_set_exact_sync); hook == nullptr: off
  float* slab = nullptr;
  float* slab_tail = nullptr;     // split-K workspace of the LAST weight-gradient chain of a backward alone (blk[0].c[0], which runs on
                                  // the caller's stream while the chain before it may still use `slab` on the side stream: backward_conv)
  float* ce_part = nullptr;
  float* hb_part = nullptr;
  float* loss_dev = nullptr;
  float* ce_wsum = nullptr;       // fu_loss_ce_weighted / _focal: D = sum of w[target] over the valid pixels, read by the gradient kernel
  float* region_coef = nullptr;   // fu_loss_ce_region: A_k, B_k and lambda of the region term (REGION_COEF_BYTES), read by its gradient pass
  float* loss_scale = nullptr;    // fp16 mode: {S, 1/S} of the running backward (fu_common.h, launch_loss_grad_eff)
  int* guard = nullptr;           // fp16 mode: non-finite flag / skipped steps / back-off exponent / clean steps (k_guard_book)
  unsigned long long* conf_tmp = nullptr;
  int64_t* n_valid = nullptr;
  fu::DeviceTable stitch_table, scene_table, train_table;   // fu_stitch_add_batch[_probs, _windowed] / fu_scene_crops / fu_scene_train_tiles[_ex]
  fu::OptimState opt;             // everything the optimiser step keeps (fu_optim_api.hip)
  fu::Profiler prof;
  struct Dp* dp = nullptr;            // fu_dp_init: RCCL communicator, communication stream, events
  std::vector<fu::PackTable> pack_tabs;   // <= MAX_PACK layers per launch
  // state
  int last_batch = 0;
  int view_n = 0;                 // fu_forward_views: views of the last forward (0: the last forward was not one) ...
  int view_batch = 0;             // ... crops per view ...
  unsigned view_codes = 0;        // ... and their codes, 3 bits per view (fu_merge_views)
  bool fwd_training = false;
  bool have_loss = false;
};

namespace fu {

inline float* P(fu_ctx* c, int idx) { return c->P + c->params[idx].off; }
inline float* G(fu_ctx* c, int idx) { return c->G + c->params[idx].off; }

// The exact-sync descriptor that the statistics launchers of one call get: the context's where fu_set_exact_sync armed it
// and the call reduces batch statistics (a training forward, its loss, a backward), else null.  Eval forwards use the
// running statistics: nothing to exchange.
inline const SyncDesc* active_sync(const fu_ctx* c, bool training) { return (training && c->sync.hook) ? &c->sync : nullptr; }
// fp16 mode: where the backward writes parameter gradients it passes this pointer to 1 / loss scale (null otherwise: 1)
inline const float* grad_unscale(const fu_ctx* c) { return c->prec == PREC_F16 ? c->loss_scale + 1 : nullptr; }

// fu_plan.hip
int build_plan(fu_ctx* c);
int alloc_workspace(fu_ctx* c);
// the device tables of one bilinear x2 resize; every allocation is appended to *allocs (the caller frees them)
int build_up_tables(std::vector<void*>* allocs, int H, int W, UpTables* t);
int repack(fu_ctx* c, hipStream_t s, bool eval);
// The events of the context hand work from one stream to another on ONE device (ev_gy, ev_blk, the fence pair): their records
// need no system-scope release, which is there for the host and for other devices (hip_runtime_api.h).  The data-parallel
// events of fu_dp.hip order work against RCCL and the host and keep it.  The waiter of fu_backward_fence may be the stream
// that RCCL's all-reduce is launched from: that holds while the collective's kernel on THIS device reads the gradients
// itself (through the local L2) and sends them on; a transport in which a peer reads the user buffer directly would need
// the fence back on ev_fence.  Only single-GPU runs have measured and checked this flag.
constexpr unsigned EVENT_FLAGS = hipEventDisableTiming | hipEventDisableSystemFence;

// fu_step.hip
int forward_impl(fu_ctx* c, const float* x, const SrcList* srcs, int B, bool training, float* logits_out,
                 hipStream_t s, int n_views = 0, unsigned view_codes = 0);
int perturb_bnb(float* part, int tiles, int C, hipStream_t s);
// s waits for everything queued on the side stream (the weight-gradient chains); no-op without one
int join_side(fu_ctx* c, hipStream_t s);
int num_backward_blocks(const fu_ctx* c);
int backward_block_index(const fu_ctx* c, int block);
int backward_block_impl(fu_ctx* c, int block, const float* dlogits_ext, hipStream_t s, bool join);
double conv_flops(fu_ctx* c, bool train);

}  // namespace fu
