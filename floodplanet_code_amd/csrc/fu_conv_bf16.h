// Private declarations shared by the five 16-bit convolution translation units: fu_conv_bf16.hip (weight pack, general
// forward / dgrad kernel, the forward route conv3x3_route), fu_conv_bf16_fast.hip, fu_conv_rs.hip, fu_conv_pp.hip (the
// aligned-shape kernels) and fu_wgrad_bf16.hip (the weight gradient, conv3x3_wgrad_route and conv3x3_wgrad_plan).
//
// ONE source, TWO element types.  The Makefile compiles every one of them twice: as they stand (bf16: v_mfma_f32_32x32x16_bf16) and
// with -DFU_HALF=1 (IEEE fp16: v_mfma_f32_32x32x16_f16, the same MFMA rate).  Tiles, LDS images, schedules, address math
// and the transposing reads are identical -- a 16-bit element is a 16-bit element -- so the only things that change are
// the four conversions (f2e / e2f_lo / e2f_hi / pack_e2), the fragment vector type and the MFMA / ds_read_tr builtins,
// all defined below.  Device buffers stay raw 16-bit storage (`bf16_t` = unsigned short in both builds); the fp16 build's
// entry points and kernels carry `f16` in their names (the #defines below); the testing hooks (ConvHooks) are defined once,
// in fu_conv.hip.
#pragma once
#include "fu_common.h"

#ifndef FU_HALF
#define FU_HALF 0
#endif
#if FU_HALF
// names of the fp16 build (the bf16 build keeps the names as written in the sources)
#define launch_pack_conv3x3_bf16 launch_pack_conv3x3_f16
#define launch_conv3x3_bf16 launch_conv3x3_f16
#define launch_conv3x3_wgrad_bf16 launch_conv3x3_wgrad_f16
#define launch_conv3x3_bf16_fast launch_conv3x3_f16_fast
#define conv3x3_bf16_fast_eligible conv3x3_f16_fast_eligible
#define conv3x3_num_stat_tiles_bf16 conv3x3_num_stat_tiles_f16
#define conv3x3_wgrad_slab_elems_bf16 conv3x3_wgrad_slab_elems_f16
#define k_pack_bf16 k_pack_f16
#define k_conv3x3_bf16 k_conv3x3_f16
#define k_conv3x3_bf16_fast k_conv3x3_f16_fast
#define k_wgrad_bf16 k_wgrad_f16
#define k_wgrad_bf16_pp k_wgrad_f16_pp
#define k_wgrad_bf16_c8 k_wgrad_f16_c8
#define conv3x3_rs_eligible conv3x3_rs_eligible_f16
#define launch_conv3x3_rs launch_conv3x3_rs_f16
#define conv3x3_c8_eligible conv3x3_c8_eligible_f16
#define launch_conv3x3_c8 launch_conv3x3_c8_f16
#define conv3x3_pp_eligible conv3x3_pp_eligible_f16
#define launch_conv3x3_pp launch_conv3x3_pp_f16
#define conv3x3_route conv3x3_route_f16
#define conv3x3_wgrad_route conv3x3_wgrad_route_f16
#define conv3x3_wgrad_plan conv3x3_wgrad_plan_f16
#endif

#include <type_traits>

namespace fu {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
#if FU_HALF
typedef _Float16 frag8_t __attribute__((ext_vector_type(8)));     // one MFMA operand fragment: 8 consecutive k per lane
typedef __fp16 tr4_t __attribute__((ext_vector_type(4)));         // (the element type the ds_read_tr16 builtin is declared with)
#define FU_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#define FU_TR16(p) __builtin_amdgcn_ds_read_tr16_b64_v4f16(p)
#else
typedef __bf16 frag8_t __attribute__((ext_vector_type(8)));
typedef __bf16 tr4_t __attribute__((ext_vector_type(4)));
#define FU_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#define FU_TR16(p) __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p)
#endif

// compile-time loop: every array index below is a constant expression, so the staging registers are never
// demoted to scratch (runtime-indexed private arrays are -- cdna guide rule 20)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

#ifdef __HIPCC__
// ---- the element conversions (the only arithmetic that depends on the 16-bit format) ----
#if FU_HALF
typedef _Float16 e16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2e(float f) { return f2h(f); }                                   // RNE
__device__ __forceinline__ float e2f_lo(unsigned v) { return h2f((unsigned short)(v & 0xffffu)); }  // v_cvt_f32_f16
__device__ __forceinline__ float e2f_hi(unsigned v) { return h2f((unsigned short)(v >> 16)); }      // v_cvt_f32_f16 sdwa WORD_1
#else
typedef __bf16 e16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2e(float f) { return f2bf(f); }
__device__ __forceinline__ float e2f_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float e2f_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
#endif
__device__ __forceinline__ unsigned pack_e2(f32x2 v) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, e16x2));    // v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 (RNE)
}

// relu(a * x + b) on the two 16-bit channels of one dword; one rounding to the element type.  Plain v_fma_f32 /
// v_max_f32 per channel: the packed-f32 form (v_pk_fma_f32, ReLU as v_pk_max_i16) is three instructions shorter per pair
// and was round 1's choice, but packed f32 VALU is slow beside a co-resident wave's MFMAs (MI355X_MICROARCH.md, "price
// of one filler": +22 cycles per v_pk_fma_f32): s_memtime stamps of the row-stationary kernel's staging phase, 10 units
// per thread and chunk: 6000 cycles packed, 3300 plain
__device__ __forceinline__ unsigned bn_relu_pair(unsigned v, f32x2 a, f32x2 b) {
  const float lo = fmaxf(fmaf(a.x, e2f_lo(v), b.x), 0.f), hi = fmaxf(fmaf(a.y, e2f_hi(v), b.y), 0.f);
  return pack_e2(f32x2{lo, hi});
}

// relu(a * x + b) on the eight channels of one 16-byte unit (the staging of the general kernel and of the weight gradient)
__device__ __forceinline__ uint4 bn_relu_pack8(uint4 v, const float4& a0, const float4& a1, const float4& b0,
                                               const float4& b1) {
  float x[8];
  x[0] = e2f_lo(v.x); x[1] = e2f_hi(v.x);
  x[2] = e2f_lo(v.y); x[3] = e2f_hi(v.y);
  x[4] = e2f_lo(v.z); x[5] = e2f_hi(v.z);
  x[6] = e2f_lo(v.w); x[7] = e2f_hi(v.w);
  x[0] = bn_act_fused(a0.x, x[0], b0.x); x[1] = bn_act_fused(a0.y, x[1], b0.y);
  x[2] = bn_act_fused(a0.z, x[2], b0.z); x[3] = bn_act_fused(a0.w, x[3], b0.w);
  x[4] = bn_act_fused(a1.x, x[4], b1.x); x[5] = bn_act_fused(a1.y, x[5], b1.y);
  x[6] = bn_act_fused(a1.z, x[6], b1.z); x[7] = bn_act_fused(a1.w, x[7], b1.w);
  uint4 o;
  o.x = (unsigned)f2e(x[0]) | ((unsigned)f2e(x[1]) << 16);
  o.y = (unsigned)f2e(x[2]) | ((unsigned)f2e(x[3]) << 16);
  o.z = (unsigned)f2e(x[4]) | ((unsigned)f2e(x[5]) << 16);
  o.w = (unsigned)f2e(x[6]) | ((unsigned)f2e(x[7]) << 16);
  return o;
}

// Workgroup barrier behind this wave's LDS traffic only (lgkmcnt), then s_barrier.  __syncthreads() also waits with vmcnt(0),
// i.e. for global loads that were issued to stay in flight across the barrier.
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

#endif

// forward / dgrad launch parameters (see launch_conv3x3_bf16)
struct BConvP {
  const bf16_t* src0; const bf16_t* src1; const float* a0; const float* b0;
  const bf16_t* wpk;   // [9][N][Cin]
  const float* bias;
  bf16_t* dst0; bf16_t* dst1; float* stats;
  int C0, C1, Cin, N, D0, D1, B, H, W, tilesX, tilesY, nPix, nCo;
  unsigned rcp_nPix, rcp_tilesX, rcp_tilesY;   // fast path: floor(2^32 / d) + 1 (0 for d == 1)
  unsigned rcp_nCo;                            // row-stationary kernel: channel tile fastest in the workgroup order
  int center_only;           // 1: every tap but the centre one of wpk is zero (embedded 1x1): the fast kernel skips them
  // row-stationary kernel, dgrad into a BatchNorm's output gradient (BnbFuse, fu_common.h): the raw conv output y of that
  // BatchNorm, its a / b / mean / invstd, and the per-tile sums [nPix][N][2]; all null otherwise
  const bf16_t* bnb_y; const float* bnb_a; const float* bnb_b; const float* bnb_mean; const float* bnb_invstd; float* bnb_part;
  int nTiles;                // persistent ping-pong kernel (fu_conv_pp.hip): nPix * nCo, walked by gridDim.x workgroups
};

// weight-gradient launch parameters (see launch_conv3x3_wgrad_bf16)
struct BWgP {
  const bf16_t* src0; const bf16_t* src1; const float* a0; const float* b0; const bf16_t* dy;
  float* slab;
  int C0, C1, Cin, Cout, B, H, W, tilesX, tilesY, nPix, nCi, nCo, S, perSplit;
  unsigned rcp_tilesX, rcp_tilesY;   // k_wgrad_bf16_pp<true>: floor(2^32 / d) + 1 (0 for d == 1), as in BConvP
};

// the pixel-tile / channel-tile counts of a launch and their reciprocals, for a kernel with tw x th-pixel, bn-channel tiles
// (the aligned-shape kernels get exact quotients)
static inline void conv_geometry(BConvP& P, int tw, int th, int bn) {
  P.tilesX = ceil_div(P.W, tw); P.tilesY = ceil_div(P.H, th);
  P.nPix = P.B * P.tilesX * P.tilesY; P.nCo = ceil_div(P.N, bn); P.nTiles = P.nPix * P.nCo;
  P.rcp_nPix = host_rcp(P.nPix); P.rcp_tilesX = host_rcp(P.tilesX); P.rcp_tilesY = host_rcp(P.tilesY);
  P.rcp_nCo = host_rcp(P.nCo);
}
// ... of a weight-gradient launch (c_out tiles of 64), and its split-K plan: about target_wgs workgroups, every split owns
// at least one pixel tile
static inline void wgrad_geometry(BWgP& P, int tw, int th, int ci_t, int target_wgs) {
  P.tilesX = ceil_div(P.W, tw); P.tilesY = ceil_div(P.H, th);
  P.nPix = P.B * P.tilesX * P.tilesY;
  P.nCi = ceil_div(P.Cin, ci_t); P.nCo = ceil_div(P.Cout, 64);
  P.rcp_tilesX = host_rcp(P.tilesX); P.rcp_tilesY = host_rcp(P.tilesY);
  int S = ceil_div(target_wgs, P.nCi * P.nCo);
  if (S > P.nPix) S = P.nPix;
  if (S < 1) S = 1;
  P.perSplit = ceil_div(P.nPix, S);
  P.S = ceil_div(P.nPix, P.perSplit);
}

// BatchNorm-backward sums of the destination (BnbFuse, fu_common.h): the launch is asked for them and is of the kind that
// can give them (a dgrad into one destination, no BatchNorm prologue) ...
static inline bool wants_bnb(const BConvP& P, const LaunchOpts& o) {
  return o.bnb != nullptr && o.bnb->y != nullptr && P.a0 == nullptr && P.dst1 == nullptr && P.stats == nullptr;
}
// ... and the rs / pp launcher's answer: with room for `tiles` rows of sums the kernel gets the pointers and the caller the count
static inline bool attach_bnb(BConvP& P, const LaunchOpts& o, int64_t tiles) {
  if (!wants_bnb(P, o) || o.bnb->tiles_out == nullptr || tiles * P.N * 2 > o.bnb->max_elems) return false;
  const BnbFuse& f = *o.bnb;
  P.bnb_y = (const bf16_t*)f.y; P.bnb_a = f.a; P.bnb_b = f.b; P.bnb_mean = f.mean; P.bnb_invstd = f.invstd;
  P.bnb_part = f.part;
  *f.tiles_out = (int)tiles;
  return true;
}

// The testing hooks (include/floodunet.h, fu_test_*): one process-wide record, defined with its setters in fu_conv.hip.
struct ConvHooks {
  int force_general;    // fu_test_force_general_conv: skip the aligned-shape kernels
  int full_taps;        // fu_test_force_full_taps: embedded 1x1 convs run all nine taps
  int tile_mode;        // fu_test_conv_tile_mode: 0 = heuristic, 1 = square fast tiles only, 2 = tall fast tile, 3 = rs, 4 = pp
  int wgrad_lockstep;   // fu_test_force_lockstep_wgrad: 1 = k_wgrad_bf16<4,8> for the ping-pong kernel, 2 = its general staging
  int op_center_only;   // fu_test_op_center_only: the fu_op_conv3x3_* hooks mark their ConvIn as an embedded 1x1
};
extern ConvHooks g_conv_hooks;

// Which kernel instantiation a forward / dgrad launch runs (conv3x3_route, fu_conv_bf16.hip: every preference and its
// measurement) and which a weight gradient (conv3x3_wgrad_route, fu_wgrad_bf16.hip).  Pure host functions of the shapes and of which pointers
// are null; fu_test_conv_route (fu_conv.hip) answers from them without a GPU.
enum ConvRoute {
  CONV_GENERAL_64, CONV_GENERAL_32, CONV_TAP1_64, CONV_TAP1_32, CONV_C8, CONV_PP, CONV_RS8, CONV_RS4, CONV_FAST_TALL,
  CONV_FAST_64, CONV_FAST_32, CONV_NUM_ROUTES
};
enum WgradRoute { WGRAD_TAP1_WIDE, WGRAD_TAP1_NARROW, WGRAD_C8, WGRAD_PP, WGRAD_LOCKSTEP_128, WGRAD_LOCKSTEP_64, WGRAD_NUM_ROUTES };
ConvRoute conv3x3_route(const BConvP& P, const LaunchOpts& o, const ConvHooks& h);
WgradRoute conv3x3_wgrad_route(const BWgP& P, bool one_tap, const ConvHooks& h);
void conv3x3_wgrad_plan(BWgP& P, WgradRoute r);   // the route's tile counts and split-K plan (P.S slabs)

// what each kernel can run (beside the kernels)
bool conv3x3_bf16_fast_eligible(const BConvP& P);   // aligned-shape fast path (fu_conv_bf16_fast.hip)
bool conv3x3_c8_eligible(const BConvP& P);          // 8-input-channel forward kernel (fu_conv_rs.hip): the network's first conv
bool conv3x3_rs_eligible(const BConvP& P);          // row-stationary 16x16x32 kernel (fu_conv_rs.hip)
bool conv3x3_pp_eligible(const BConvP& P);          // persistent ping-pong row-stationary kernel (fu_conv_pp.hip)
// ... and their launchers
int launch_conv3x3_bf16_fast(BConvP& P, ConvRoute r, const LaunchOpts& o, hipStream_t s);   // the one-tap and fast routes
int launch_conv3x3_c8(BConvP& P, const LaunchOpts& o, hipStream_t s);
int launch_conv3x3_rs(BConvP& P, bool rows8, const LaunchOpts& o, hipStream_t s);
int launch_conv3x3_pp(BConvP& P, const LaunchOpts& o, hipStream_t s);

}  // namespace fu
