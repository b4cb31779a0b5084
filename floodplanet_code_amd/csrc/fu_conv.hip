// What the 3x3 convolutions of all three precisions share (compiled once): the dispatch on the context's precision
// to fu_conv_f32.hip / fu_conv_bf16.hip + fu_wgrad_bf16.hip (the latter two compiled a second time for fp16), and the tail of every
// weight-gradient launch, which sums the split-K slabs in a fixed order into fp32 OIHW and the bias gradient.
#include "fu_common.h"
#include "fu_conv_bf16.h"
#include "floodunet.h"

namespace fu {

// ---- the 16-bit convs' testing hooks (include/floodunet.h) and the query for what they and the shapes decide -----------
ConvHooks g_conv_hooks = {0, 0, 0, 0, 0};
bool test_op_center_only() { return g_conv_hooks.op_center_only != 0; }

// the parameter blocks as launch_conv3x3_bf16 / launch_conv3x3_wgrad_bf16 fill them, with stand-in non-null pointers: a
// forward launch carries bias and statistics, a dgrad launch neither, and the fused-sums request when want_bnsums
static int query_route(int kind, int C0, int has_bn0, int C1, int D0, int D1, int center_only, int want_bnsums, int B, int H,
                       int W, int64_t* slab_elems) {
  static const float fake[2] = {0.f, 0.f};
  const bf16_t* const act = reinterpret_cast<const bf16_t*>(fake);
  const bool one_tap = center_only && !g_conv_hooks.full_taps;
  if (kind == 2) {
    BWgP P = {};
    P.src0 = act; P.src1 = C1 > 0 ? act : nullptr; P.a0 = has_bn0 ? fake : nullptr; P.b0 = P.a0;
    P.C0 = C0; P.C1 = C1 > 0 ? C1 : 0; P.Cin = P.C0 + P.C1; P.Cout = D0; P.B = B; P.H = H; P.W = W;
    const WgradRoute r = conv3x3_wgrad_route(P, one_tap, g_conv_hooks);
    conv3x3_wgrad_plan(P, r);
    if (slab_elems) *slab_elems = (int64_t)P.S * 9 * P.Cin * P.Cout;
    return r;
  }
  BConvP P = {};
  P.src0 = act; P.src1 = C1 > 0 ? act : nullptr; P.a0 = has_bn0 ? fake : nullptr; P.b0 = P.a0;
  P.dst0 = const_cast<bf16_t*>(act); P.dst1 = D1 > 0 ? P.dst0 : nullptr;
  if (kind == 0) { P.bias = fake; P.stats = const_cast<float*>(fake); }
  P.C0 = C0; P.C1 = C1 > 0 ? C1 : 0; P.Cin = P.C0 + P.C1; P.N = D0 + D1; P.D0 = D0; P.D1 = D1; P.B = B; P.H = H; P.W = W;
  P.center_only = one_tap ? 1 : 0;
  BnbFuse f;
  f.y = fake;
  LaunchOpts o;
  if (want_bnsums) o.bnb = &f;
  return conv3x3_route(P, o, g_conv_hooks);
}

// ---- precision dispatch -------------------------------------------------------------------------
int conv3x3_num_stat_tiles(Prec p, int B, int H, int W) {
  return p == PREC_F32 ? conv3x3_num_stat_tiles_f32(B, H, W)
                       : (p == PREC_BF16 ? conv3x3_num_stat_tiles_bf16(B, H, W) : conv3x3_num_stat_tiles_f16(B, H, W));
}
int launch_conv3x3(Prec p, const ConvIn& in, const void* wpk, const float* bias, void* dst0, int D0, void* dst1,
                   int D1, float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s) {
  if (p == PREC_F32)
    return launch_conv3x3_f32(in, (const float*)wpk, bias, (float*)dst0, D0, (float*)dst1, D1, stats, n_stat_tiles, B,
                              H, W, s);
  if (p == PREC_BF16)
    return launch_conv3x3_bf16(in, (const bf16_t*)wpk, bias, (bf16_t*)dst0, D0, (bf16_t*)dst1, D1, stats, n_stat_tiles,
                               B, H, W, s);
  return launch_conv3x3_f16(in, (const bf16_t*)wpk, bias, (bf16_t*)dst0, D0, (bf16_t*)dst1, D1, stats, n_stat_tiles, B,
                            H, W, s);
}
int64_t conv3x3_wgrad_slab_elems(Prec p, int Cin, int Cout, int B, int H, int W) {
  return p == PREC_F32 ? conv3x3_wgrad_slab_elems_f32(Cin, Cout, B, H, W)
                       : (p == PREC_BF16 ? conv3x3_wgrad_slab_elems_bf16(Cin, Cout, B, H, W)
                                         : conv3x3_wgrad_slab_elems_f16(Cin, Cout, B, H, W));
}
int launch_conv3x3_wgrad(Prec p, const ConvIn& in, const void* dy, int Cout, float* slab, float* dw_oihw,
                         int cin_real, const float* db_partials, int n_db_partials, float* db, int B, int H, int W,
                         hipStream_t s) {
  if (p == PREC_F32)
    return launch_conv3x3_wgrad_f32(in, (const float*)dy, Cout, slab, dw_oihw, cin_real, db_partials, n_db_partials,
                                    db, B, H, W, s);
  if (p == PREC_BF16)
    return launch_conv3x3_wgrad_bf16(in, (const bf16_t*)dy, Cout, slab, dw_oihw, cin_real, db_partials, n_db_partials,
                                     db, B, H, W, s);
  return launch_conv3x3_wgrad_f16(in, (const bf16_t*)dy, Cout, slab, dw_oihw, cin_real, db_partials, n_db_partials, db,
                                  B, H, W, s);
}
int64_t conv3x3_pack_elems(Prec p, int cin_pad, int Cout) {
  (void)p;
  return (int64_t)9 * cin_pad * Cout;
}
int launch_pack_conv3x3(Prec p, const float* w_oihw, int Cout, int cin_real, int cin_pad, void* wfwd, void* wdgrad,
                        hipStream_t s) {
  if (p == PREC_F32) return launch_pack_conv3x3_f32(w_oihw, Cout, cin_real, cin_pad, (float*)wfwd, (float*)wdgrad, s);
  if (p == PREC_BF16) return launch_pack_conv3x3_bf16(w_oihw, Cout, cin_real, cin_pad, (bf16_t*)wfwd, (bf16_t*)wdgrad, s);
  return launch_pack_conv3x3_f16(w_oihw, Cout, cin_real, cin_pad, (bf16_t*)wfwd, (bf16_t*)wdgrad, s);
}

// ------------------------------------------------------------------------------------------------
// split-K slabs -> dw (OIHW) and db.  Per output element, on every path below, the summation tree is the same:
// split lane sl = s mod SL accumulates four interleaved fp32 partials (s, s + SL, s + 2 SL, s + 3 SL per round, then single
// steps), combines them as (a0 + a1) + (a2 + a3); the SL lane sums are added in lane order in fp64 and rounded to fp32; the
// fp16 unscale factor (a power of two) is applied on the way into dw.  Only which thread owns which element differs.
// ------------------------------------------------------------------------------------------------

// one split lane's sum of the float4 at p over slabs sl, sl + SL, ...: four independent loads in flight
template <int SL>
__device__ __forceinline__ float4 wgrad_lane_sum(const float* __restrict__ p, int64_t nSlab, int S, int sl) {
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  int s = sl;
  for (; s + 3 * SL < S; s += 4 * SL) {
    const float4 v0 = *reinterpret_cast<const float4*>(p + (int64_t)s * nSlab);
    const float4 v1 = *reinterpret_cast<const float4*>(p + (int64_t)(s + SL) * nSlab);
    const float4 v2 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 2 * SL) * nSlab);
    const float4 v3 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 3 * SL) * nSlab);
    a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
    a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
    a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
  }
  for (; s < S; s += SL) {
    const float4 v0 = *reinterpret_cast<const float4*>(p + (int64_t)s * nSlab);
    a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
  }
  return make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y), (a0.z + a1.z) + (a2.z + a3.z),
                     (a0.w + a1.w) + (a2.w + a3.w));
}

// the SL lane sums of one element, parked in LDS rows of `stride` floats, added in lane order
template <int SL>
__device__ __forceinline__ float wgrad_lanes_total(const float* sm, int stride, int e) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SL; ++k) acc += (double)sm[k * stride + e];
  return (float)acc;
}

// bias gradient (the tail blocks of the reduce launches): db[co] = sum_i dbp[i][co] for the 16 channels of block bblk.
// 256 threads = 16 channels x 16 partial lanes, 8 independent loads in flight per lane
// (one thread walking all ~2000 partials is a 100+ us latency chain that would set this kernel's duration)
__device__ __forceinline__ void wgrad_bias_block(int64_t bblk, int Cout, const float* __restrict__ dbp, int ndb,
                                                 float* __restrict__ db, const float* __restrict__ unscale) {
  __shared__ double smd[16][16];
  const bool act = threadIdx.x < 256;
  const int c16 = threadIdx.x & 15, pl = (threadIdx.x >> 4) & 15;
  const int co = (int)(bblk * 16 + c16);
  double acc = 0.0;
  if (act && co < Cout) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int i = pl;
    for (; i + 7 * 16 < ndb; i += 8 * 16) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += dbp[(int64_t)(i + u * 16) * Cout + co];
    }
    for (; i < ndb; i += 16) a[0] += dbp[(int64_t)i * Cout + co];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (double)a[u];
  }
  if (act) smd[pl][c16] = acc;
  __syncthreads();
  if (act && pl == 0 && co < Cout) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += smd[k][c16];
    if (unscale) t *= (double)*unscale;       // fp16 mode: dy carried the loss scale
    db[co] = (float)t;
  }
}

// fp32 path, first of two kernels: slab 0 = sum_s slab[s] ([tap][ci][co], in place);  db[co] = sum_i dbp[i][co]
// Bandwidth kernel: 256 threads = SL split lanes x (256/SL) float4 columns; a block owns 4*256/SL consecutive slab
// elements (co fastest -> coalesced rows); lanes meet in LDS in a fixed order (deterministic).
template <int SL>
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ slab, int S, int Cin, int Cout,
                                                      const float* __restrict__ dbp, int ndb, float* __restrict__ db,
                                                      const float* __restrict__ unscale) {
  constexpr int COLS = 256 / SL, ELEMS = 4 * COLS;
  __shared__ float sm[SL][ELEMS];
  const int64_t nSlab = (int64_t)9 * Cin * Cout;          // elements of one slab ([tap][ci][co], Cout % 4 == 0)
  const int64_t nBlocksW = (nSlab + ELEMS - 1) / ELEMS;
  const int col = threadIdx.x % COLS, sl = threadIdx.x / COLS;
  if ((int64_t)blockIdx.x < nBlocksW) {
    const int64_t e0 = (int64_t)blockIdx.x * ELEMS + col * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e0 < nSlab) a = wgrad_lane_sum<SL>(slab + e0, nSlab, S, sl);
    *reinterpret_cast<float4*>(&sm[sl][col * 4]) = a;
    __syncthreads();
    // the block's summed elements go back IN PLACE into slab 0 (only this block ever touches them), coalesced;
    // k_wgrad_transpose then turns [tap][ci][co] into OIHW with full-line writes
    if (threadIdx.x < COLS && e0 < nSlab) {
      float4 o;
      o.x = wgrad_lanes_total<SL>(&sm[0][0], ELEMS, col * 4 + 0);
      o.y = wgrad_lanes_total<SL>(&sm[0][0], ELEMS, col * 4 + 1);
      o.z = wgrad_lanes_total<SL>(&sm[0][0], ELEMS, col * 4 + 2);
      o.w = wgrad_lanes_total<SL>(&sm[0][0], ELEMS, col * 4 + 3);
      *reinterpret_cast<float4*>(const_cast<float*>(slab) + e0) = o;
    }
  } else if (db) {
    wgrad_bias_block((int64_t)blockIdx.x - nBlocksW, Cout, dbp, ndb, db, unscale);
  }
}

// fp32 path, second kernel: packed [tap][Cin][Cout] (slab 0 after the reduce) -> dw OIHW [Cout][cin_real][9].
// block tile: 32 co x 8 ci x 9 taps through LDS: 128-byte reads along co, 288-byte writes along (ci, tap).
__global__ __launch_bounds__(256) void k_wgrad_transpose(const float* __restrict__ packed, int Cin, int Cout,
                                                         int cin_real, float* __restrict__ dw,
                                                         const float* __restrict__ unscale) {
  __shared__ float t[72][33];
  const float us = unscale ? *unscale : 1.f;      // fp16 mode: 1 / loss scale (a power of two: exact)
  const int nCo = (Cout + 31) / 32;
  const int co0 = (blockIdx.x % nCo) * 32, ci0 = (blockIdx.x / nCo) * 8;
  for (int i = threadIdx.x; i < 72 * 32; i += 256) {
    const int row = i >> 5, c = i & 31;          // row = tap*8 + ci_local
    const int tap = row >> 3, ci = ci0 + (row & 7), co = co0 + c;
    t[row][c] = (ci < Cin && co < Cout) ? packed[((int64_t)tap * Cin + ci) * Cout + co] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * 72; i += 256) {
    const int c = i / 72, j = i - c * 72;        // j = ci_local*9 + tap  (OIHW order inside the tile)
    const int cil = j / 9, tap = j - cil * 9;
    const int ci = ci0 + cil, co = co0 + c;
    if (ci < cin_real && co < Cout) dw[((int64_t)co * cin_real + ci) * 9 + tap] = t[tap * 8 + cil][c] * us;
  }
}

// 16-bit paths, one kernel: dw[co][ci][tap] = sum_s slab[s][tap][ci / 4][co][ci % 4];  db[co] = sum_i dbp[i][co]
// The 16-bit weight-gradient kernels write their slabs as [tap][Cin / 4][Cout][4] -- a lane of the 32x32 accumulator tile
// holds four consecutive c_in of one c_out, so each lane stores 16 bytes and a wave 512 contiguous bytes.  The slabs are
// read once, in that order, and the sums go straight to OIHW: the output is 1 / S of the traffic, so its order is chosen
// per regime for the reads' sake.
//   SL > 1 (S >= 16, slabs of at most 64 K float4): the block shape of k_wgrad_reduce (SL split lanes x 256 / SL float4
//     columns of consecutive slab elements, as many blocks as before); 1024 / SL threads add the lanes of one element each
//     and store it with a 4-byte store (the four c_in of a column are 36 bytes apart in OIHW).
//   SL == 1 (S < 16, the wide layers, up to 1.2 M float4 per slab): a block owns 32 c_out x 4 c_in x 9 taps = 288 float4
//     columns (nine 512-byte runs per slab), one per thread of its 320, turns them in LDS and writes 32 runs of 144
//     bytes, as k_wgrad_transpose does.
template <int SL>
__global__ __launch_bounds__(SL == 1 ? 320 : 256) void k_wgrad_reduce_oihw(
    const float* __restrict__ slab, int S, int Cin, int Cout, int cin_real, float* __restrict__ dw,
    const float* __restrict__ dbp, int ndb, float* __restrict__ db, const float* __restrict__ unscale) {
  const int64_t nSlab = (int64_t)9 * Cin * Cout;
  const int cq = Cin >> 2;
  if constexpr (SL == 1) {
    __shared__ float t[32][37];
    const int nCo = (Cout + 31) / 32;
    const int64_t nBlocksW = (int64_t)nCo * cq;
    if ((int64_t)blockIdx.x < nBlocksW) {
      const float us = unscale ? *unscale : 1.f;
      const int co0 = (int)(blockIdx.x % nCo) * 32, q = (int)(blockIdx.x / nCo);
      const int c = threadIdx.x & 31, tap = threadIdx.x >> 5;
      if (tap < 9) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (co0 + c < Cout) a = wgrad_lane_sum<1>(slab + (((int64_t)tap * cq + q) * Cout + co0 + c) * 4, nSlab, S, 0);
        const float* ap = &a.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[c][k * 9 + tap] = wgrad_lanes_total<1>(ap, 0, k);
      }
      __syncthreads();
      for (int i = threadIdx.x; i < 32 * 36; i += 320) {
        const int cl = i / 36, j = i - cl * 36;      // j = ci_local * 9 + tap  (OIHW order inside the tile)
        const int ci = 4 * q + j / 9, co = co0 + cl;
        if (ci < cin_real && co < Cout) dw[((int64_t)co * cin_real + 4 * q) * 9 + j] = t[cl][j] * us;
      }
    } else if (db) {
      wgrad_bias_block((int64_t)blockIdx.x - nBlocksW, Cout, dbp, ndb, db, unscale);
    }
  } else {
    constexpr int COLS = 256 / SL, ELEMS = 4 * COLS;
    __shared__ float sm[SL][ELEMS];
    const int64_t nBlocksW = (nSlab + ELEMS - 1) / ELEMS;
    const int col = threadIdx.x % COLS, sl = threadIdx.x / COLS;
    if ((int64_t)blockIdx.x < nBlocksW) {
      const int64_t e0 = (int64_t)blockIdx.x * ELEMS + col * 4;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e0 < nSlab) a = wgrad_lane_sum<SL>(slab + e0, nSlab, S, sl);
      *reinterpret_cast<float4*>(&sm[sl][col * 4]) = a;
      __syncthreads();
      // one element per thread: its SL lane sums, then its place in OIHW (element = ((tap * cq + ci / 4) * Cout + co) * 4 + ci % 4)
      const unsigned e = (unsigned)blockIdx.x * ELEMS + threadIdx.x;
      if (threadIdx.x < ELEMS && e < (unsigned)nSlab) {
        const float us = unscale ? *unscale : 1.f;
        const unsigned f = e >> 2, r = f / (unsigned)Cout, co = f - r * (unsigned)Cout;
        const unsigned tap = r / (unsigned)cq, ci = 4 * (r - tap * (unsigned)cq) + (e & 3);
        if (ci < (unsigned)cin_real)
          dw[((int64_t)co * cin_real + ci) * 9 + tap] = wgrad_lanes_total<SL>(&sm[0][0], ELEMS, threadIdx.x) * us;
      }
    } else if (db) {
      wgrad_bias_block((int64_t)blockIdx.x - nBlocksW, Cout, dbp, ndb, db, unscale);
    }
  }
}

template <int SL>
static int launch_wgrad_reduce_sl(const float* slab, int S, int Cin, int Cout, const float* dbp, int ndb, float* db,
                                  const float* unscale, hipStream_t s) {
  constexpr int ELEMS = 4 * (256 / SL);
  const int64_t nSlab = (int64_t)9 * Cin * Cout;
  const int64_t blocks = (nSlab + ELEMS - 1) / ELEMS + (db ? (Cout + 15) / 16 : 0);
  hipLaunchKernelGGL(k_wgrad_reduce<SL>, dim3((unsigned)blocks), dim3(256), 0, s, slab, S, Cin, Cout, dbp, ndb, db,
                     unscale);
  FU_LAUNCH_CHECK();
  return 0;
}

// fp32 path: [tap][ci][co] slabs
int launch_wgrad_reduce(const float* slab, int S, int Cin, int Cout, int cin_real, float* dw, const float* dbp,
                        int ndb, float* db, const float* unscale, hipStream_t s) {
  int st;
  if (S >= 64) st = launch_wgrad_reduce_sl<16>(slab, S, Cin, Cout, dbp, ndb, db, unscale, s);
  else if (S >= 16) st = launch_wgrad_reduce_sl<4>(slab, S, Cin, Cout, dbp, ndb, db, unscale, s);
  else st = launch_wgrad_reduce_sl<1>(slab, S, Cin, Cout, dbp, ndb, db, unscale, s);
  if (st) return st;
  const int blocks = ceil_div(Cout, 32) * ceil_div(Cin, 8);
  hipLaunchKernelGGL(k_wgrad_transpose, dim3(blocks), dim3(256), 0, s, slab, Cin, Cout, cin_real, dw, unscale);
  FU_LAUNCH_CHECK();
  return 0;
}

template <int SL>
static int launch_wgrad_reduce_oihw_sl(const float* slab, int S, int Cin, int Cout, int cin_real, float* dw,
                                       const float* dbp, int ndb, float* db, const float* unscale, hipStream_t s) {
  constexpr int ELEMS = 4 * (256 / SL);
  const int64_t nSlab = (int64_t)9 * Cin * Cout;
  const int64_t blocksW = SL == 1 ? (int64_t)ceil_div(Cout, 32) * (Cin >> 2) : (nSlab + ELEMS - 1) / ELEMS;
  const int64_t blocks = blocksW + (db ? (Cout + 15) / 16 : 0);
  hipLaunchKernelGGL(k_wgrad_reduce_oihw<SL>, dim3((unsigned)blocks), dim3(SL == 1 ? 320 : 256), 0, s, slab, S, Cin,
                     Cout, cin_real, dw, dbp, ndb, db, unscale);
  FU_LAUNCH_CHECK();
  return 0;
}

// 16-bit paths: [tap][ci / 4][co][4] slabs; the same SL for the same S as the fp32 path
int launch_wgrad_reduce_oihw(const float* slab, int S, int Cin, int Cout, int cin_real, float* dw, const float* dbp,
                             int ndb, float* db, const float* unscale, hipStream_t s) {
  FU_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0, "wgrad_reduce_oihw: the interleaved slab layout needs c_in %% 4 == 0 and c_out %% 4 == 0");
  FU_REQUIRE((int64_t)9 * Cin * Cout < (int64_t(1) << 31), "wgrad_reduce_oihw: slab elements are indexed in 32 bits");
  if (S >= 64) return launch_wgrad_reduce_oihw_sl<16>(slab, S, Cin, Cout, cin_real, dw, dbp, ndb, db, unscale, s);
  if (S >= 16) return launch_wgrad_reduce_oihw_sl<4>(slab, S, Cin, Cout, cin_real, dw, dbp, ndb, db, unscale, s);
  return launch_wgrad_reduce_oihw_sl<1>(slab, S, Cin, Cout, cin_real, dw, dbp, ndb, db, unscale, s);
}

}  // namespace fu

extern "C" {
void fu_test_force_general_conv(int on) { fu::g_conv_hooks.force_general = on; }
void fu_test_force_lockstep_wgrad(int on) { fu::g_conv_hooks.wgrad_lockstep = on; }
void fu_test_force_full_taps(int on) { fu::g_conv_hooks.full_taps = on; }
void fu_test_conv_tile_mode(int mode) { fu::g_conv_hooks.tile_mode = mode; }
void fu_test_op_center_only(int on) { fu::g_conv_hooks.op_center_only = on ? 1 : 0; }
int fu_test_conv_f32_tile_rows(int B, int H, int W, int N) { return fu::conv3x3_f32_tile_rows(B, H, W, N); }

int fu_test_conv_route(int kind, int C0, int has_bn0, int C1, int D0, int D1, int center_only, int want_bnsums, int B, int H,
                       int W) {
  if (kind < 0 || kind > 2) return -1;
  return fu::query_route(kind, C0, has_bn0, C1, D0, D1, center_only, want_bnsums, B, H, W, nullptr);
}
const char* fu_test_conv_route_name(int kind, int route) {
  static const char* const conv[fu::CONV_NUM_ROUTES] = {"general64", "general32", "tap1_64", "tap1_32", "c8", "pp",
                                                        "rs8", "rs4", "fast_tall", "fast64", "fast32"};
  static const char* const wgrad[fu::WGRAD_NUM_ROUTES] = {"tap1_wide", "tap1_narrow", "c8", "pp", "lockstep128", "lockstep64"};
  if (kind == 2) return route >= 0 && route < fu::WGRAD_NUM_ROUTES ? wgrad[route] : "?";
  return (kind == 0 || kind == 1) && route >= 0 && route < fu::CONV_NUM_ROUTES ? conv[route] : "?";
}
int fu_test_wgrad_slab(int C0, int has_bn0, int C1, int Cout, int center_only, int B, int H, int W, int64_t* used_elems,
                       int64_t* bound_elems) {
  if (bound_elems) *bound_elems = fu::conv3x3_wgrad_slab_elems_bf16(C0 + (C1 > 0 ? C1 : 0), Cout, B, H, W);
  return fu::query_route(2, C0, has_bn0, C1, Cout, 0, center_only, 0, B, H, W, used_elems);
}
}
