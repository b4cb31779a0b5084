// bf16 3x3 convolutions for gfx950: im2col-free implicit GEMMs on v_mfma_f32_32x32x16_bf16 (fp32 accumulate): the weight
// pack, the general forward / dgrad kernel and the forward route decision.  (The weight gradient: fu_wgrad_bf16.hip.)
//
//   forward / dgrad : out[p][n] = sum_{tap,c} in[p+tap][c] * w[tap][n][c]
//       workgroup tile = (WM*64) output pixels (TH x 16) x (WN*64) channels, K chunks of 32 input channels;
//       each wave owns 64 px x 64 ch = 2x2 MFMA tiles (64 accumulator registers).  The halo tile of the virtual
//       two-source NHWC input is staged once per chunk as [pixel][32ch + 8 pad] (80-byte rows: conflict-free
//       ds_read_b128 fragments) with the producer's BatchNorm+ReLU applied on the way (fp32 math, one rounding to
//       bf16); weights as [tap][n][32ch + 8 pad].  Next chunk's global loads are issued before the MFMA block.
//       Epilogue: bias, bf16 NHWC stores (two destinations for dgrad), fp32 (sum, sumsq) partials per tile.
#include "fu_common.h"
#include "fu_conv_bf16.h"

#include <type_traits>

namespace fu {

// ------------------------------------------------------------------------------------------------
// weight packing (bf16): OIHW fp32 -> wf[tap][co][ci_pad] and wd[8-tap][ci_pad][co]
// ------------------------------------------------------------------------------------------------
__global__ void k_pack_bf16(const float* __restrict__ w, int Cout, int cin_real, int cin_pad,
                            bf16_t* __restrict__ wf, bf16_t* __restrict__ wd, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(idx % cin_pad);
    const int64_t r = idx / cin_pad;
    const int co = (int)(r % Cout);
    const int tap = (int)(r / Cout);
    const float v = ci < cin_real ? w[((int64_t)co * cin_real + ci) * 9 + tap] : 0.f;
    const bf16_t h = f2e(v);
    if (wf) wf[idx] = h;                                                    // [tap][co][ci]
    if (wd) wd[((int64_t)(8 - tap) * cin_pad + ci) * Cout + co] = h;        // [8-tap][ci][co]
  }
}

int launch_pack_conv3x3_bf16(const float* w_oihw, int Cout, int cin_real, int cin_pad, bf16_t* wfwd, bf16_t* wdgrad,
                             hipStream_t s) {
  const int64_t total = (int64_t)9 * cin_pad * Cout;
  int g = (int)((total + 255) / 256);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_pack_bf16, dim3(g), dim3(256), 0, s, w_oihw, Cout, cin_real, cin_pad, wfwd, wdgrad, total);
  FU_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// forward / dgrad
// ------------------------------------------------------------------------------------------------

template <int WM, int WN, int NTW>
struct BCfg {
  // WM x WN waves; each wave owns 64 pixels x (32*NTW) channels
  static constexpr int TW = 16, TH = 4 * WM, BN = 32 * NTW * WN, KC = 32, KCP = 40;
  static constexpr int NT = 64 * WM * WN;
  static constexpr int HWd = TW + 2, HHt = TH + 2, NHP = HHt * HWd;
  static constexpr int A_UNITS = NHP * 4, W_UNITS = 9 * BN * 4;   // 16-byte units (8 channels)
  static constexpr int A_ITERS = (A_UNITS + NT - 1) / NT, W_ITERS = (W_UNITS + NT - 1) / NT;
  static constexpr int AB_FLOATS = 2 * 1024;                      // BN scale/shift of source 0 (C0 <= 1024)
  static constexpr int SMEM_BYTES = (NHP + 9 * BN) * KCP * 2 + AB_FLOATS * 4;
};

template <int WM, int WN, int NTW>
__global__ __launch_bounds__(64 * WM * WN) void k_conv3x3_bf16(BConvP P) {
  using Cfg = BCfg<WM, WN, NTW>;
  constexpr int TW = Cfg::TW, TH = Cfg::TH, BN = Cfg::BN, KC = Cfg::KC, KCP = Cfg::KCP, NT = Cfg::NT;
  constexpr int HWd = Cfg::HWd, NHP = Cfg::NHP, A_ITERS = Cfg::A_ITERS, W_ITERS = Cfg::W_ITERS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* sA = reinterpret_cast<bf16_t*>(smem_raw);   // [NHP][KCP]
  bf16_t* sW = sA + NHP * KCP;                        // [9][BN][KCP]
  float* sAB = reinterpret_cast<float*>(sW + 9 * BN * KCP);  // [2][1024] BN scale / shift of source 0

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int coT = logical / P.nPix;
  const int pixT = logical - coT * P.nPix;
  const int tx = pixT % P.tilesX;
  const int t2 = pixT / P.tilesX;
  const int ty = t2 % P.tilesY;
  const int bb = t2 / P.tilesY;
  const int x0 = tx * TW, y0 = ty * TH, n0 = coT * BN;

  const bool has_bn = P.a0 != nullptr;
  if (has_bn) {
    for (int c = tid; c < P.C0; c += NT) { sAB[c] = P.a0[c]; sAB[1024 + c] = P.b0[c]; }
  }

  // ---- staging descriptors: loads are UNCONDITIONAL from clamped addresses (no branch, no early wait);
  //      masking to zero happens when the registers are written to LDS -----------------------------------
  const int aq = tid & 3;  // channel octet inside the chunk (NT % 4 == 0)
  int a_pix[A_ITERS];
  unsigned a_okmask = 0;
  static_for<0, A_ITERS>([&](auto I) {
    constexpr int it = decltype(I)::value;
    const int u = tid + it * NT;
    const int hp = u >> 2;
    const int hy = hp / HWd, hx = hp - hy * HWd;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (u < Cfg::A_UNITS) && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
    a_okmask |= ok ? (1u << it) : 0u;
    a_pix[it] = ok ? ((bb * P.H + iy) * P.W + ix) : 0;
  });
  int w_off[W_ITERS];
  unsigned w_okmask = 0;
  static_for<0, W_ITERS>([&](auto I) {
    constexpr int it = decltype(I)::value;
    const int u = tid + it * NT;
    const int q = u & 3;
    const int co = (u >> 2) % BN;
    const int tap = u / (4 * BN);
    const int n = n0 + co;
    const bool ok = (u < Cfg::W_UNITS) && n < P.N;
    w_okmask |= ok ? (1u << it) : 0u;
    w_off[it] = ok ? ((tap * P.N + n) * P.Cin + 8 * q) : 0;
  });
  uint4 ra[A_ITERS];
  uint4 rw[W_ITERS];

  auto load_chunk = [&](int k0) {
    const int c = k0 + 8 * aq;
    const bool cval = c < P.Cin;
    const bool from0 = c < P.C0;
    const bf16_t* base = (from0 || !cval) ? P.src0 : P.src1;
    const int cs = (from0 || !cval) ? P.C0 : P.C1;
    const int cc = !cval ? 0 : (from0 ? c : c - P.C0);
    static_for<0, A_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      ra[it] = *reinterpret_cast<const uint4*>(base + (int64_t)a_pix[it] * cs + cc);
    });
    // weights: ci = k0 + 8q; the last chunk of a ragged Cin is clamped to offset 0 and masked at store time
    static_for<0, W_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int q = (tid + it * NT) & 3;
      const bool wv = k0 + 8 * q < P.Cin;
      rw[it] = *reinterpret_cast<const uint4*>(P.wpk + (wv ? (int64_t)w_off[it] + k0 : 0));
    });
  };

  auto store_chunk = [&](int k0) {
    const int c = k0 + 8 * aq;
    const bool cval = c < P.Cin;
    const bool bn = has_bn && c < P.C0;
    float4 av0, av1, bv0, bv1;
    if (bn) {
      av0 = *reinterpret_cast<const float4*>(sAB + c);
      av1 = *reinterpret_cast<const float4*>(sAB + c + 4);
      bv0 = *reinterpret_cast<const float4*>(sAB + 1024 + c);
      bv1 = *reinterpret_cast<const float4*>(sAB + 1024 + c + 4);
    }
    static_for<0, A_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      if (u < Cfg::A_UNITS) {
        uint4 v = ra[it];
        if (bn) v = bn_relu_pack8(v, av0, av1, bv0, bv1);
        const bool keep = cval && ((a_okmask >> it) & 1u);   // component-wise: a ?: on uint4 lvalues would take
        v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u;         // addresses and demote the arrays to scratch
        v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
        *reinterpret_cast<uint4*>(sA + (u >> 2) * KCP + 8 * aq) = v;
      }
    });
    static_for<0, W_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      if (u < Cfg::W_UNITS) {
        const bool wv = (k0 + 8 * (u & 3) < P.Cin) && ((w_okmask >> it) & 1u);
        uint4 v = rw[it];
        v.x = wv ? v.x : 0u; v.y = wv ? v.y : 0u; v.z = wv ? v.z : 0u; v.w = wv ? v.w : 0u;
        *reinterpret_cast<uint4*>(sW + (u >> 2) * KCP + 8 * (u & 3)) = v;
      }
    });
  };

  f32x16 acc[2][NTW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment base offsets (bf16 elements)
  int aoff[2], boff[NTW];
  // m-tile = 2 image rows x 16 columns.  Lanes 16..31 (second row) take their columns ROTATED by HWd mod 16:
  // the halo pitch (18 pixels) would otherwise put rows 12..15 of the first image row and 4..11 of the second on the
  // same LDS bank slots inside every 16-lane ds_read_b128 group (2-way conflict on each A read; measured 38 % of the
  // LDS-active cycles).  With the rotation the 16 lanes of a group hit 16 distinct slots.
  const int mrow = l31 >> 4;
  const int mcol = mrow ? ((l31 - 16 - (HWd & 15)) & 15) : l31;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
    aoff[mt] = (((wm * 2 + mt) * 2 + mrow) * HWd + mcol) * KCP + 8 * lh;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) boff[nt] = (wn * 32 * NTW + nt * 32 + l31) * KCP + 8 * lh;

  const int nChunks = (P.Cin + KC - 1) / KC;
  load_chunk(0);
  for (int ch = 0; ch < nChunks; ++ch) {
    __syncthreads();            // previous chunk's fragment reads are done (and sAB is visible on the first pass)
    store_chunk(ch * KC);
    __syncthreads();
    if (ch + 1 < nChunks) load_chunk((ch + 1) * KC);   // raw loads stay in flight under the MFMA block
    // 18 k-steps (9 taps x 2 halves of the 32-channel chunk), software-pipelined by hand: the fragments of step
    // s+1 are requested from LDS before the MFMAs of step s are issued (hipcc otherwise issues each step's
    // ds_reads just in time and exposes one LDS latency per 4 MFMAs).
    frag8_t af[2][2], bfr[2][NTW];
    auto load_frags = [&](auto Sc, auto Bc) {
      constexpr int st = decltype(Sc)::value, buf = decltype(Bc)::value;
      constexpr int tap = st >> 1, ks = st & 1;
      constexpr int toff = ((tap / 3) * HWd + (tap % 3)) * KCP + ks * 16;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) af[buf][mt] = *reinterpret_cast<const frag8_t*>(sA + aoff[mt] + toff);
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
        bfr[buf][nt] = *reinterpret_cast<const frag8_t*>(sW + tap * BN * KCP + boff[nt] + ks * 16);
    };
    load_frags(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    static_for<0, 18>([&](auto S) {
      constexpr int st = decltype(S)::value, buf = st & 1;
      if constexpr (st + 1 < 18) {
        load_frags(std::integral_constant<int, st + 1>{}, std::integral_constant<int, buf ^ 1>{});
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of this step's MFMAs
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
          acc[mt][nt] = FU_MFMA32(af[buf][mt], bfr[buf][nt], acc[mt][nt]);
    });
  }

  // ---- epilogue ----------------------------------------------------------------------------------
  // The accumulator holds one channel per lane and 16 pixels in registers; a 2-byte store per value would make the
  // epilogue store-issue bound.  Two DPP exchanges inside each lane quad (xor 1, then xor 2) transpose 4 pixels x
  // 4 channels so that every lane owns 4 consecutive channels of ONE pixel: one 8-byte store per 4 registers,
  // each wave instruction writing 8 pixels x 64 contiguous bytes.
  float ssum[NTW], ssq[NTW];
  const int qj = l31 & 3;
  const bool q_even = !(l31 & 1), q_lo = qj < 2;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    ssum[nt] = 0.f; ssq[nt] = 0.f;
    const int n = n0 + wn * 32 * NTW + nt * 32 + l31;
    const bool nok = n < P.N;
    const float bias = (P.bias && nok) ? P.bias[n] : 0.f;
    const int nq = n & ~3;                       // first channel of this lane quad (N, D0 are multiples of 8)
    bf16_t* dst;
    int dstride, dn;
    if (nq < P.D0) { dst = P.dst0; dstride = P.D0; dn = nq; }
    else { dst = P.dst1; dstride = P.D1; dn = nq - P.D0; }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a = acc[mt][nt][4 * g + k];
          const int p = k + 8 * g + 4 * lh;                       // MFMA row -> pixel (second row rotated, see aoff)
          const int oy = y0 + (wm * 2 + mt) * 2 + (p >> 4);
          const int ox = x0 + ((p >> 4) ? ((p - 16 - (HWd & 15)) & 15) : p);
          if (nok && oy < P.H && ox < P.W) { ssum[nt] += a; ssq[nt] += a * a; }
          v[k] = a + bias;
        }
        // level 1: pairs of channels
        const float s01 = q_even ? v[1] : v[0];
        const float s23 = q_even ? v[3] : v[2];
        const float r01 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s01), 0xB1, 0xF, 0xF, true));
        const float r23 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s23), 0xB1, 0xF, 0xF, true));
        const unsigned A = q_even ? ((unsigned)f2e(v[0]) | ((unsigned)f2e(r01) << 16))
                                  : ((unsigned)f2e(r01) | ((unsigned)f2e(v[1]) << 16));
        const unsigned Bq = q_even ? ((unsigned)f2e(v[2]) | ((unsigned)f2e(r23) << 16))
                                   : ((unsigned)f2e(r23) | ((unsigned)f2e(v[3]) << 16));
        // level 2: pairs of channel pairs
        const unsigned send = q_lo ? Bq : A;
        const unsigned recv = (unsigned)__builtin_amdgcn_mov_dpp((int)send, 0x4E, 0xF, 0xF, true);
        uint2 o;
        o.x = q_lo ? A : recv;
        o.y = q_lo ? recv : Bq;
        const int p = qj + 8 * g + 4 * lh;       // this lane now owns pixel row qj of the register quad
        const int oy = y0 + (wm * 2 + mt) * 2 + (p >> 4);
        const int ox = x0 + ((p >> 4) ? ((p - 16 - (HWd & 15)) & 15) : p);
        if (nq < P.N && oy < P.H && ox < P.W)
          *reinterpret_cast<uint2*>(dst + (((int64_t)bb * P.H + oy) * P.W + ox) * dstride + dn) = o;
      }
    }
  }
  if (P.stats) {
    float* red = reinterpret_cast<float*>(smem_raw);  // [WM][BN][2]
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      ssum[nt] += __shfl_xor(ssum[nt], 32, 64);
      ssq[nt] += __shfl_xor(ssq[nt], 32, 64);
    }
    __syncthreads();
    if (lh == 0) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int cn = wn * 32 * NTW + nt * 32 + l31;
        red[(wm * BN + cn) * 2 + 0] = ssum[nt];
        red[(wm * BN + cn) * 2 + 1] = ssq[nt];
      }
    }
    __syncthreads();
    if (tid < BN && n0 + tid < P.N) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int m = 0; m < WM; ++m) { s += red[(m * BN + tid) * 2 + 0]; q += red[(m * BN + tid) * 2 + 1]; }
      float* o = P.stats + ((int64_t)pixT * P.N + n0 + tid) * 2;
      o[0] = s;
      o[1] = q;
    }
  }
}

int conv3x3_num_stat_tiles_bf16(int B, int H, int W) { return B * ceil_div(H, 16) * ceil_div(W, 16); }

template <int WM, int WN, int NTW>
static int launch_cfg(BConvP& P, const LaunchOpts& o, hipStream_t s) {
  using Cfg = BCfg<WM, WN, NTW>;
  conv_geometry(P, Cfg::TW, Cfg::TH, Cfg::BN);
  return launch_conv_kernel<k_conv3x3_bf16<WM, WN, NTW>>(dim3(P.nPix * P.nCo), dim3(Cfg::NT), Cfg::SMEM_BYTES, o, s, P);
}

// ---- the decision: which kernel a forward / dgrad launch runs.  What a kernel CAN run is its *_eligible predicate, beside
// the kernel; everything that is PREFERRED is here, with the measurement behind it. ----
// Workgroups that give every CU two: the threshold of the 64-channel tiles and of the row-stationary kernel.
static constexpr int CONV_TWO_PER_CU_WGS = 512;
// Tiles of the persistent kernel (one workgroup per CU for the whole launch): at least one per CU.  128 tiles leave half the
// chip idle -- 512 -> 256 at 32 x 32 measured 54.8 us against 50.5 on the two-workgroup kernel.
static constexpr int CONV_PP_MIN_TILES = 256;
// ... of a dgrad launch that is asked for the BatchNorm-backward sums of its destination: from 8 chunks on.  The sums are ~450
// vector instructions per wave and tile in the epilogue, which ran beside the other group's MFMA phase at ~8 cycles per
// instruction; on the two-chunk 256 x 256 layers that is the kernel's critical path (64 -> 64: 125 us against 114 on the
// two-workgroup kernel, whose second workgroup covers it); from 256 input channels on it disappears (512 -> 512 at 32 x 32: 63
// against 74 us).  With the epilogue in a phase of its own (fu_conv_pp.hip, body) the picture is the same -- one-stream trace,
// pp | rs<8>: 64 -> 64 at 256 x 256 125 / 117 | 115 / 114 us, 128 -> 64 at 128 x 128 65 | 54, 256 -> 128 at 64 x 64 49 | 44,
// 128 -> 128 at 128 x 128 92 | 83 (with the threshold at 64).
static constexpr int CONV_PP_BNB_MIN_CIN = 256;
// Tall tile of the fast kernel (16 x 32 pixels, 16-channel chunks).  Measured per layer against the square tile (bench shapes,
// one stream): 5-9 % faster where it still yields >= 2048 workgroups (the 256x256 layers; the 8-channel first conv 60 -> 46
// us), within +-4 % at 1024, 10 % slower at <= 512 -- hence the threshold.
static constexpr int CONV_TALL_MIN_WGS = 2048;

ConvRoute conv3x3_route(const BConvP& P, const LaunchOpts& o, const ConvHooks& h) {
  // workgroups of 64 channels x 16x16 or 16x32 pixels (exact quotients wherever the rs / pp kernels are eligible)
  const int64_t nco64 = ceil_div(P.N, 64);
  const int64_t wg256 = (int64_t)P.B * ceil_div(P.H, 16) * ceil_div(P.W, 16) * nco64;
  const int64_t wg512 = (int64_t)P.B * ceil_div(P.H, 32) * ceil_div(P.W, 16) * nco64;
  // Tile choice of the general and the fast kernel (all tiles are 16x16 = 256 output pixels).  Measured on MI355X
  // (profiles/): two 4-wave workgroups per CU (256x64 tile, 80 KB LDS) overlap one group's LDS staging with the other's MFMA
  // block and beat the 8-wave 256x128 tile (higher FLOP/byte but lock-step phases) on every layer that yields >= 512
  // workgroups; 256x32 keeps the small deep levels at >= 256 workgroups.  (Also tried and measured slower, hence not built:
  // the 8-wave 256x128 tile with single or double-buffered 16-channel LDS stages (810-900 TF where this one reaches 870-1040)
  // and a warp-specialised 4 loader + 4 compute wave version with two LDS stages (790-915 TF).  Removing the per-chunk
  // staging altogether lets the same MFMA loop run at 1200-1430 TF, so staging costs ~30 % on the deep layers.)
  const bool two_per_cu = P.N >= 64 && wg256 >= CONV_TWO_PER_CU_WGS;
  if (h.force_general || !conv3x3_bf16_fast_eligible(P)) return two_per_cu ? CONV_GENERAL_64 : CONV_GENERAL_32;
  const bool wide = two_per_cu && (!P.dst1 || P.D0 % 64 == 0);
  if (P.center_only) return wide ? CONV_TAP1_64 : CONV_TAP1_32;
  // 8 input channels (the network's first conv): the K = 72 kernel without LDS staging
  if (h.tile_mode == 0 && conv3x3_c8_eligible(P)) return CONV_C8;
  // persistent ping-pong kernel: tile mode 4 forces it; by default wherever it is preferred
  if (conv3x3_pp_eligible(P)) {
    const bool preferred = wg512 >= CONV_PP_MIN_TILES && (!wants_bnb(P, o) || P.Cin >= CONV_PP_BNB_MIN_CIN);
    if (h.tile_mode == 4 || (h.tile_mode == 0 && preferred)) return CONV_PP;
  }
  // Row-stationary kernel, wherever the shape is eligible and one of its tiles gives every CU two workgroups.  Measured per
  // layer against the fast kernel (bench shapes, forward, tools/conv_modes.py): 5-11 % faster on the 128x128, 64x64 and 32x32
  // layers with N >= 512 channels x tiles, equal on the two-chunk 256x256 layers, slower below 512 workgroups (16x16 level,
  // 512 -> 256 at 32x32).  Tile mode 3 forces it, modes 1 / 2 exclude it.  16 x 32-pixel tiles where they still give every
  // CU two workgroups, 16 x 16 otherwise.
  if (conv3x3_rs_eligible(P) && (h.tile_mode == 3 || (h.tile_mode == 0 && wg256 >= CONV_TWO_PER_CU_WGS)))
    return (P.H % 32) == 0 && wg512 >= CONV_TWO_PER_CU_WGS ? CONV_RS8 : CONV_RS4;
  const bool tall = h.tile_mode == 2 ? wide : (h.tile_mode == 0 && wide && wg512 >= CONV_TALL_MIN_WGS);
  if (tall) return CONV_FAST_TALL;
  return wide ? CONV_FAST_64 : CONV_FAST_32;
}

int launch_conv3x3_bf16(const ConvIn& in, const bf16_t* wpk, const float* bias, bf16_t* dst0, int D0, bf16_t* dst1,
                        int D1, float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s) {
  BConvP P;
  P.src0 = (const bf16_t*)in.src0; P.src1 = (const bf16_t*)in.src1; P.a0 = in.a0; P.b0 = in.b0;
  P.wpk = wpk; P.bias = bias; P.dst0 = dst0; P.dst1 = dst1; P.stats = stats;
  P.C0 = in.C0; P.C1 = in.src1 ? in.C1 : 0; P.Cin = P.C0 + P.C1; P.N = D0 + D1; P.D0 = D0; P.D1 = D1;
  P.B = B; P.H = H; P.W = W;
  P.center_only = (in.center_only && !g_conv_hooks.full_taps) ? 1 : 0;
  P.bnb_y = nullptr; P.bnb_a = P.bnb_b = P.bnb_mean = P.bnb_invstd = nullptr; P.bnb_part = nullptr;
  FU_REQUIRE(P.C0 % 8 == 0 && P.C1 % 8 == 0, "conv3x3_bf16: input channel counts must be multiples of 8 (C0=%d C1=%d)",
             P.C0, P.C1);
  FU_REQUIRE(P.a0 == nullptr || P.C0 <= 1024, "conv3x3_bf16: at most 1024 BN-activated channels in source 0 (got %d)",
             P.C0);   // (the LDS table of BN coefficients; a plain source has no such limit)
  int st = 1;
  const ConvRoute r = conv3x3_route(P, in.opt, g_conv_hooks);
  switch (r) {
    case CONV_GENERAL_64: st = launch_cfg<4, 1, 2>(P, in.opt, s); break;
    case CONV_GENERAL_32: st = launch_cfg<4, 1, 1>(P, in.opt, s); break;
    case CONV_C8: st = launch_conv3x3_c8(P, in.opt, s); break;
    case CONV_PP: st = launch_conv3x3_pp(P, in.opt, s); break;
    case CONV_RS8: st = launch_conv3x3_rs(P, true, in.opt, s); break;
    case CONV_RS4: st = launch_conv3x3_rs(P, false, in.opt, s); break;
    case CONV_TAP1_64: case CONV_TAP1_32: case CONV_FAST_TALL: case CONV_FAST_64: case CONV_FAST_32:
      st = launch_conv3x3_bf16_fast(P, r, in.opt, s); break;
    case CONV_NUM_ROUTES: break;
  }
  if (n_stat_tiles) *n_stat_tiles = P.nPix;
  return st;
}

}  // namespace fu
