// bf16 3x3 weight gradient for gfx950: dW[tap][c][n] = sum_p in[p+tap][c] * dy[p][n] on v_mfma_f32_32x32x16_bf16.
//       M = 64 c_in, N = 64 c_out, K = pixels.  Both operands need K (= pixels) contiguous per lane while memory is
//       channel-contiguous: the tiles are staged untransposed ([pixel][64ch + 32 pad], 192-byte rows) and the
//       fragments are fetched with the hardware transposing read ds_read_b64_tr_b16.  9 accumulator tiles per
//       wave (one per tap); split-K slabs in fp32, reduced by the shared fixed-order kernel.
// Three kernels (lock-step, ping-pong, the 8-band first conv), the route decision and the split-K plan.
#include "fu_common.h"
#include "fu_conv_bf16.h"

#include <algorithm>
#include <type_traits>

namespace fu {

// Two transposing reads -> one MFMA fragment.  NOTE (hipcc / ROCm 7.2): the v4i16 form of the builtin followed by
// per-element bit casts to __bf16 is miscompiled (element 0 is replicated); the v4bf16 form + shufflevector is correct
// (checked on hardware, tools/probes/tr_probe3.hip).
__device__ __forceinline__ frag8_t tr_frag(const bf16_t* p0, const bf16_t* p1) {
  typedef __attribute__((address_space(3))) tr4_t lds_tr4;
  const tr4_t v = FU_TR16((lds_tr4*)p0);
  const tr4_t w = FU_TR16((lds_tr4*)p1);
  return __builtin_bit_cast(frag8_t, __builtin_shufflevector(v, w, 0, 1, 2, 3, 4, 5, 6, 7));
}

// WMI waves along c_in (32 each) x 2 waves along c_out (32 each); pixel stage = PTH x 16 pixels with halo.
template <int WMI, int PTH>
struct WCfg {
  static constexpr int CI_T = 32 * WMI, CO_T = 64, NT = 128 * WMI, PTW = 16;
  static constexpr int HWd = PTW + 2, NHP = (PTH + 2) * HWd, NPX = PTH * PTW;
  static constexpr int RSX = CI_T + 32, RSD = CO_T + 32;    // row strides (elements): 64-byte residue mod 256 B
  static constexpr int XQ = CI_T / 8, DQ = CO_T / 8;        // 16-byte units per pixel row
  static constexpr int X_UNITS = NHP * XQ, D_UNITS = NPX * DQ;
  static constexpr int X_ITERS = (X_UNITS + NT - 1) / NT, D_ITERS = (D_UNITS + NT - 1) / NT;
  static constexpr int SMEM_BYTES = (NHP * RSX + NPX * RSD) * 2 + 2 * CI_T * 4;
};

// ------------------------------------------------------------------------------------------------
// What the lock-step and the ping-pong kernel share (Cfg = WCfg<..> or WPCfg).  The launch parameters go in BY VALUE: a helper
// that takes the kernel's BWgP by const reference grew every k_wgrad_bf16 instantiation.  Three pieces of the same text stay in
// both kernels (profiles/README.md has the figures): the fill of sAB and the thread's channel octets -- as a helper (by value,
// by reference, forced inline or not) either of them alone turns k_wgrad_bf16_pp<true> into other code, inverted compares and
// branch senses in its staging dispatch, 44 bytes shorter and 0.4 - 1.4 % faster -- and the a / b fetch from sAB, which as a
// helper reordered the instructions of four kernels and put k_wgrad_bf16_pp<true> 0.1 % outside the parent's spread.
// ------------------------------------------------------------------------------------------------
// workgroup -> (split-K slab, first c_in of its tile, first c_out of its tile), through xcd_remap
struct WTile { int split, ci0, co0; };
template <typename Cfg>
__device__ __forceinline__ WTile wgrad_tile(BWgP P) {
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int nT = P.nCi * P.nCo;
  const int split = logical / nT;
  const int t = logical - split * nT;
  const int ciT = t / P.nCo, coT = t - ciT * P.nCo;
  return {split, ciT * Cfg::CI_T, coT * Cfg::CO_T};
}

// The MFMA phase of one stage.  Walk the halo rows once: the X fragment of (halo row hr, column shift dx) feeds up to three
// taps (dy = 0..2 with pixel row r = hr - dy), so every fragment is fetched from LDS once; dy fragments of the last three pixel
// rows stay in a 4-deep register ring, x fragments in a ring AHEAD steps in front of the MFMAs.  The kernel's loaders fill the
// rings: loadA(st) puts the x fragment of step st = 3 hr + dx into Af[st % (AHEAD + 1)], loadB(r) the dy fragment of pixel row
// r into Bf[r & 3].  wgrad_prefetch requests the first ones; the walk requests step st + AHEAD before the MFMAs of step st.
template <int AHEAD, typename LA, typename LB>
__device__ __forceinline__ void wgrad_prefetch(const LA& loadA, const LB& loadB) {
  loadB(std::integral_constant<int, 0>{});
  static_for<0, AHEAD>([&](auto Sc) { loadA(Sc); });
}
template <int PTH, int AHEAD, typename LA, typename LB>
__device__ __forceinline__ void wgrad_walk(f32x16 (&acc)[9], const frag8_t (&Af)[AHEAD + 1], const frag8_t (&Bf)[4],
                                           const LA& loadA, const LB& loadB) {
  constexpr int NA = AHEAD + 1, NST = 3 * (PTH + 2);
  static_for<0, NST>([&](auto S) {
    constexpr int st = decltype(S)::value, hr = st / 3, dx = st % 3;
    if constexpr (st + AHEAD < NST) loadA(std::integral_constant<int, st + AHEAD>{});
    if constexpr (dx == 0 && hr + 1 < PTH) loadB(std::integral_constant<int, hr + 1>{});
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 3>([&](auto DY) {
      constexpr int dy = decltype(DY)::value, r = hr - dy;
      if constexpr (r >= 0 && r < PTH)
        acc[dy * 3 + dx] = FU_MFMA32(Af[st % NA], Bf[r & 3], acc[dy * 3 + dx]);
    });
  });
}

// slab[split][tap][Cin / 4][Cout][4] (see k_wgrad_reduce_oihw): accumulator registers 4j .. 4j+3 of a lane are c_in
// 8j + 4 lh + {0..3} of its c_out -- one 16-byte store, 512 contiguous bytes per 32 lanes.  (TAPS = 1: the centre tap's slab.)
template <int TAPS>
__device__ __forceinline__ void wgrad_store_slab(BWgP P, const f32x16 (&acc)[TAPS], WTile w, int mi, int ni, int l31, int lh) {
  const int co = w.co0 + ni * 32 + l31;
  if (co < P.Cout) {
    const int cq = P.Cin >> 2;                       // Cin % 8 == 0 (launch_conv3x3_wgrad_bf16)
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int tap = TAPS == 9 ? t : 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ci = w.ci0 + mi * 32 + 8 * j + 4 * lh;
        if (ci < P.Cin)
          *reinterpret_cast<float4*>(P.slab + ((((int64_t)w.split * 9 + tap) * cq + (ci >> 2)) * P.Cout + co) * 4) =
              make_float4(acc[t][4 * j], acc[t][4 * j + 1], acc[t][4 * j + 2], acc[t][4 * j + 3]);
      }
    }
  }
}

// TAPS = 9: the 3x3 weight gradient.  TAPS = 1: only its centre tap (the embedded 1x1 fusion convs of the late-fusion
// net): 8 MFMAs per stage instead of 72; the other eight tap slabs are left unwritten and must not be read.
template <int WMI, int PTH, int TAPS = 9>
__global__ __launch_bounds__(128 * WMI) void k_wgrad_bf16(BWgP P) {
  using Cfg = WCfg<WMI, PTH>;
  constexpr int CI_T = Cfg::CI_T, NT = Cfg::NT, HWd = Cfg::HWd, NHP = Cfg::NHP, NPX = Cfg::NPX;
  constexpr int RSX = Cfg::RSX, RSD = Cfg::RSD, XQ = Cfg::XQ, DQ = Cfg::DQ;
  constexpr int X_ITERS = Cfg::X_ITERS, D_ITERS = Cfg::D_ITERS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* sX = reinterpret_cast<bf16_t*>(smem_raw);   // [NHP][RSX]
  bf16_t* sD = sX + NHP * RSX;                        // [NPX][RSD]
  float* sAB = reinterpret_cast<float*>(sD + NPX * RSD);  // [2][CI_T] BN scale / shift of this c_in tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int mi = wave >> 1, ni = wave & 1;

  const WTile w = wgrad_tile<Cfg>(P);
  const int ci0 = w.ci0, co0 = w.co0;

  f32x16 acc[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

  // transposing-read lane roles: group g = lane>>4 -> channel block 16*(g&1), pixel half g>>1 (= lh);
  // within the group lane 4q+p supplies the address of pixel q, channels 4p..4p+3
  const int g = lane >> 4, gi = lane & 15, tq = gi >> 2, tp = gi & 3;
  const int tr_ch = 16 * (g & 1) + 4 * tp;
  const int tr_px = 8 * lh + tq;   // column inside the 16-pixel row (second read: +4)

  const bool has_bn = P.a0 != nullptr;
  if (has_bn) {
    for (int c = tid; c < CI_T; c += NT) {
      const int cc = ci0 + c;
      const bool ok = cc < P.C0;
      sAB[c] = ok ? P.a0[cc] : 1.f;
      sAB[CI_T + c] = ok ? P.b0[cc] : 0.f;
    }
  }
  // this thread's channel octets (NT % XQ == 0 and NT % DQ == 0)
  const int xq = tid % XQ, dq = tid % DQ;
  const int cX = ci0 + 8 * xq;
  const int cD = co0 + 8 * dq;
  const bool xval = cX < P.Cin, dval = cD < P.Cout;
  const bool from0 = cX < P.C0;
  const bool xbn = has_bn && from0 && xval;
  const bf16_t* xbase = (from0 || !xval) ? P.src0 : P.src1;
  const int xcs = (from0 || !xval) ? P.C0 : P.C1;
  const int xcc = !xval ? 0 : (from0 ? cX : cX - P.C0);
  const int dcc = dval ? cD : 0;

  uint4 rx[X_ITERS], rd[D_ITERS];
  unsigned xmask = 0, dmask = 0;

  auto load_tile = [&](int pt) {
    const int tx = pt % P.tilesX;
    const int t2 = pt / P.tilesX;
    const int bb = t2 / P.tilesY;
    const int y0 = (t2 % P.tilesY) * PTH;
    const int x0 = tx * Cfg::PTW;
    xmask = 0; dmask = 0;
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      const int hp = u / XQ;
      const int hy = hp / HWd, hx = hp - hy * HWd;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      const bool ok = (u < Cfg::X_UNITS) && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
      xmask |= ok ? (1u << it) : 0u;
      const int pix = ok ? ((bb * P.H + iy) * P.W + ix) : 0;
      rx[it] = *reinterpret_cast<const uint4*>(xbase + (int64_t)pix * xcs + xcc);
    });
    static_for<0, D_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      const int p = u / DQ;
      const int oy = y0 + (p >> 4), ox = x0 + (p & 15);
      const bool ok = (u < Cfg::D_UNITS) && oy < P.H && ox < P.W;
      dmask |= ok ? (1u << it) : 0u;
      const int pix = ok ? ((bb * P.H + oy) * P.W + ox) : 0;
      rd[it] = *reinterpret_cast<const uint4*>(P.dy + (int64_t)pix * P.Cout + dcc);
    });
  };
  auto store_tile = [&]() {
    float4 av0, av1, bv0, bv1;
    if (xbn) {
      av0 = *reinterpret_cast<const float4*>(sAB + 8 * xq);
      av1 = *reinterpret_cast<const float4*>(sAB + 8 * xq + 4);
      bv0 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq);
      bv1 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq + 4);
    }
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      if (u < Cfg::X_UNITS) {
        uint4 v = rx[it];
        if (xbn) v = bn_relu_pack8(v, av0, av1, bv0, bv1);
        const bool keep = xval && ((xmask >> it) & 1u);
        v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u; v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
        *reinterpret_cast<uint4*>(sX + (u / XQ) * RSX + 8 * xq) = v;
      }
    });
    static_for<0, D_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int u = tid + it * NT;
      if (u < Cfg::D_UNITS) {
        uint4 v = rd[it];
        const bool keep = dval && ((dmask >> it) & 1u);
        v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u; v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
        *reinterpret_cast<uint4*>(sD + (u / DQ) * RSD + 8 * dq) = v;
      }
    });
  };

  const int pt0 = w.split * P.perSplit;
  const int pt1 = min(P.nPix, pt0 + P.perSplit);
  if (pt0 < pt1) load_tile(pt0);
  for (int pt = pt0; pt < pt1; ++pt) {
    __syncthreads();            // previous stage's fragment reads are done (sAB visible on the first pass)
    store_tile();
    __syncthreads();
    // in flight under the MFMA block.  ALWAYS issued (the last stage re-reads its own tile): under `if (pt + 1 < pt1)`
    // the staging registers are phis of a loaded and a not-loaded path, hipcc copies some of them right behind the
    // loads and waits for them (vmcnt) in front of the MFMA block -- with one workgroup per CU nothing covers that
    load_tile(min(pt + 1, pt1 - 1));
    frag8_t Af[2], Bf[4];
    auto loadA = [&](auto Sc) {
      constexpr int st = decltype(Sc)::value, hr = st / 3, dx = st % 3;
      const bf16_t* ad = sX + (hr * HWd + tr_px + dx) * RSX + mi * 32 + tr_ch;
      Af[st & 1] = tr_frag(ad, ad + 4 * RSX);
    };
    auto loadB = [&](auto Rc) {
      constexpr int r = decltype(Rc)::value;
      const bf16_t* bd = sD + (r * 16 + tr_px) * RSD + ni * 32 + tr_ch;
      Bf[r & 3] = tr_frag(bd, bd + 4 * RSD);
    };
    if constexpr (TAPS == 9) {      // the walk of wgrad_walk, next step's x fragment requested before this step's MFMAs
      wgrad_prefetch<1>(loadA, loadB);
      wgrad_walk<PTH, 1>(acc, Af, Bf, loadA, loadB);
    } else {
      // centre tap only: pixel row r pairs halo row r + 1, column shift 1 (stage index 3 (r + 1) + 1 of loadA)
      loadB(std::integral_constant<int, 0>{});
      loadA(std::integral_constant<int, 4>{});
      static_for<0, PTH>([&](auto R) {
        constexpr int r = decltype(R)::value;
        if constexpr (r + 1 < PTH) {
          loadA(std::integral_constant<int, 3 * (r + 2) + 1>{});
          loadB(std::integral_constant<int, r + 1>{});
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[0] = FU_MFMA32(Af[(3 * (r + 1) + 1) & 1], Bf[r & 3], acc[0]);
      });
    }
  }
  wgrad_store_slab<TAPS>(P, acc, w, mi, ni, l31, lh);
}


// ------------------------------------------------------------------------------------------------
// wgrad, ping-pong version for c_in tiles of 128 (8 waves, one workgroup per CU)
//
// k_wgrad_bf16<4,8> spends half of every stage with the MFMA pipe idle (s_memtime stamps: per stage 4450 cycles of
// MFMA work for the two waves of a SIMD, 2400 BN/ReLU + LDS store, 1900 load issue at the texture unit's 64 B/clk, all
// in lock step because the single LDS stage needs two barriers).  Here the stage is double-buffered (rows unpadded and
// XOR-swizzled by 64-byte chunk instead, 2 x 62.5 KB) and the 8 waves form two groups half a stage apart: while waves
// 0-3 multiply stage n (one wave per SIMD feeds the MFMA pipe alone), waves 4-7 activate and store their half of the
// next stage and issue the loads after that, then the roles swap.  Every wave runs the same instruction stream
// { MFMA(n) ; barrier ; store(n+1+grp), load(n+2+grp) ; barrier }; group 1 is shifted by one pre-loop staging step and
// group 0 pays the matching barrier after the loop.  Accumulators, split-K slabs and the reduce are unchanged, so the
// results are bit-identical to k_wgrad_bf16<4,8>.
// ------------------------------------------------------------------------------------------------
struct WPCfg {
  static constexpr int CI_T = 128, CO_T = 64, NT = 512, PTH = 8, PTW = 16, GT = 256;
  static constexpr int HWd = PTW + 2, NHP = (PTH + 2) * HWd, NPX = PTH * PTW;
  static constexpr int RSX = CI_T, RSD = CO_T;               // unpadded rows (elements)
  static constexpr int XQ = CI_T / 8, DQ = CO_T / 8;
  static constexpr int XH_UNITS = NHP * XQ / 2, DH_UNITS = NPX * DQ / 2;   // per group
  static constexpr int X_ITERS = (XH_UNITS + GT - 1) / GT, D_ITERS = (DH_UNITS + GT - 1) / GT;
  static constexpr int BUF_ELEMS = NHP * RSX + NPX * RSD;
  static constexpr int SMEM_BYTES = 2 * BUF_ELEMS * 2 + 2 * CI_T * 4;
  static_assert((NHP * XQ) % 2 == 0 && XH_UNITS % XQ == 0 && DH_UNITS % DQ == 0, "halves split on row boundaries");
};

//
// FAST (round 2): the staging half of a stage was ~470 instructions per thread against 72 MFMAs of the other group -- the
// stage was issue-bound on tile decode (three integer divisions), per-slot bounds tests, 64-bit address products, per-slot
// select masks and one convert + one permute per CHANNEL.  With whole tiles (H % 8 == 0, W % 16 == 0), whole channel tiles
// (Cin % 128 == 0, Cout % 64 == 0) and < 2^24 pixels everything per slot is a thread constant: the byte offset of the slot
// from the tile's origin pixel (relX / relD), four bit sets naming the slots that fall off the image when the tile touches
// the top / bottom / left / right border, and LDS addresses that differ by immediates.  Per stage the decode is scalar
// (multiply-high by host reciprocals), a load is one add (+ the 64-bit base), interior tiles carry no masks at all, and
// the BatchNorm + ReLU converts channel PAIRS (v_cvt_pk with both operands).  Lanes of an un-normalised second source take
// a = 1, b = 0 and a NaN floor (v_max_f32 returns the other operand), so the stream has no divergent branch.  The
// arithmetic per element is unchanged: results are bit-identical to FAST = false, which keeps every other shape.
template <bool FAST>
__global__ __launch_bounds__(512) void k_wgrad_bf16_pp(BWgP P) {
  using Cfg = WPCfg;
  constexpr int CI_T = Cfg::CI_T, GT = Cfg::GT, HWd = Cfg::HWd, NHP = Cfg::NHP;
  constexpr int PTH = Cfg::PTH, RSX = Cfg::RSX, RSD = Cfg::RSD, XQ = Cfg::XQ, DQ = Cfg::DQ;
  constexpr int X_ITERS = Cfg::X_ITERS, D_ITERS = Cfg::D_ITERS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* sBuf = reinterpret_cast<bf16_t*>(smem_raw);                       // 2 x { X [NHP][RSX], D [NPX][RSD] }
  float* sAB = reinterpret_cast<float*>(sBuf + 2 * Cfg::BUF_ELEMS);         // [2][CI_T]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int grp = __builtin_amdgcn_readfirstlane(wave >> 2), tg = tid & (GT - 1);
  // staging halves: group 1 stages the TOP half of a stage (halo rows 0-4, dy rows 0-3), group 0 the bottom half.  A group
  // stores its half of its next stage right before it multiplies that stage; the other half was stored by the other
  // group one interval earlier, i.e. in front of a barrier this group has already passed.  With the top half coming from
  // the OTHER group, the first fragments of the next MFMA phase (row 0) can be requested before the barrier that ends
  // the staging, and their LDS latency (the phase measured 2650 cycles for 2304 of MFMA work with an idle partner: the
  // pipe waits ~250 cycles for its first fragments) overlaps the barrier wait.
  const int hg = 1 - grp;
  const int mi = wave & 3;                 // c_in block of this wave; both c_out blocks: see ni below
  // waves 0-3 and 4-7 must split the MFMA work so that each group covers all (mi, ni): wave = 4*grp + w, w = 0..3
  // -> group g owns c_out block ni = g, all four c_in blocks
  const int ni = grp;

  const WTile w = wgrad_tile<Cfg>(P);
  const int ci0 = w.ci0, co0 = w.co0;

  f32x16 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

  const int g = lane >> 4, gi = lane & 15, tq = gi >> 2, tp = gi & 3;
  const int tr_ch = 16 * (g & 1) + 4 * tp;
  const int tr_px = 8 * lh + tq;
  // swizzled fragment offsets (elements).  X: 64-byte chunk mi of row r sits at chunk mi ^ (r & 3); the rows of a
  // fragment are c + tr_px (+4) with c a compile-time constant, so four lane offsets cover c & 3 = 0..3.
  int aoff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) aoff[j] = tr_px * RSX + ((mi ^ ((j + tr_px) & 3)) * 32) + tr_ch;
  // D: 128-byte rows, chunk ni of row r at chunk ni ^ ((r >> 1) & 1); rows are 16 r + tr_px (+4)
  const int boff = tr_px * RSD + ((ni ^ ((tr_px >> 1) & 1)) * 32) + tr_ch;

  const bool has_bn = P.a0 != nullptr;
  if (has_bn) {
    for (int c = tid; c < CI_T; c += Cfg::NT) {
      const int cc = ci0 + c;
      const bool ok = cc < P.C0;
      sAB[c] = ok ? P.a0[cc] : 1.f;
      sAB[CI_T + c] = ok ? P.b0[cc] : 0.f;
    }
  }
  const int xq = tid & (XQ - 1), dq = tid & (DQ - 1);
  const int cX = ci0 + 8 * xq;
  const int cD = co0 + 8 * dq;
  const bool xval = cX < P.Cin, dval = cD < P.Cout;
  const bool from0 = cX < P.C0;
  const bool xbn = has_bn && from0 && xval;
  const bf16_t* xbase = (from0 || !xval) ? P.src0 : P.src1;
  const int xcs = (from0 || !xval) ? P.C0 : P.C1;
  const int xcc = !xval ? 0 : (from0 ? cX : cX - P.C0);
  const int dcc = dval ? cD : 0;

  uint4 rx[X_ITERS], rd[D_ITERS];
  unsigned xmask = 0, dmask = 0;

  auto load_half = [&](auto pt) __attribute__((always_inline)) {      // (generic: only instantiated where used, i.e. for FAST = false)
    const int tx = pt % P.tilesX;
    const int t2 = pt / P.tilesX;
    const int bb = t2 / P.tilesY;
    const int y0 = (t2 % P.tilesY) * PTH;
    const int x0 = tx * Cfg::PTW;
    xmask = 0; dmask = 0;
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int ul = tg + it * GT;
      const int hp = (hg * Cfg::XH_UNITS + ul) / XQ;
      const int hy = hp / HWd, hx = hp - hy * HWd;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      const unsigned ok = unsigned(ul < Cfg::XH_UNITS) & unsigned((unsigned)iy < (unsigned)P.H) &
                          unsigned((unsigned)ix < (unsigned)P.W);   // bitwise: no exec-mask branches
      xmask |= ok << it;
      const int pix = ok ? ((bb * P.H + iy) * P.W + ix) : 0;
      rx[it] = *reinterpret_cast<const uint4*>(xbase + (int64_t)pix * xcs + xcc);
    });
    static_for<0, D_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int ul = tg + it * GT;
      const int p = (hg * Cfg::DH_UNITS + ul) / DQ;
      const int oy = y0 + (p >> 4), ox = x0 + (p & 15);
      const unsigned ok = unsigned(ul < Cfg::DH_UNITS) & unsigned(oy < P.H) & unsigned(ox < P.W);
      dmask |= ok << it;
      const int pix = ok ? ((bb * P.H + oy) * P.W + ox) : 0;
      rd[it] = *reinterpret_cast<const uint4*>(P.dy + (int64_t)pix * P.Cout + dcc);
    });
  };
  auto store_half = [&](auto* sX) __attribute__((always_inline)) {
    bf16_t* sD = sX + NHP * RSX;
    float4 av0, av1, bv0, bv1;
    if (xbn) {
      av0 = *reinterpret_cast<const float4*>(sAB + 8 * xq);
      av1 = *reinterpret_cast<const float4*>(sAB + 8 * xq + 4);
      bv0 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq);
      bv1 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq + 4);
    }
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int ul = tg + it * GT;
      if (ul < Cfg::XH_UNITS) {
        uint4 v = rx[it];
        // (the packed form of the fast conv kernel -- v_pk_fma_f32 / v_pk_max_i16 -- is 90 instructions shorter per
        // stage here and was measured 10 % SLOWER, same box: 8.30 -> 9.15 ms per 98 launches)
        if (xbn) v = bn_relu_pack8(v, av0, av1, bv0, bv1);
        const bool keep = xval && ((xmask >> it) & 1u);
        v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u; v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
        const int hp = (hg * Cfg::XH_UNITS + ul) / XQ;
        *reinterpret_cast<uint4*>(sX + hp * RSX + 8 * (xq ^ ((hp & 3) << 2))) = v;
      }
    });
    static_for<0, D_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int ul = tg + it * GT;
      if (ul < Cfg::DH_UNITS) {
        uint4 v = rd[it];
        const bool keep = dval && ((dmask >> it) & 1u);
        v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u; v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
        const int p = (hg * Cfg::DH_UNITS + ul) / DQ;
        *reinterpret_cast<uint4*>(sD + p * RSD + 8 * (dq ^ (((p >> 1) & 1) << 2))) = v;
      }
    });
  };

  // ---- FAST staging (see the kernel's header comment)
  constexpr int X_FULL = Cfg::XH_UNITS / GT;                 // slots every thread of the group owns (the last one is partial)
  unsigned relX[X_ITERS], relD[D_ITERS];                     // byte offsets from the tile's origin pixel (mod 2^32)
  unsigned mT = 0, mB = 0, mL = 0, mR = 0;                   // bit it: slot it lies in the halo row / column of that side
  unsigned xbad = 0;                                         // slots of the tile in registers that are outside the image
  bool xborder = false;                                      // (uniform) ... and whether there is any
  const unsigned cs2 = (unsigned)xcs * 2u;
  const char* xb = reinterpret_cast<const char*>(xbase + xcc);
  const char* db = reinterpret_cast<const char*>(P.dy + dcc);
  const float relu_floor = (has_bn && !from0) ? __builtin_nanf("") : 0.f;
  unsigned ldsX0 = 0, ldsD0 = 0;                             // LDS byte offsets of slot 0 inside a buffer
  uint4 rdf0, rdf1;                                          // the two dy units in flight (named: as an array they went to scratch)
  if constexpr (FAST) {
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int ul = tg + it * GT;
      const bool own = ul < Cfg::XH_UNITS;
      const int hp = (hg * Cfg::XH_UNITS + ul) / XQ;
      const int hy = hp / HWd, hx = hp - hy * HWd;
      relX[it] = own ? (unsigned)(((hy - 1) * P.W + (hx - 1)) * (int)cs2) : 0u;     // not owned: the origin pixel, never stored
      mT |= (own && hy == 0) ? (1u << it) : 0u;  mB |= (own && hy == PTH + 1) ? (1u << it) : 0u;
      mL |= (own && hx == 0) ? (1u << it) : 0u;  mR |= (own && hx == HWd - 1) ? (1u << it) : 0u;
    });
    static_for<0, D_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      const int p = (hg * Cfg::DH_UNITS + tg + it * GT) / DQ;
      relD[it] = (unsigned)(((p >> 4) * P.W + (p & 15)) * P.Cout * 2);
    });
    const int hp0 = (hg * Cfg::XH_UNITS + tg) / XQ;         // slot it: halo pixel hp0 + 16 it, same swizzle
    ldsX0 = (unsigned)(hp0 * RSX + 8 * (xq ^ ((hp0 & 3) << 2))) * 2u;
    const int p0 = (hg * Cfg::DH_UNITS + tg) / DQ;          // slot it: pixel p0 + 32 it, same swizzle
    ldsD0 = (unsigned)((NHP * RSX) + p0 * RSD + 8 * (dq ^ (((p0 >> 1) & 1) << 2))) * 2u;
  }
  auto load_half_fast = [&](int pt) __attribute__((always_inline)) {                        // pt uniform
    const int t2 = fast_div(pt, P.tilesX, P.rcp_tilesX);
    const int tx = pt - t2 * P.tilesX;
    const int bb = fast_div(t2, P.tilesY, P.rcp_tilesY);
    const int y0 = (t2 - bb * P.tilesY) * PTH, x0 = tx * Cfg::PTW;
    const unsigned tile_pix = (unsigned)((bb * P.H + y0) * P.W + x0);
    const unsigned ft = y0 == 0 ? ~0u : 0u, fb = y0 + PTH == P.H ? ~0u : 0u;
    const unsigned fl = x0 == 0 ? ~0u : 0u, fr = x0 + Cfg::PTW == P.W ? ~0u : 0u;
    xborder = (ft | fb | fl | fr) != 0u;
    xbad = (mT & ft) | (mB & fb) | (mL & fl) | (mR & fr);
    const unsigned tX = (tile_pix & 0xffffffu) * (cs2 & 0xffffffu);                // v_mul_u32_u24 (eligibility: < 2^24 each)
    const char* dbt = db + (size_t)tile_pix * (size_t)(P.Cout * 2);                // uniform
    if (xborder) {
      const unsigned good = ~xbad;
      static_for<0, X_ITERS>([&](auto I) {
        constexpr int it = decltype(I)::value;
        const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)good, it, 1);      // bit it -> 0 / 0xffffffff
        rx[it] = *reinterpret_cast<const uint4*>(xb + (tX + (relX[it] & m)));      // off the image: the origin pixel
      });
    } else {
      static_for<0, X_ITERS>([&](auto I) {
        constexpr int it = decltype(I)::value;
        rx[it] = *reinterpret_cast<const uint4*>(xb + (tX + relX[it]));
      });
    }
    static_assert(D_ITERS == 2, "two dy units per thread and stage");
    rdf0 = *reinterpret_cast<const uint4*>(dbt + relD[0]);
    rdf1 = *reinterpret_cast<const uint4*>(dbt + relD[1]);
  };
  auto store_half_fast = [&](bf16_t* sXb, auto Mc, auto Bc) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(Mc)::value, BNR = decltype(Bc)::value;
    unsigned char* lx = reinterpret_cast<unsigned char*>(sXb) + ldsX0;
    unsigned char* ld = reinterpret_cast<unsigned char*>(sXb) + ldsD0;
    float4 av0, av1, bv0, bv1;
    if constexpr (BNR) {
      av0 = *reinterpret_cast<const float4*>(sAB + 8 * xq);
      av1 = *reinterpret_cast<const float4*>(sAB + 8 * xq + 4);
      bv0 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq);
      bv1 = *reinterpret_cast<const float4*>(sAB + CI_T + 8 * xq + 4);
    }
    const unsigned good = ~xbad;
    static_for<0, X_ITERS>([&](auto I) {
      constexpr int it = decltype(I)::value;
      if (it < X_FULL || tg + it * GT < Cfg::XH_UNITS) {
        uint4 v = rx[it];
        if constexpr (BNR) {
          auto act = [&](unsigned w, float a_lo, float a_hi, float b_lo, float b_hi) {
            const float lo = __builtin_fmaxf(fmaf(a_lo, e2f_lo(w), b_lo), relu_floor);
            const float hi = __builtin_fmaxf(fmaf(a_hi, e2f_hi(w), b_hi), relu_floor);
            return pack_e2(f32x2{lo, hi});
          };
          v.x = act(v.x, av0.x, av0.y, bv0.x, bv0.y); v.y = act(v.y, av0.z, av0.w, bv0.z, bv0.w);
          v.z = act(v.z, av1.x, av1.y, bv1.x, bv1.y); v.w = act(v.w, av1.z, av1.w, bv1.z, bv1.w);
        }
        if constexpr (MASKED) {
          const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)good, it, 1);
          v.x &= m; v.y &= m; v.z &= m; v.w &= m;
        }
        *reinterpret_cast<uint4*>(lx + it * (16 * RSX * 2)) = v;
      }
    });
    *reinterpret_cast<uint4*>(ld) = rdf0;
    *reinterpret_cast<uint4*>(ld + 32 * RSD * 2) = rdf1;
  };
  auto load_half_any = [&](int pt) __attribute__((always_inline)) {
    if constexpr (FAST) load_half_fast(pt); else load_half(pt);
  };
  auto store_half_any = [&](bf16_t* sXb) __attribute__((always_inline)) {
    if constexpr (FAST) {
      if (xborder) { if (has_bn) store_half_fast(sXb, std::true_type{}, std::true_type{}); else store_half_fast(sXb, std::true_type{}, std::false_type{}); }
      else { if (has_bn) store_half_fast(sXb, std::false_type{}, std::true_type{}); else store_half_fast(sXb, std::false_type{}, std::false_type{}); }
    } else {
      store_half(sXb);
    }
  };
  // x fragments: a ring APD steps ahead of the MFMAs (depths 1-3 measured the same once the first fragments are in flight
  // before the phase starts)
  constexpr int APD = 2, NA = APD + 1;
  static_assert(APD <= 3, "the fragments requested ahead of the barrier must lie in halo row 0");
  frag8_t Af[NA], Bf[4];
  // fragment addresses = one lane base per (buffer, row residue) + an immediate (ds offsets reach 64 KB, a buffer is 62.5 KB:
  // the second buffer gets its own bases; they are opaque to the compiler, which otherwise materialises base + constant
  // per fragment as loop invariants and spills them)
  int aoffp[2][4], boffp[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    aoffp[0][j] = aoff[j];
    aoffp[1][j] = aoff[j] + Cfg::BUF_ELEMS;
    asm volatile("" : "+v"(aoffp[0][j]), "+v"(aoffp[1][j]));
  }
  boffp[0] = boff + NHP * RSX;
  boffp[1] = boff + NHP * RSX + Cfg::BUF_ELEMS;
  asm volatile("" : "+v"(boffp[0]), "+v"(boffp[1]));
  auto loadA = [&](auto Par, auto Sc) __attribute__((always_inline)) {
    constexpr int par = decltype(Par)::value, st = decltype(Sc)::value, hr = st / 3, dx = st % 3, c = hr * HWd + dx;
    const bf16_t* ad = sBuf + aoffp[par][c & 3] + c * RSX;
    Af[st % NA] = tr_frag(ad, ad + 4 * RSX);
  };
  auto loadB = [&](auto Par, auto Rc) __attribute__((always_inline)) {
    constexpr int par = decltype(Par)::value, r = decltype(Rc)::value;
    const bf16_t* bd = sBuf + boffp[par] + r * 16 * RSD;
    Bf[r & 3] = tr_frag(bd, bd + 4 * RSD);
  };
  auto mfma_prefetch = [&](auto Par) __attribute__((always_inline)) {   // row 0 of x and of dy: staged by the other group (see hg)
    wgrad_prefetch<APD>([&](auto Sc) __attribute__((always_inline)) { loadA(Par, Sc); },
                        [&](auto Rc) __attribute__((always_inline)) { loadB(Par, Rc); });
  };
  auto mfma_stage = [&](auto Par) __attribute__((always_inline)) {      // after mfma_prefetch(Par)
    wgrad_walk<PTH, APD>(acc, Af, Bf, [&](auto Sc) __attribute__((always_inline)) { loadA(Par, Sc); },
                         [&](auto Rc) __attribute__((always_inline)) { loadB(Par, Rc); });
  };

  const int pt0 = w.split * P.perSplit;
  const int pt1 = min(P.nPix, pt0 + P.perSplit);
  const int T = pt1 - pt0;
  if (T <= 0) return;       // uniform over the workgroup (cannot happen with the launcher's split)
  bf16_t* buf0 = sBuf;
  bf16_t* buf1 = sBuf + Cfg::BUF_ELEMS;
  __syncthreads();                               // sAB
  load_half_any(pt0);
  store_half_any(buf0);
  load_half_any(min(pt0 + 1, pt1 - 1));
  __syncthreads();                               // stage 0 complete
  if (grp) {                                     // group 1 runs half a stage ahead with its staging
    store_half_any(buf1);
    load_half_any(min(pt0 + 2, pt1 - 1));
    __syncthreads();
  }
  // The loop is unrolled by the buffer parity: with `(n & 1) ? buf1 : buf0` every LDS address of the MFMA phase existed in
  // two variants that hipcc kept in spilled SGPRs and selected at the top of each iteration -- 60 scalar instructions between
  // the barrier and the first fragment read.
  bf16_t* const sbuf0 = grp ? buf0 : buf1;       // where this wave stages while it multiplies an even stage: stage n+1+grp
  bf16_t* const sbuf1 = grp ? buf1 : buf0;
  mfma_prefetch(std::integral_constant<int, 0>{});
  // Barrier of the loop, wg_barrier(): this wave's LDS traffic done (lgkmcnt), then s_barrier.  __syncthreads() also waits with vmcnt(0),
  // i.e. for the loads of stage n+2 that the staging half has just issued -- they are needed one whole interval later (round 4:
  // found with the persistent conv kernel, fu_conv_pp.hip; here the staging interval ended with an HBM latency in it).
  auto body = [&](auto Par, int n) __attribute__((always_inline)) {
    constexpr int par = decltype(Par)::value;
    mfma_stage(Par);
    wg_barrier();
    // stage n+1+grp (already in registers) -> the other buffer of that stage's parity; past the last stage this stores a
    // copy of the last tile into a buffer nobody reads any more (unconditional on purpose: conditional loads become
    // phis that hipcc waits for in front of the MFMA block)
    // (measured and dropped, twice: storing slot by slot with the next tile's load of the same slot issued in between -- the
    //  texture path takes ~45 cycles per 1 KB wave load, 1250 cycles for the eight of a thread -- and a raised s_setprio for
    //  the staging group.  The staging phase shrinks by a third in the stamps; the kernel gets 2-3 % SLOWER, one register
    //  spill included.)
    store_half_any(par ? sbuf1 : sbuf0);
    load_half_any(min(pt0 + n + 2 + grp, pt1 - 1));
    mfma_prefetch(std::integral_constant<int, 1 - par>{});   // (past the last stage: reads of a valid buffer, never used)
    wg_barrier();
  };
  for (int n = 0; n < T; n += 2) {
    body(std::integral_constant<int, 0>{}, n);
    if (n + 1 >= T) break;
    body(std::integral_constant<int, 1>{}, n + 1);
  }
  if (!grp) wg_barrier();                        // group 1's pre-loop barrier

  wgrad_store_slab<9>(P, acc, w, mi, ni, l31, lh);
}

// ------------------------------------------------------------------------------------------------
// wgrad of the network's first conv: 8 input channels (the image bands, no BatchNorm in front), 64 output channels
//
// On the kernels above this layer pads c_in to a 64-row tile: 7 of 8 MFMA rows multiply zeros, 58-60 us against ~30 us
// of traffic (134 MB of dy + 17 MB of x).  With 8 channels a pixel of x is ONE 16-byte vector and the whole 3x3 window
// is M = 72 = 9 taps x 8 channels, so the GEMM is (72 x pixels) . (pixels x 64) and the kernel is a stream over dy:
//   * MFMA 16x16x32, K = one tile row of 32 pixels; M tile j = taps 2j, 2j + 1 (the fifth holds tap 8 twice, its second
//     half is never stored), N tile s = 16 output channels: 5 x 4 accumulator tiles = 80 registers per wave;
//   * the 4 waves split K: wave w multiplies tile rows 2w, 2w + 1 (10 + 8 transposing fragment reads per 20 MFMAs) and
//     the workgroup adds its four partial sums once, at the end, through LDS in a fixed order -- one split-K slab per
//     workgroup, same slab layout as the other kernels (the reduce / transpose passes are shared);
//   * dy goes global -> LDS by LDS-DMA (no staging registers, no ds_write): [pixel][64 channels] rows of 128 bytes, the
//     32-byte segment s of pixel p stored at s ^ (p & 3) ^ ((p >> 3) & 1), which spreads the four (eight) pixels of a
//     ds_read_b64_tr_b16 lane group over all banks; the swizzle is applied on the SOURCE side (a lane of the DMA picks
//     its global address, its LDS slot is fixed);
//   * x ([10][38 px][8 ch]; 38: the one tap pair that straddles two halo rows, (0,2) / (1,0), lands on disjoint banks)
//     passes through two registers per thread, zeroed off the image;
//   * two stages of 38 KB, two workgroups per CU; per tile: wait for the own DMA, store x, ONE barrier, issue the next
//     tile's DMA and loads, multiply.
// Eligible: C_in = 8 from one un-normalised source, C_out = 64, H % 8 = 0, W % 32 = 0 (launch_conv3x3_wgrad_bf16).
// ------------------------------------------------------------------------------------------------
#if FU_HALF
#define FU_MFMA16W(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#else
#define FU_MFMA16W(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#endif
typedef float f32x4w __attribute__((ext_vector_type(4)));

struct WC8 {
  static constexpr int NT = 256, TH = 8, TW = 32, XRS = 38, XROWS = TH + 2, XCOLS = TW + 2;
  static constexpr int X_UNITS = XROWS * XCOLS;              // 340 halo pixels of 16 bytes
  static constexpr int D_BYTES = TH * TW * 128;              // 32768
  static constexpr int X_BYTES = XROWS * XRS * 16;           // 6080
  static constexpr int STAGE = D_BYTES + X_BYTES;            // 38848
  static constexpr int SMEM_BYTES = 2 * STAGE;               // 77696: two workgroups per CU
  static_assert(3 * 20 * 1024 <= SMEM_BYTES, "the final reduction of three waves' accumulators reuses the stages");
};

__global__ __launch_bounds__(256, 2) void k_wgrad_bf16_c8(BWgP P) {
  using C = WC8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int split = blockIdx.x;
  const int pt0 = split * P.perSplit;
  const int pt1 = min(P.nPix, pt0 + P.perSplit);
  const int T = pt1 - pt0;
  if (T <= 0) return;                                        // (uniform; cannot happen with the launcher's split)

  f32x4w acc[5][4];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[j][s] = f32x4w{0.f, 0.f, 0.f, 0.f};

  // fragment addresses (bytes from the stage base): lane 4q + p of k-group g supplies pixel 8g + q (+ 4 in the second
  // read) and "channels" 4p .. 4p + 3 of the 16 rows / columns of the operand tile
  int abase[2][5], bbase[2][4];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int tap = min(2 * j + (p >> 1), 8), ky = tap / 3, kx = tap - 3 * ky;
    abase[0][j] = C::D_BYTES + ((2 * wave + ky) * C::XRS + 8 * g + q + kx) * 16 + 8 * (p & 1);
    abase[1][j] = abase[0][j] + C::STAGE;
    asm volatile("" : "+v"(abase[0][j]), "+v"(abase[1][j]));
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    bbase[0][s] = (2 * wave * C::TW + 8 * g + q) * 128 + ((s ^ q ^ (g & 1)) * 32) + 8 * p;
    bbase[1][s] = bbase[0][s] + C::STAGE;
    asm volatile("" : "+v"(bbase[0][s]), "+v"(bbase[1][s]));
  }

  // dy DMA: wave-instruction i = 8 wave + it covers pixels 8i .. 8i + 7 of the tile (row i >> 2, columns 8 (i & 3) ..),
  // lane = (pixel lane >> 3, 16-byte slot lane & 7); the slot holds source unit 2 ((slot >> 1) ^ sw) + (slot & 1),
  // sw = (pixel & 3) ^ (i & 1)
  unsigned dlane[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int lp = lane >> 3, sl = lane & 7, sw = (lp & 3) ^ par;
    dlane[par] = (unsigned)(lp * 128 + (2 * ((sl >> 1) ^ sw) + (sl & 1)) * 16);
  }
  // x: halo pixel u = tid (+ 256): byte offset from the tile's origin pixel, border membership, LDS address
  int xrel[2], xlds[2];
  unsigned xT = 0, xB = 0, xL = 0, xR = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int u = min(tid + k * C::NT, C::X_UNITS - 1);
    const int hy = u / C::XCOLS, hx = u - hy * C::XCOLS;
    xrel[k] = ((hy - 1) * P.W + (hx - 1)) * 16;
    xlds[k] = C::D_BYTES + (hy * C::XRS + hx) * 16;
    xT |= (hy == 0) ? (1u << k) : 0u;  xB |= (hy == C::XROWS - 1) ? (1u << k) : 0u;
    xL |= (hx == 0) ? (1u << k) : 0u;  xR |= (hx == C::XCOLS - 1) ? (1u << k) : 0u;
  }
  const bool x2 = tid + C::NT < C::X_UNITS;                  // this thread owns a second halo pixel
  const char* xb = reinterpret_cast<const char*>(P.src0);
  const char* db = reinterpret_cast<const char*>(P.dy);
  const unsigned rowB = (unsigned)P.W * 128u;

  uint4 rx0, rx1;
  unsigned xbad = 0;
  auto issue = [&](int pt, int st) __attribute__((always_inline)) {        // pt, st uniform
    const int t2 = fast_div(pt, P.tilesX, P.rcp_tilesX);
    const int tx = pt - t2 * P.tilesX;
    const int bb = fast_div(t2, P.tilesY, P.rcp_tilesY);
    const int y0 = (t2 - bb * P.tilesY) * C::TH, x0 = tx * C::TW;
    const size_t tile_pix = (size_t)((bb * P.H + y0) * P.W + x0);
    const char* dt = db + tile_pix * 128 + (size_t)(2 * wave) * rowB;
    unsigned char* ls = smem_raw + st * C::STAGE + wave * 8192;
    unsigned d0 = dlane[0], d1 = dlane[1];
    asm volatile("" : "+v"(d0), "+v"(d1));                   // (opaque: see fu_conv_rs.hip, hoisted 64-bit lane addresses)
#pragma unroll
    for (int it = 0; it < 8; ++it)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(dt + (size_t)(it >> 2) * rowB + (size_t)((it & 3) * 1024) + (size_t)((it & 1) ? d1 : d0)),
          (__attribute__((address_space(3))) void*)(ls + it * 1024), 16, 0, 0);
    const unsigned ft = y0 == 0 ? ~0u : 0u, fb = y0 + C::TH == P.H ? ~0u : 0u;
    const unsigned fl = x0 == 0 ? ~0u : 0u, fr = x0 + C::TW == P.W ? ~0u : 0u;
    xbad = (xT & ft) | (xB & fb) | (xL & fl) | (xR & fr);
    const char* xt = xb + tile_pix * 16;
    rx0 = *reinterpret_cast<const uint4*>(xt + ((xbad & 1u) ? 0 : xrel[0]));   // off the image: the origin pixel, zeroed below
    rx1 = *reinterpret_cast<const uint4*>(xt + ((xbad & 2u) ? 0 : xrel[1]));
  };
  auto store_x = [&](int st) __attribute__((always_inline)) {
    const unsigned m0 = (xbad & 1u) ? 0u : ~0u, m1 = (xbad & 2u) ? 0u : ~0u;
    uint4 v0 = rx0, v1 = rx1;
    v0.x &= m0; v0.y &= m0; v0.z &= m0; v0.w &= m0;
    v1.x &= m1; v1.y &= m1; v1.z &= m1; v1.w &= m1;
    *reinterpret_cast<uint4*>(smem_raw + st * C::STAGE + xlds[0]) = v0;
    if (x2) *reinterpret_cast<uint4*>(smem_raw + st * C::STAGE + xlds[1]) = v1;
  };
  // the fragments of both tile rows of this wave are requested BEFORE the next tile's DMA is issued and multiplied after it:
  // hipcc orders every LDS read behind an outstanding LDS-DMA (s_waitcnt vmcnt) -- reads that follow the issue in program
  // order would wait for the tile that has just been requested
  frag8_t Bf[2][4], Af[2][5];
  auto read_frags = [&](auto Par) __attribute__((always_inline)) {
    constexpr int par = decltype(Par)::value;
    static_for<0, 2>([&](auto RR) {
      constexpr int rr = decltype(RR)::value;
      static_for<0, 4>([&](auto S) {
        constexpr int s = decltype(S)::value;
        const bf16_t* bd = reinterpret_cast<const bf16_t*>(smem_raw + bbase[par][s] + rr * (C::TW * 128));
        Bf[rr][s] = tr_frag(bd, bd + 4 * 64);
      });
      static_for<0, 5>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const bf16_t* ad = reinterpret_cast<const bf16_t*>(smem_raw + abase[par][j] + rr * (C::XRS * 16));
        Af[rr][j] = tr_frag(ad, ad + 4 * 8);
      });
    });
  };
  auto multiply = [&]() __attribute__((always_inline)) {
    static_for<0, 2>([&](auto RR) {
      constexpr int rr = decltype(RR)::value;
      static_for<0, 5>([&](auto J) {
        constexpr int j = decltype(J)::value;
        static_for<0, 4>([&](auto S) {
          constexpr int s = decltype(S)::value;
          acc[j][s] = FU_MFMA16W(Af[rr][j], Bf[rr][s], acc[j][s]);
        });
      });
    });
  };
  auto body = [&](auto Par, int n) __attribute__((always_inline)) {
    constexpr int par = decltype(Par)::value;
    __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));    // vmcnt(0): this lane's share of stage n (the builtin, so that hipcc knows the DMA has landed)
    store_x(par);
    wg_barrier();                                            // stage n complete; everybody is done with stage n - 1
    read_frags(Par);
    __builtin_amdgcn_sched_barrier(0);
    issue(pt0 + min(n + 1, T - 1), 1 - par);                 // (past the last tile: the last tile again, never read)
    __builtin_amdgcn_sched_barrier(0);
    multiply();
  };
  issue(pt0, 0);
  for (int n = 0; n < T; n += 2) {
    body(std::integral_constant<int, 0>{}, n);
    if (n + 1 >= T) break;
    body(std::integral_constant<int, 1>{}, n + 1);
  }
  __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));      // the trailing DMA writes LDS: it must have landed before the reuse
  wg_barrier();

  // waves 1-3 park their partial sums, wave 0 adds them in wave order and writes the workgroup's slab
  float* red = reinterpret_cast<float*>(smem_raw);
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        *reinterpret_cast<f32x4w*>(red + (((wave - 1) * 20 + j * 4 + s) * 64 + lane) * 4) = acc[j][s];
  }
  wg_barrier();
  if (wave == 0) {
    // D tile: lane = column (output channel 16 s + lane % 16), registers = rows 4 g + i = tap 2j + (g >> 1), channels
    // 4 (g & 1) + i  ->  slab[split][tap][c_in / 4][c_out][4]: one 16-byte store per accumulator tile
    const int co = lane & 15;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int tap = 2 * j + (g >> 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        f32x4w v = acc[j][s];
#pragma unroll
        for (int w = 0; w < 3; ++w) v += *reinterpret_cast<const f32x4w*>(red + ((w * 20 + j * 4 + s) * 64 + lane) * 4);
        if (tap < 9)
          *reinterpret_cast<f32x4w*>(P.slab + ((((int64_t)split * 9 + tap) * 2 + (g & 1)) * 64 + 16 * s + co) * 4) = v;
      }
    }
  }
}

static bool wgrad_c8_eligible(const BWgP& P) {
  const int64_t npx = (int64_t)P.B * P.H * P.W;
  return P.C0 == 8 && P.C1 == 0 && P.a0 == nullptr && P.Cout == 64 && P.H % WC8::TH == 0 && P.W % WC8::TW == 0 &&
         npx * 128 < (int64_t(1) << 40) && npx < (int64_t(1) << 31);
}

// one launch per route on the grid conv3x3_wgrad_plan laid out: (c_in tile, c_out tile, split) workgroups
template <auto Kernel, typename Cfg>
static int launch_wgrad(const BWgP& P, const LaunchOpts& o, hipStream_t s) {
  return launch_conv_kernel<Kernel>(dim3(P.nCi * P.nCo * P.S), dim3(Cfg::NT), Cfg::SMEM_BYTES, o, s, P);
}

static int launch_wgrad_pp(const BWgP& P, const LaunchOpts& o, hipStream_t s) {
  using Cfg = WPCfg;
  // whole pixel tiles, whole channel tiles, 24-bit pixel indices and pixel strides, 32-bit byte offsets inside a source
  const int64_t npx = (int64_t)P.B * P.H * P.W;
  const int cmax = P.C0 > P.C1 ? P.C0 : P.C1;
  const bool fast = g_conv_hooks.wgrad_lockstep != 2 && P.H % Cfg::PTH == 0 && P.W % Cfg::PTW == 0 && P.Cin % Cfg::CI_T == 0 &&
                    P.Cout % Cfg::CO_T == 0 && npx < (1 << 24) && npx * cmax * 2 < (int64_t(1) << 32) &&
                    npx * P.Cout * 2 < (int64_t(1) << 32) && (int64_t)P.nPix * P.nCi * P.nCo < (int64_t(1) << 31);
  return fast ? launch_wgrad<k_wgrad_bf16_pp<true>, Cfg>(P, o, s) : launch_wgrad<k_wgrad_bf16_pp<false>, Cfg>(P, o, s);
}

// Workgroups of the ping-pong kernel.  Its 8-wave workgroups (248 registers, 125 KB of LDS) take a CU each and live for the
// whole launch (45-290 us).  At 256 of them -- one per CU, round 2 -- every kernel of the main backward chain that starts while
// a weight-gradient launch is in flight (BatchNorm-backward finalize / apply, bilinear backward, the next dgrad) waits for
// those workgroups to retire before it gets a single CU: in the two-stream trace the 36 finalize launches took 494 us against
// 190 alone, the four bilinear backwards 525 against 105 (profiles/r3_*).  Launching FEWER, longer workgroups leaves CUs to
// the critical chain from the first cycle, and the split-K slabs shrink with the workgroup count (75 -> 52 MB written and
// re-read per layer).  Measured, same box, ms per step | conv class TFLOP/s event-timed in the step: 256: 5.74 / 5.75 | 835 /
// 856, 208: 5.61 / 5.64 | 830 / 827, 192: 5.58 / 5.61 | 790 / 790, 176: 5.59 / 5.61 | 793 / 789, 160: 5.56 / 5.57 | 780 / 790,
// 128: 5.67 (another box, against 5.78 at 256).  Below 208 the step gains another 0.5 % while the dgrad launches -- which then
// share the GPU with the longer-running weight-gradient launch of the layer before -- lose 5 %: 208 takes most of the one
// without the other.
// Round 4: 160.  The persistent conv kernel (fu_conv_pp.hip) takes a whole CU per workgroup like this one, so a dgrad launch that
// starts beside a weight-gradient launch runs on the CUs this kernel leaves and the rest of its grid waits; measured again with
// that dispatch, two boxes, ms per step | conv class TFLOP/s event-timed in the step: 256: 5.60 | 913, 208: 5.40-5.47 | 890-922,
// 192: 5.34-5.39 | 853-866, 176: 5.33-5.40 | 848-867, 160: 5.28-5.35 | 834-843, 144: 5.38 | 825, 128: 5.57 | 825 -- the step is the
// product's metric (-1.8 % at 160); the conv launches' event-timed rate falls with it by construction (they share more of their
// own duration), their rate with the GPU to themselves (roofline.achieved_serial) does not change.  Capping the dgrad launches'
// grid to the complement instead (128 + 128, 112 + 144, 96 + 160) is no better (5.35-5.40) and slower alone.
static constexpr int WGRAD_PP_TARGET = 160;
// ... of the narrow launches: the 8-band first conv and k_wgrad_bf16<2,8> (256 threads, two workgroups per CU)
static constexpr int WGRAD_C64_TARGET = 512;
// ... of the one-tap launches (embedded 1x1): one 8-wave workgroup per CU, or two 4-wave ones
static constexpr int WGRAD_TAP1_WIDE_TARGET = 256, WGRAD_TAP1_NARROW_TARGET = 512;

WgradRoute conv3x3_wgrad_route(const BWgP& P, bool one_tap, const ConvHooks& h) {
  // embedded 1x1 (late-fusion convs): the stage is all staging, so the lock-step kernel (all 8 waves stage together) wins
  // over the ping-pong one; the eight unwritten tap slabs reach only taps of dw_oihw that the caller never reads
  if (one_tap) return P.Cin > 64 ? WGRAD_TAP1_WIDE : WGRAD_TAP1_NARROW;
  if (!h.wgrad_lockstep && wgrad_c8_eligible(P)) return WGRAD_C8;   // the 8-band first conv: K = 72 stream over dy
  // 512 threads, 128 c_in x 64 c_out, one WG per CU: the ping-pong kernel, or the lock-step one on the same split
  // (bit-identical sums); 256 threads, 64 x 64, two WGs per CU below
  if (P.Cin > 64) return h.wgrad_lockstep != 1 ? WGRAD_PP : WGRAD_LOCKSTEP_128;
  return WGRAD_LOCKSTEP_64;
}

void conv3x3_wgrad_plan(BWgP& P, WgradRoute r) {
  switch (r) {
    case WGRAD_TAP1_WIDE: wgrad_geometry(P, WCfg<4, 8>::PTW, 8, WCfg<4, 8>::CI_T, WGRAD_TAP1_WIDE_TARGET); break;
    case WGRAD_TAP1_NARROW: wgrad_geometry(P, WCfg<2, 8>::PTW, 8, WCfg<2, 8>::CI_T, WGRAD_TAP1_NARROW_TARGET); break;
    case WGRAD_C8: wgrad_geometry(P, WC8::TW, WC8::TH, 8, WGRAD_C64_TARGET); break;   // one tile of its 8 c_in x 64 c_out
    case WGRAD_PP: wgrad_geometry(P, WPCfg::PTW, WPCfg::PTH, WPCfg::CI_T, WGRAD_PP_TARGET); break;
    case WGRAD_LOCKSTEP_128: wgrad_geometry(P, WCfg<4, 8>::PTW, 8, WCfg<4, 8>::CI_T, WGRAD_PP_TARGET); break;
    case WGRAD_LOCKSTEP_64: wgrad_geometry(P, WCfg<2, 8>::PTW, 8, WCfg<2, 8>::CI_T, WGRAD_C64_TARGET); break;
    case WGRAD_NUM_ROUTES: break;
  }
}

// upper bound of the slab size over every plan above: the largest workgroup target of the 128- and of the 64-c_in tiles
// on 8x16-pixel stages (the 8-band kernel's 8x32 tiles give no more splits), one slab to spare
int64_t conv3x3_wgrad_slab_elems_bf16(int Cin, int Cout, int B, int H, int W) {
  constexpr int T128 = std::max(WGRAD_PP_TARGET, WGRAD_TAP1_WIDE_TARGET), T64 = std::max(WGRAD_C64_TARGET, WGRAD_TAP1_NARROW_TARGET);
  const int64_t npix = (int64_t)B * ceil_div(H, WPCfg::PTH) * ceil_div(W, WPCfg::PTW);
  const int nT128 = ceil_div(Cin, WCfg<4, 8>::CI_T) * ceil_div(Cout, 64);
  const int nT64 = ceil_div(Cin, WCfg<2, 8>::CI_T) * ceil_div(Cout, 64);
  const int64_t smax = std::min<int64_t>(std::max(ceil_div(T128, nT128), ceil_div(T64, nT64)), npix);
  return (smax + 1) * 9 * (int64_t)Cin * Cout;
}

int launch_conv3x3_wgrad_bf16(const ConvIn& in, const bf16_t* dy, int Cout, float* slab, float* dw_oihw, int cin_real,
                              const float* db_partials, int n_db_partials, float* db, int B, int H, int W,
                              hipStream_t s) {
  BWgP P;
  P.src0 = (const bf16_t*)in.src0; P.src1 = (const bf16_t*)in.src1; P.a0 = in.a0; P.b0 = in.b0; P.dy = dy;
  P.slab = slab;
  P.C0 = in.C0; P.C1 = in.src1 ? in.C1 : 0; P.Cin = P.C0 + P.C1; P.Cout = Cout; P.B = B; P.H = H; P.W = W;
  FU_REQUIRE(P.C0 % 8 == 0 && P.C1 % 8 == 0 && Cout % 8 == 0, "wgrad_bf16: channel counts must be multiples of 8");
  const WgradRoute r = conv3x3_wgrad_route(P, in.center_only && !g_conv_hooks.full_taps, g_conv_hooks);
  conv3x3_wgrad_plan(P, r);
  int st = 1;
  switch (r) {
    case WGRAD_TAP1_WIDE: st = launch_wgrad<k_wgrad_bf16<4, 8, 1>, WCfg<4, 8>>(P, in.opt, s); break;
    case WGRAD_TAP1_NARROW: st = launch_wgrad<k_wgrad_bf16<2, 8, 1>, WCfg<2, 8>>(P, in.opt, s); break;
    case WGRAD_C8: st = launch_wgrad<k_wgrad_bf16_c8, WC8>(P, in.opt, s); break;
    case WGRAD_PP: st = launch_wgrad_pp(P, in.opt, s); break;
    case WGRAD_LOCKSTEP_128: st = launch_wgrad<k_wgrad_bf16<4, 8>, WCfg<4, 8>>(P, in.opt, s); break;
    case WGRAD_LOCKSTEP_64: st = launch_wgrad<k_wgrad_bf16<2, 8>, WCfg<2, 8>>(P, in.opt, s); break;
    case WGRAD_NUM_ROUTES: break;
  }
  if (st) return st;
  return launch_wgrad_reduce_oihw(slab, P.S, P.Cin, Cout, cin_real, dw_oihw, db_partials, n_db_partials, db, in.opt.unscale, s);
}

}  // namespace fu
