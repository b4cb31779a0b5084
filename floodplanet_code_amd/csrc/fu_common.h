// Shared declarations for libfloodunet (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "fu_device_slots.h"

// host tables of include/floodunet.h that the launchers below validate
struct fu_stitch_entry;
struct fu_scene_crop;
struct fu_scene_train_entry;
struct fu_scene_aug;
struct fu_class_threshold;
struct fu_mask_box;
struct fu_tiff_layout;

namespace fu {

typedef unsigned short bf16_t;  // raw bf16 storage
struct f16_t { unsigned short v; };   // raw IEEE fp16 storage (a distinct type, so that the kernels can be instantiated on it)

// PREC_F16: fp16 activations / weights / gradient maps on the matrix cores (v_mfma_f32_32x32x16_f16, the bf16 rate), fp32
// accumulation, statistics, loss and master weights; the gradient maps carry a power-of-two loss scale (see LossScale).
enum Prec { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2 };

// The one place that maps a Prec to an element type: f(T{}) with T = the element type of p.  The launchers pass a generic
// lambda (`using T = decltype(tag)`); FU_REQUIRE / FU_LAUNCH_CHECK inside it return from the lambda, so such a lambda
// returns the status (int) and the caller returns or FU_TRYs the call's result.
template <typename F> auto dispatch_prec(Prec p, F&& f) {
  if (p == PREC_F32) return f(float{});
  if (p == PREC_BF16) return f(bf16_t{});
  return f(f16_t{});
}

// ---- error plumbing (thread-local message, never exceptions across the ABI) ----------------
void set_error(const char* fmt, ...);
const char* get_error();

#define FU_HIP_CHECK(expr)                                                                   \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      ::fu::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return 2;                                                                              \
    }                                                                                        \
  } while (0)

#define FU_LAUNCH_CHECK()                                                       \
  do {                                                                          \
    hipError_t _e = hipGetLastError();                                          \
    if (_e != hipSuccess) {                                                     \
      ::fu::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
      return 2;                                                                 \
    }                                                                           \
  } while (0)

#define FU_REQUIRE(cond, ...)          \
  do {                                 \
    if (!(cond)) {                     \
      ::fu::set_error(__VA_ARGS__);    \
      return 1;                        \
    }                                  \
  } while (0)

#define FU_TRY(expr)           \
  do {                         \
    int _s = (expr);           \
    if (_s != 0) return _s;    \
  } while (0)

__host__ __device__ static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
static inline unsigned host_rcp(int d) { return d <= 1 ? 0u : (unsigned)((((unsigned long long)1) << 32) / (unsigned)d + 1); }
// blocks of a grid-stride launch: ceil(work / block), clamped to [1, cap]
static inline int grid_for(int64_t work, int block, int cap = 8192) {
  int64_t g = ceil_div64(work, block);
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// ---- device helpers -------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
  return __builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ float h2f(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }   // v_cvt_f32_f16
__device__ __forceinline__ unsigned short f2h(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }  // RNE
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_h2(float a, float b) {     // two floats -> packed fp16 pair (RNE)
  const float2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, half2_t));
}
__device__ __forceinline__ void unpack_h2(unsigned u, float& a, float& b) {
  const float2_t v = __builtin_convertvector(__builtin_bit_cast(half2_t, u), float2_t);
  a = v.x; b = v.y;
}

template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
  static constexpr int VEC = 4;  // elements per 16-byte access
  __device__ static __forceinline__ void load4(const float* p, float (&v)[4]) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ static __forceinline__ void store4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __device__ static __forceinline__ float load1(const float* p) { return *p; }
  __device__ static __forceinline__ void store1(float* p, float v) { *p = v; }
};
template <> struct ElemIO<bf16_t> {
  static constexpr int VEC = 8;
  __device__ static __forceinline__ void load4(const bf16_t* p, float (&v)[4]) {
    uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
  }
  __device__ static __forceinline__ void store4(bf16_t* p, const float (&v)[4]) {
    uint2 t;
    t.x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
    t.y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = t;
  }
  __device__ static __forceinline__ float load1(const bf16_t* p) { return bf2f(*p); }
  __device__ static __forceinline__ void store1(bf16_t* p, float v) { *p = f2bf(v); }
};

template <> struct ElemIO<f16_t> {
  static constexpr int VEC = 8;
  __device__ static __forceinline__ void load4(const f16_t* p, float (&v)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    unpack_h2(t.x, v[0], v[1]); unpack_h2(t.y, v[2], v[3]);
  }
  __device__ static __forceinline__ void store4(f16_t* p, const float (&v)[4]) {
    uint2 t;
    t.x = pack_h2(v[0], v[1]); t.y = pack_h2(v[2], v[3]);
    *reinterpret_cast<uint2*>(p) = t;
  }
  __device__ static __forceinline__ float load1(const f16_t* p) { return h2f(p->v); }
  __device__ static __forceinline__ void store1(f16_t* p, float v) { p->v = f2h(v); }
};

// The activation every consumer re-derives from a stored pre-BN value y: relu(a*y + b), with a = gamma*invstd and
// b = beta - mean*a.  ATen's CPU batch_norm (what the reference runs, and what the golden fixtures were made with)
// forms exactly these two coefficients and evaluates x*alpha + beta as a multiply and a separate add, so the parity
// definition is TWO roundings, never an fma: with it the activations are bit-identical to torch's given identical
// y / mean / invstd, and ReLU / max-pool near-ties fall the same way (measured: with an fma here the worst gradient
// tensor of the 300x300 fixture moved from 0.6 % to 1.2 % off the reference).  The bf16 conv staging rounds the
// result to bf16 anyway and uses the fused form (bn_act_fused).
__device__ __forceinline__ float bn_act_pre(float a, float y, float b) {
#pragma clang fp contract(off)   // (HIP's __fmul_rn / __fadd_rn are plain operators and DO get fused under -ffp-contract=fast)
  const float p = a * y;
  return p + b;
}
__device__ __forceinline__ float bn_act(float a, float y, float b) { return fmaxf(bn_act_pre(a, y, b), 0.f); }
__device__ __forceinline__ float bn_act_fused(float a, float y, float b) { return fmaxf(fmaf(a, y, b), 0.f); }

// 16-byte vector access: V elements of T as floats (V = 4 for fp32, 8 for bf16 and fp16)
template <typename T> struct VecIO;
template <> struct VecIO<float> {
  static constexpr int V = 4;
  __device__ static __forceinline__ void load(const float* p, float (&v)[4]) { ElemIO<float>::load4(p, v); }
  __device__ static __forceinline__ void store(float* p, const float (&v)[4]) { ElemIO<float>::store4(p, v); }
};
template <> struct VecIO<bf16_t> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u);
    v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
  }
  __device__ static __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
    uint4 t;
    t.x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
    t.y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
    t.z = (unsigned)f2bf(v[4]) | ((unsigned)f2bf(v[5]) << 16);
    t.w = (unsigned)f2bf(v[6]) | ((unsigned)f2bf(v[7]) << 16);
    *reinterpret_cast<uint4*>(p) = t;
  }
};

template <> struct VecIO<f16_t> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const f16_t* p, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    unpack_h2(t.x, v[0], v[1]); unpack_h2(t.y, v[2], v[3]); unpack_h2(t.z, v[4], v[5]); unpack_h2(t.w, v[6], v[7]);
  }
  __device__ static __forceinline__ void store(f16_t* p, const float (&v)[8]) {
    uint4 t;
    t.x = pack_h2(v[0], v[1]); t.y = pack_h2(v[2], v[3]); t.z = pack_h2(v[4], v[5]); t.w = pack_h2(v[6], v[7]);
    *reinterpret_cast<uint4*>(p) = t;
  }
};

// n / d for n * d < 2^32 with rcp = floor(2^32 / d) + 1 made on the host (0 encodes d == 1)
__device__ __forceinline__ int fast_div(int n, int d, unsigned rcp) {
  (void)d;
  return rcp ? (int)__umulhi((unsigned)n, rcp) : n;
}

// XCD-aware bijective remap of a linear block id: blocks b and b+8 share an XCD (observed round
// robin), so give each XCD a contiguous chunk of the logical id space (speed only, never correctness).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// Test-time-augmentation view codes (1 = flip(-1), 2 = flip(-2), 4 = transpose, applied in the order transpose, flip(-1),
// flip(-2)): view_src_pixel maps a pixel of the view to the pixel of the image it shows, view_dst_pixel the other way
// round (the inverse view).
__device__ __forceinline__ int view_src_pixel(int code, int y, int x, int H, int W) {
  if (code & 2) y = H - 1 - y;
  if (code & 1) x = W - 1 - x;
  return (code & 4) ? x * W + y : y * W + x;
}
__device__ __forceinline__ int view_dst_pixel(int code, int y, int x, int H, int W) {
  if (code & 4) { const int t = y; y = x; x = t; }
  if (code & 1) x = W - 1 - x;
  if (code & 2) y = H - 1 - y;
  return y * W + x;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
#endif  // __HIPCC__

// Optional event pair recorded immediately around the main kernel of ONE conv / wgrad launch (LaunchOpts::prof: filled by
// the API layer from the context's profiler when profiling is on; per launch, never process-wide state).
struct ProfSlot { hipEvent_t start = nullptr; hipEvent_t stop = nullptr; };

// Exact data-parallel mode (fu_set_exact_sync): at every statistics reduction the partial sums are summed over the
// ranks before they are finalised.  The four launchers with such a reduction (BN forward statistics, BN backward sums,
// CE loss sums, region-term sums) take the descriptor as an argument, null = off; the step code gets it from
// active_sync (fu_ctx.h), once per call.
struct SyncDesc {
  int (*hook)(void* user, int64_t n_elems, int is_double) = nullptr;   // sums xbuf[0..n) over the ranks, in place
  void* user = nullptr;
  void* xbuf = nullptr;        // caller-owned device exchange buffer
  int64_t xbytes = 0;
  int world = 1;
};
static inline int sync_world(const SyncDesc* d) { return (d && d->hook) ? d->world : 1; }
// payload (device, n elements of float or double) -> xbuf, hook, back; no-op where sync_world(d) is 1
int sync_sum_over_ranks(const SyncDesc* d, void* payload, int64_t n_elems, bool is_double, hipStream_t s);

// fp16 mode: the gradient maps (fp16) carry a power-of-two loss scale S chosen on the device from max|dL/dlogits| at the
// start of every backward (launch_loss_grad_eff).  scale[0] = S, scale[1] = 1/S.  The places that write PARAMETER
// gradients (weight-gradient reduce + bias tail, BN backward finalize, head backward finalize, the ConvTranspose bias sum)
// multiply by 1/S, so the flat gradient buffer always holds true gradients.  Each of them takes the pointer to 1/S with its
// launch (LaunchOpts::unscale, BnBwdArgs::unscale, an argument); nullptr (fp32 / bf16) means 1.  The backward gets it from
// grad_unscale (fu_ctx.h).

// BatchNorm-backward sums from the PRODUCER of dL/dz (round 2): a dgrad launch whose single destination g = dL/d relu(bn(y))
// feeds a BatchNorm backward can emit that backward's two sums (sum g*m, sum g*m*xhat, m = [a*y + b > 0]) per workgroup
// tile from its epilogue, where g is still in registers -- k_bn_bwd_reduce (one read of g and one of y, 14 launches per
// step) then disappears for that layer.  The API layer passes this request with the launch (ConvIn::opt.bnb);
// a kernel that honours it (the row-stationary 16-bit kernel, single destination, <= max_tiles workgroup tiles) writes
// part[tile][channel][2] and *tiles_out = number of tiles; everything else leaves *tiles_out untouched (0 = not fused).
struct BnbFuse {
  const void* y = nullptr;                 // raw conv output of the BatchNorm, NHWC, the destination's shape
  const float *a = nullptr, *b = nullptr, *mean = nullptr, *invstd = nullptr;
  float* part = nullptr;
  int64_t max_elems = 0;                   // capacity of part (floats)
  int* tiles_out = nullptr;
  bool skip_g = false;                     // head backward only: g itself is not stored (HeadGrad below recomputes it)
};
static inline BnbFuse bnb_fuse(const void* y, const float* a, const float* b, const float* mean, const float* invstd,
                               float* part, int64_t cap, int* tiles_out) {
  BnbFuse f;
  f.y = y; f.a = a; f.b = b; f.mean = mean; f.invstd = invstd;
  f.part = part; f.max_elems = cap; f.tiles_out = tiles_out;
  return f;
}
// The head's data gradient g[p][c] = sum_k dl[p][k] w[k][c] is two or three FMAs per element: when the head backward has
// left the BatchNorm-backward sums of g behind (BnbFuse), the apply pass of that BatchNorm recomputes g from dl and w
// instead of reading a stored copy -- one 134 MB write and one 134 MB read less per step at the bench shape.
struct HeadGrad {
  const float* dl = nullptr;               // dL/dlogits, NHWC fp32 [npix][ncls]
  const float* w = nullptr;                // head weight [ncls][C]
  int ncls = 0;
};
// per-launch options of the conv / wgrad launchers (host side only; travels inside ConvIn)
struct LaunchOpts {
  ProfSlot prof;                  // events around the main kernel
  const BnbFuse* bnb = nullptr;   // dgrad launches: request for the destination BatchNorm's backward sums
  const float* unscale = nullptr; // wgrad launches, fp16: device 1 / loss scale, applied where dw / db are written (null = 1)
};

// Per-device launch facts.  Both are kept per device index in a DeviceSlots (fu_device_slots.h: DeviceSlots::CAP indices,
// filled once each from whichever host thread comes first; an index beyond asks the runtime every time), so no launch
// depends on which device launched first, and a launch after the first on its device costs one hipGetDevice.
// The CU count of the current device (the grid of the persistent conv kernel); *n_cu > 0 on success.
inline int current_device_cus(int* n_cu) {
  static DeviceSlots cus;
  int dev = 0;
  FU_HIP_CHECK(hipGetDevice(&dev));
  *n_cu = cus.get(dev, [dev] {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n > 0 ? n : 256;
  });
  FU_REQUIRE(*n_cu > 0, "the CU count of device %d is not available", dev);
  return 0;
}
#ifdef __HIPCC__
// The one way a conv / wgrad main kernel is launched: the opt-in to more dynamic LDS once per kernel AND device, the launch's
// event pair immediately around the kernel, the launch check.  The opt-in is made from 48 KiB on: the fp32 kernels (44 - 48 KiB)
// never made it, the 16-bit launchers made it for every kernel, the 36 KiB one-tap tile included, which does not need it.
// (A kernel launches with one LDS size, so the first launch's size serves the later ones.)
template <auto Kernel, typename P>
int launch_conv_kernel(dim3 grid, dim3 block, size_t smem, const LaunchOpts& o, hipStream_t s, const P& p) {
  if (smem > 48 * 1024) {
    static DeviceSlots opted;   // of this kernel: what the opt-in returned on each device
    int dev = 0;
    FU_HIP_CHECK(hipGetDevice(&dev));
    const hipError_t opt_in = (hipError_t)opted.get(dev, [smem] {
      return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)smem);
    });
    FU_HIP_CHECK(opt_in);
  }
  if (o.prof.start) (void)hipEventRecord(o.prof.start, s);
  hipLaunchKernelGGL(Kernel, grid, block, smem, s, p);
  if (o.prof.stop) (void)hipEventRecord(o.prof.stop, s);
  FU_LAUNCH_CHECK();
  return 0;
}
#endif
// out = dlogits * (*up_scale_dev or 1) * (S or 1); scale != null (fp16): S chosen from max|dlogits * up| and written to scale[0..1]
int launch_loss_grad_eff(const float* dlogits, float* out, int64_t n, const float* up_scale_dev,
                         float* partials /* >= 256 floats */, float* scale /* [2] or null */, hipStream_t s,
                         const int* guard = nullptr /* fp16 guard words: [2] = back-off exponent */);

// A library-owned device copy of a small host table that an entry point rebuilds on every call (fu_stitch_add_batch,
// fu_scene_crops, fu_scene_train_tiles: one table each, in the context).  The buffer is reused from call to call, so the
// calls that share a table must be ordered on ONE stream: a call on another stream would overwrite the table under a
// launch that still reads it (include/floodunet.h says so for each entry point).
struct DeviceTable {
  void* dev = nullptr;
  size_t cap = 0;              // bytes
  // host[0 .. bytes) -> dev, ordered on s; grows to at least 64 entries of entry_bytes
  int upload(const void* host, size_t bytes, size_t entry_bytes, hipStream_t s) {
    if (bytes > cap) {
      if (dev) {
        FU_HIP_CHECK(hipDeviceSynchronize());     // an earlier launch may still read the old table
        FU_HIP_CHECK(hipFree(dev));
        dev = nullptr;
        cap = 0;
      }
      const size_t want = bytes > 64 * entry_bytes ? bytes : 64 * entry_bytes;
      FU_HIP_CHECK(hipMalloc(&dev, want));
      cap = want;
    }
    FU_HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  void release() {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
    cap = 0;
  }
};

// ---- kernel launchers (implemented in the .hip files) ----------------------------------------
// All pointers are device pointers; T-typed buffers are `void*` + Prec.

struct ConvIn {              // the (virtual) input of a 3x3 convolution
  const void* src0; int C0;  // first C0 channels (skip / plain input)
  const float* a0;           // optional BN scale for src0: x = relu(a0*src0 + b0)
  const float* b0;
  const void* src1; int C1;  // next C1 channels, taken as they are (may be null/0)
  bool center_only = false;  // the packed weights are a 1x1 conv embedded as the centre tap (late-fusion convs)
  LaunchOpts opt;            // events / fused-sum request of this launch
};

// conv as implicit GEMM: out[p][n] = sum_{tap,c} in[p+tap][c] * wpk[tap][c][n] (+bias[n])
// wpk layout is precision specific (see the pack kernels).  Output channels [0,D0) -> dst0, [D0,D0+D1) -> dst1.
// stats: optional [nStatTiles][N][2] partial (sum, sumsq) of the bias-free result per pixel tile;
// *n_stat_tiles receives the number of tiles written (<= conv3x3_num_stat_tiles()).
int conv3x3_num_stat_tiles(Prec p, int B, int H, int W);
int launch_conv3x3(Prec p, const ConvIn& in, const void* wpk, const float* bias, void* dst0, int D0, void* dst1,
                   int D1, float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s);
// dW partial slabs + fixed-order reduce into fp32 OIHW (+ bias gradient from db_partials [n][Cout]).
int64_t conv3x3_wgrad_slab_elems(Prec p, int Cin, int Cout, int B, int H, int W);
int launch_conv3x3_wgrad(Prec p, const ConvIn& in, const void* dy, int Cout, float* slab, float* dw_oihw,
                         int cin_real, const float* db_partials, int n_db_partials, float* db, int B, int H,
                         int W, hipStream_t s);

// weight packing: fp32 OIHW [Cout][cin_real][3][3] -> fwd pack (GEMM K = cin padded to cin_pad, N = Cout)
// and dgrad pack (taps reversed, K = Cout, N = cin_pad).  Either destination may be null.
int64_t conv3x3_pack_elems(Prec p, int cin_pad, int Cout);
int launch_pack_conv3x3(Prec p, const float* w_oihw, int Cout, int cin_real, int cin_pad, void* wfwd, void* wdgrad,
                        hipStream_t s);

// the tail of every weight-gradient launch (fu_conv.hip): S split-K slabs -> dw (fp32 OIHW) and db, in a fixed order.
// fp32 path: [tap][ci][co] slabs; 16-bit paths: [tap][ci / 4][co][4] slabs.  unscale: LaunchOpts::unscale of the launch
int launch_wgrad_reduce(const float* slab, int S, int Cin, int Cout, int cin_real, float* dw, const float* dbp, int ndb,
                        float* db, const float* unscale, hipStream_t s);
int launch_wgrad_reduce_oihw(const float* slab, int S, int Cin, int Cout, int cin_real, float* dw, const float* dbp,
                             int ndb, float* db, const float* unscale, hipStream_t s);
// the split-K plan of the fp32 weight-gradient kernel (fu_conv_f32.hip, in its tile sizes)
void wgrad_split_shared(int Cin, int Cout, int B, int H, int W, int* nPix, int* S, int* perSplit);

// precision-specific implementations (fu_conv_f32.hip / fu_conv_bf16.hip; the 16-bit weight gradient: fu_wgrad_bf16.hip)
int conv3x3_num_stat_tiles_f32(int B, int H, int W);
int conv3x3_f32_tile_rows(int B, int H, int W, int N);   // the TH instantiation of k_conv3x3_f32 a launch of this shape runs (8 or 4)
bool test_op_center_only();                              // fu_test_op_center_only (fu_conv.hip)
int launch_conv3x3_f32(const ConvIn& in, const float* wpk, const float* bias, float* dst0, int D0, float* dst1, int D1,
                       float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s);
int64_t conv3x3_wgrad_slab_elems_f32(int Cin, int Cout, int B, int H, int W);
int launch_conv3x3_wgrad_f32(const ConvIn& in, const float* dy, int Cout, float* slab, float* dw_oihw, int cin_real,
                             const float* db_partials, int n_db_partials, float* db, int B, int H, int W,
                             hipStream_t s);
int launch_pack_conv3x3_f32(const float* w_oihw, int Cout, int cin_real, int cin_pad, float* wfwd, float* wdgrad,
                            hipStream_t s);
int conv3x3_num_stat_tiles_bf16(int B, int H, int W);
int64_t conv3x3_wgrad_slab_elems_bf16(int Cin, int Cout, int B, int H, int W);
int launch_conv3x3_bf16(const ConvIn& in, const bf16_t* wpk, const float* bias, bf16_t* dst0, int D0, bf16_t* dst1,
                        int D1, float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s);
int launch_conv3x3_wgrad_bf16(const ConvIn& in, const bf16_t* dy, int Cout, float* slab, float* dw_oihw, int cin_real,
                              const float* db_partials, int n_db_partials, float* db, int B, int H, int W,
                              hipStream_t s);
int launch_pack_conv3x3_bf16(const float* w_oihw, int Cout, int cin_real, int cin_pad, bf16_t* wfwd, bf16_t* wdgrad,
                             hipStream_t s);
// the same sources compiled for IEEE fp16 (fu_conv_bf16.h, -DFU_HALF=1); buffers are raw 16-bit storage
int conv3x3_num_stat_tiles_f16(int B, int H, int W);
int64_t conv3x3_wgrad_slab_elems_f16(int Cin, int Cout, int B, int H, int W);
int launch_conv3x3_f16(const ConvIn& in, const bf16_t* wpk, const float* bias, bf16_t* dst0, int D0, bf16_t* dst1,
                       int D1, float* stats, int* n_stat_tiles, int B, int H, int W, hipStream_t s);
int launch_conv3x3_wgrad_f16(const ConvIn& in, const bf16_t* dy, int Cout, float* slab, float* dw_oihw, int cin_real,
                             const float* db_partials, int n_db_partials, float* db, int B, int H, int W,
                             hipStream_t s);
int launch_pack_conv3x3_f16(const float* w_oihw, int Cout, int cin_real, int cin_pad, bf16_t* wfwd, bf16_t* wdgrad,
                            hipStream_t s);

int launch_nchw_to_nhwc(Prec p, const float* src, void* dst, int B, int C, int H, int W, int c_pad, hipStream_t s,
                        int src_channels = 0, int src_channel_offset = 0);
int launch_nhwc_to_nchw(Prec p, const void* src, float* dst, int B, int C, int H, int W, int c_pad, hipStream_t s);
// up to 8 fp32 NCHW tensors [B, c[k], H, W] taken side by side along the channel axis; coff = prefix sums of c
struct SrcList { const float* p[8]; int c[8]; int coff[9]; int n; };
// The SrcList of n_src caller sources (fu_forward_srcs, fu_forward_views, fu_op_gather_nchw_to_nhwc): rejects a null table,
// n_src outside 1..8, a null source and a channel count below 1; `who` names the caller in the message.
int make_src_list(const char* who, const float* const* srcs, const int32_t* src_channels, int n_src, SrcList* S);
// n_views view codes packed 3 bits each, the form the views gather takes: rejects null codes, n_views outside 1..8, a code
// outside 0..7 and, where `distinct` is set (fu_forward_views), a repeated code.
int pack_view_codes(const char* who, const int32_t* codes, int n_views, bool distinct, unsigned* packed);
// The one statement of the square-tile rule: a transposing code (bit 4) among the n_views packed ones needs H == W.
int check_view_geometry(const char* who, int n_views, unsigned codes, int H, int W);
// dst [B,H,W,c_pad] <- channels [ch_off, ch_off + C) of the virtual concatenation (zero padding above C)
int launch_gather_nchw_to_nhwc(Prec p, const SrcList& S, void* dst, int B, int C, int H, int W, int c_pad, int ch_off,
                               hipStream_t s);
// test-time augmentation: dst sample v * B + b (v < n_views) <- view ((codes >> 3v) & 7) of crop b (fu_forward_views)
int launch_gather_views_nchw_to_nhwc(Prec p, const SrcList& S, void* dst, int B, int n_views, unsigned codes, int C, int H,
                                     int W, int c_pad, int ch_off, hipStream_t s);

// BN: finalize forward statistics.  partials [nTiles][C][2]; count = B*H*W.
// training: writes mean/invstd/a/b, updates running stats (momentum 0.1, unbiased var) and nbt.
// sync != null (exact data-parallel mode): the statistics of all ranks' batches.
struct BnFwdOut {
  const float* conv_bias; const float* gamma; const float* beta; float eps, momentum;
  float *mean, *invstd, *a, *b, *rmean, *rvar; int64_t* nbt;
};
int launch_bn_finalize(const BnFwdOut& o, const float* partials, int nTiles, int C, int64_t count, double* dscratch,
                       const SyncDesc* sync, hipStream_t s);
// fp64 scratch needed by the two-level reductions: elements for a layer with C channels
static inline int64_t reduce_scratch_elems(int C) { return (int64_t)32 * C * 2; }
// backward: g (in place -> dy).  Two launches + finalize inside.  partials scratch: >= bn_bwd_partial_elems.
int64_t bn_bwd_partial_elems(int C, int64_t npix);
struct BnBwdOut { const float* unscale; float *dgamma, *dbeta, *coef; };
struct BnBwdArgs {
  void* g = nullptr; const void* y = nullptr;          // NHWC [npix][C]
  int C = 0; int64_t npix = 0;
  const float *a = nullptr, *b = nullptr, *mean = nullptr, *invstd = nullptr;
  float *dgamma = nullptr, *dbeta = nullptr;
  float *partials = nullptr, *coef = nullptr;          // scratch: the two sums per block; [C][2] s1/N, s2/N
  float* db_partials = nullptr; int* n_db_partials = nullptr;   // out: per-block sums of dy (the conv's bias gradient) and their count
  double* dscratch = nullptr;
  const SyncDesc* sync = nullptr;                      // exact data-parallel mode: the two sums are summed over the ranks
  const float* unscale = nullptr;                      // fp16: device 1 / loss scale for dgamma / dbeta (null = 1)
  // optional.  g_pool != null: y's 2x2 max-pool ran in forward and g_pool [B, H/2, W/2, C] is dL/d(pooled): the pool's backward
  // is folded into the two passes (g is then the skip gradient only); B, H, W are needed with it
  const void* g_pool = nullptr; int B = 0, H = 0, W = 0;
  int ext_partials = 0;                                // > 0: `partials` already holds that many rows (BnbFuse)
  const HeadGrad* head = nullptr;                      // g is recomputed from the head's dl and w instead of read
  bool two_level = false;                              // test hook: finalise the sums by reduce_partials + k_bn_bwd_finalize (the exact
                                                       // data-parallel form) with world = 1; needs dscratch
};
int launch_bn_bwd(Prec p, const BnBwdArgs& A, hipStream_t s);

int launch_maxpool2(Prec p, const void* src, const float* a, const float* b, void* dst, int B, int H, int W, int C,
                    hipStream_t s);
struct UpTables {  // device tables for one bilinear x2 resize (H x W -> 2H x 2W, placed inside outH x outW)
  const int* y_i0; const int* y_i1; const float* y_w1;  // [2H]
  const int* x_i0; const int* x_i1; const float* x_w1;  // [2W]
  // backward gather lists: for input index i up to UP_BWD_MAX (o, w) pairs
  const int* yb_o; const float* yb_w;  // [H][UP_BWD_MAX]
  const int* xb_o; const float* xb_w;  // [W][UP_BWD_MAX]
  float scale_y, scale_x;              // (in - 1) / (out - 1) in float, as ATen: the forward kernel evaluates the
};                                     // index/weight expressions itself (same values as y_*/x_*)
static constexpr int UP_BWD_MAX = 6;
int launch_upsample2(Prec p, const void* src, const float* a, const float* b, void* dst, int B, int H, int W, int C,
                     int outH, int outW, const UpTables& t, hipStream_t s);
int launch_upsample2_bwd(Prec p, const void* g_dst, void* g_src, int B, int H, int W, int C, int outH, int outW,
                         const UpTables& t, hipStream_t s);

// ConvTranspose2d(k2,s2) helpers (bilinear=False variant): the four phase GEMMs run as one 1x1 conv with 4 cout channels at
// the low resolution; depth-to-space (+ F.pad) / space-to-depth (- pad) move between [B,h,w,4C] and [B,2h(+pad),2w(+pad),C];
// pad-region zeroing, bias-gradient partial sums, weight <-> embedded-centre-tap conversions
int launch_depth_to_space(Prec p, const void* y4, void* up, int B, int h, int w, int C, int outH, int outW, hipStream_t s);
int launch_space_to_depth(Prec p, const void* gup, void* g4, int B, int h, int w, int C, int outH, int outW, hipStream_t s);
int launch_colsum_partials(const float* partials, int n, int C, const float* unscale /* fp16: 1 / loss scale, or null */,
                           float* out, hipStream_t s);
int launch_channel_partial_sums(Prec p, const void* g, int C, int64_t npix, float* partials, int* n_partials,
                                hipStream_t s);
int launch_convT_to_w3(const float* w, const float* b, int Cin, int Cout, float* w3, float* bias4, hipStream_t s);
int launch_convT_grad_from_w3(const float* dw3, int Cin, int Cout, float* dw, hipStream_t s);
int launch_copy_channels(Prec p, const void* src, int srcC, int src_off, const float* a, const float* b, void* dst,
                         int dstC, int dst_off, int C, int64_t npix, hipStream_t s);
int launch_center_to_w3(const float* w, int64_t n, float* w3, hipStream_t s);
int launch_center_from_w3(const float* dw3, int64_t n, float* dw, hipStream_t s);

// head: 1x1 conv + bias on relu(a*y+b); logits fp32 NHWC [npix][ncls] (+ optional NCHW copy)
int launch_head_fwd(Prec p, const void* y, const float* a, const float* b, const float* w, const float* bias, int C,
                    int ncls, int B, int H, int W, float* logits_nhwc, float* logits_nchw, hipStream_t s);
static constexpr int HEAD_MAX_CLS = 8;
// the partial buffer of the loss launches (fu_ctx::ce_part), one row of sums per block: the block caps of the loss
// kernels are derived from, or asserted against, this one size
static constexpr int LOSS_PART_FLOATS = 4 * 1024;
// fu_loss_ce_weighted's extras.  class_weight: fp32 [ncls] on the device or null (all ones); c_nll = 1 - eps,
// c_smooth = eps / ncls; weight_sum_dev receives D = sum w[t] (fp32), which launch_ce_grad divides by.
// focal_gamma > 0 (fu_loss_ce_focal; then c_nll = 1, c_smooth = 0): the focal instantiations, each pixel's term times
// (1 - p[t])^gamma; 0 = the weighted instantiations, untouched.
struct CeWeighting {
  const float* class_weight;
  float c_nll, c_smooth;
  float* weight_sum_dev;
  float* weight_sum_out;   // optional
  float focal_gamma = 0.f;
};
// CE loss over stored logits, plain (cw == null) or class-weighted and label-smoothed.  partials (LOSS_PART_FLOATS):
// [nblk][2] (loss sum, valid count as float), weighted [nblk][4] (sum w[t] nll, sum smoothing term, sum w[t], valid
// count; focal: sum w[t] u^gamma nll, 0, sum w[t], valid count) -> finalize
int launch_ce_loss(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                   const CeWeighting* cw, float* partials, float* loss_out, int64_t* n_valid_dev,
                   int64_t* confusion_accum, int64_t* n_valid_out, unsigned long long* conf_tmp /* [64], zero-initialised */,
                   const SyncDesc* sync /* null, or the sums are taken over the ranks */, hipStream_t s);
// dlogits (NHWC fp32) from CE: (softmax - onehot)/n_valid on valid pixels; weighted: the gradient of the loss above
int launch_ce_grad(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                   const CeWeighting* cw, const int64_t* n_valid_dev, float* dlogits_nhwc, hipStream_t s);
// fu_loss_ce_region's soft Tversky term (fu_loss.hip), run after launch_ce_loss / launch_ce_grad of the same call on the same
// stream: adds weight * R to *loss_io and, where dlogits_nhwc is given (training forwards), its gradient to the stored CE
// gradient.  weight > 0, alpha, beta >= 0 with alpha + beta > 0 and smooth > 0 are the caller's to check.  coef:
// REGION_COEF_BYTES on the device (the gradient pass's coefficients); region_out: optional device [1 + ncls] = R, TI_k.
// partials: LOSS_PART_FLOATS floats, free once the CE finalize has run.
static constexpr int REGION_COEF_BYTES = 256;
struct RegionTerm {
  float weight, alpha, beta, smooth;
  float* coef;
  float* region_out;   // optional
};
int launch_region_term(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                       const RegionTerm& rg, float* partials, float* loss_io, float* dlogits_nhwc, const SyncDesc* sync,
                       hipStream_t s);
// BCE + soft Dice on softmax(z)[1]; partials: LOSS_PART_FLOATS floats, coef 4 floats; dlogits may be null (eval)
int launch_bce_dice(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int64_t npix,
                    float dice_w, float* partials, float* coef, float* loss_out, int64_t* n_valid_dev,
                    float* dlogits_nhwc, hipStream_t s);
int launch_dlogits_from_nchw(const float* dlogits_nchw, float* dlogits_nhwc, int ncls, int B, int H, int W,
                             hipStream_t s);
// head backward: G[y] = dlogits * W ; dW = sum dlogits (x) z ; db = sum dlogits
int64_t head_bwd_partial_elems(int C, int ncls);
int launch_head_bwd(Prec p, const float* dlogits_nhwc, const void* y, const float* a, const float* b, const float* w,
                    int C, int ncls, int64_t npix, void* g, float* partials, float* dw, float* db,
                    const float* unscale /* fp16: 1 / loss scale for dw / db, or null */, hipStream_t s,
                    const BnbFuse* fuse = nullptr);

int launch_stitch_add(const float* logits_nhwc, int ncls, int cropW, float* canvas, float* weight, int canvasW, int h0,
                      int w0, int dh, int dw, hipStream_t s);
int launch_stitch_finalize(float* canvas, const float* weight, int ncls, int64_t npix, int64_t* argmax_out,
                           hipStream_t s);
// fu_stitch_add_batch (probs == false: src = the resident NHWC logits) and fu_stitch_add_batch_probs (true: src = the
// caller's probabilities), src [n_samples, H, W, ncls] fp32: validates the host table (fn / batch_name go into the
// messages), uploads it and launches; every check comes before anything is copied or launched
// win_y / win_x (fu_stitch_add_batch_windowed): fp32 device arrays of H and W elements, both or neither; with them crop
// pixel (ly, lx) counts with win_y[ly] * win_x[lx] instead of 1
int launch_stitch_add_batch(DeviceTable& table, const char* fn, const char* batch_name, int n, const fu_stitch_entry* entries,
                            const float* src, int n_samples, bool probs, int H, int W, int ncls, hipStream_t s,
                            const float* win_y = nullptr, const float* win_x = nullptr);
// fu_stitch_finalize_maps: normalised canvas (in place when normalize), uint8 class map / probability bands / top-2
// margin and int64 pixels per argmax class (ADDED to) in one pass; every output optional.  class_values: HOST bytes or null.
// thr (fu_stitch_finalize_maps_ex): null = the argmax; else the class map and the counts follow the thresholded decision
int launch_stitch_finalize_maps(float* canvas, const float* weight, int ncls, int64_t npix, float eps, bool normalize,
                                const unsigned char* class_values, unsigned char* class_out, unsigned char* prob_out,
                                unsigned char* margin_out, int64_t* counts, const fu_class_threshold* thr, hipStream_t s,
                                const unsigned char* valid = nullptr, int nodata_value = 0);
// fu_scene_valid_mask / fu_mask_box_counts (fu_valid_mask.hip): the valid-pixel mask of a resident scene on its grid and its
// count (n_valid: WRITTEN, zeroed on s first), and the non-zero bytes of every box of a table of masks (counts[i] WRITTEN).
// Both check every argument before anything is copied or launched.  valid / nodata_value above
// (fu_stitch_finalize_maps_masked): null = the unmasked kernels; else a pixel whose byte is 0 is finalised as an uncovered
// one, with class byte nodata_value
int launch_scene_valid_mask(const float* raster, int C, int src_h, int src_w, bool use_nodata, float nodata, const int* iy,
                            const float* wy, const int* ix, const float* wx, int grid_h, int grid_w,
                            unsigned char* src_valid, unsigned char* valid, int64_t* n_valid, hipStream_t s);
int launch_mask_box_counts(DeviceTable& table, int n, const fu_mask_box* entries, int64_t* counts, hipStream_t s);
// fu_tiff_unpack (fu_tiff_unpack.hip): the entropy-decoded segments of a TIFF -> fp32 [n_bands, height, width], one launch;
// checks every argument (n_bytes against the layout's arithmetic total included) before it launches
int launch_tiff_unpack(const uint8_t* src, int64_t n_bytes, const fu_tiff_layout& layout, const int32_t* bands, int n_bands,
                       float* out, hipStream_t s);
// fu_tiff_pack (fu_tiff_pack.hip): the inverse -- a strided device raster -> the predictor-applied, tile- or strip-cut byte
// buffer of a TIFF writer, one launch; checks every argument (n_bytes against the layout's total included) before it launches
int launch_tiff_pack(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, const fu_tiff_layout& layout,
                     uint8_t* dst, int64_t n_bytes, hipStream_t s);
// fu_map_overviews (fu_overview.hip): the ceil-halved overview levels of a strided device raster, six per launch from one
// LDS-resident base tile; checks every argument before it launches
int launch_map_overviews(const void* src, int64_t band_stride, int64_t row_stride, int64_t col_stride, int bands, int h, int w,
                         int kind, const uint8_t* valid, int nodata_value, int n_levels, void* dst, int64_t dst_elems,
                         uint8_t* valid_dst, hipStream_t s);
// fu_map_components / fu_map_sieve (fu_post.hip): union-find labelling of a uint8 map (the label of a pixel = the smallest
// linear index of its component) and the connected-component sieve on top of it; the caller has checked every argument.
// workspace: sieve_workspace_bytes(h, w) = 16 B per pixel (64-bit donor keys, labels, sizes); stats: int64[2] ADDED to, or null
int64_t sieve_workspace_bytes(int h, int w);
int launch_map_components(const unsigned char* map, int h, int w, int connectivity, int* labels, hipStream_t s);
int launch_map_sieve(const unsigned char* map, unsigned char* out, int h, int w, int connectivity, int min_pixels, int frozen,
                     int passes, void* workspace, int64_t* stats, hipStream_t s);
// fu_map_edge_offsets / fu_map_edge_rings (fu_vector.hip): the crack edges of a class map's selected values (select: host
// [256]) and their rings; both check every argument before anything is launched.  The *_workspace_bytes give 0 for a size
// the calls reject.
int64_t map_edges_workspace_bytes(int h, int w);
int64_t map_rings_workspace_bytes(int64_t capacity);
int launch_map_edge_offsets(const unsigned char* map, int h, int w, const unsigned char* select, int* offsets, void* workspace,
                            int64_t workspace_bytes, hipStream_t s);
int launch_map_edge_rings(const unsigned char* map, const int* labels, int h, int w, const unsigned char* select, int connectivity,
                          const int* offsets, int64_t capacity, int* start, int* comp, int* ring, int* rank, int* flags,
                          void* workspace, int64_t workspace_bytes, hipStream_t s);
int launch_eval_confusion(const float* logits_nhwc, const int64_t* target, int ncls, int ignore_index, int B, int64_t hw,
                          int64_t* counts, hipStream_t s);
// fu_eval_prob_hist (logits: src = the resident NHWC logits) / fu_prob_hist (src = fp32 probabilities [npix, ncls]):
// hist[c][t][bin] and top[argmax == t][bin], both ADDED to, either optional; checks every argument (fn goes into the messages)
int launch_prob_hist(const char* fn, const float* src, bool logits, const int64_t* target, int64_t npix, int ncls,
                     int ignore_index, int n_bins, int64_t* hist, int64_t* top, hipStream_t s);
// fu_merge_views: softmax of each view's logits, inverse view, mean in view order -> probs [B, H, W, k] (optional) and
// confusion counts of its argmax (optional, with target; ADDED to)
int launch_merge_views(const float* logits_nhwc, int H, int W, int ncls, int B, int n_views, unsigned codes, float* probs,
                       const int64_t* target, int ignore_index, int64_t* counts, hipStream_t s);
int launch_assemble_tiles(const float* const* srcs, const int* src_channels, int n_src, int B, int H, int W, const int* vh,
                          const int* vw, int norm_mode, const float* gmean, const float* gstd, float pad_value, float* out,
                          float* mean_out, float* std_out, hipStream_t s);
// fu_scene_crops: the boxes as fu_assemble_tiles would assemble them from a zero batch holding each box in the top-left
// corner (valid size = the box) -- the same kernels, instantiated on scene-box addressing.  Validates every argument and
// entry, then uploads the table and launches: a rejected call leaves the stream untouched.
int launch_scene_crops(DeviceTable& table, int n, const fu_scene_crop* entries, int C, int H, int W, int norm_mode,
                       const float* gmean, const float* gstd, float pad_value, float* out, float* mean_out, float* std_out,
                       hipStream_t s);
// fu_scene_train_tiles[_ex] (fu_scene_train.hip): launch_scene_crops composed with launch_augment and the label decode, with
// no batch in between, and the radiometric and zoom parts of `aug` applied in the same pass; checked, uploaded and launched
// in the same way, every array of `aug` included.  A null or all-off `aug` is fu_scene_train_tiles: its table, its messages
// and its kernel.
int launch_scene_train_tiles(DeviceTable& table, int n, const fu_scene_train_entry* entries, int C, int H, int W,
                             int norm_mode, const float* gmean, const float* gstd, float pad_value, int64_t nodata_value,
                             int64_t target_fill, float* image_out, int64_t* target_out, float* mean_out, float* std_out,
                             const fu_scene_aug* aug, hipStream_t s);
// fu_label_class_counts: counts[d] += #pixels of the entries' label boxes that decode to class d (0 <= d < n_classes);
// checked, uploaded and launched in the same way
int launch_label_class_counts(DeviceTable& table, int n, const fu_scene_train_entry* entries, int64_t nodata_value,
                              int n_classes, int64_t* counts, hipStream_t s);
// fu_label_box_counts: counts[i][0..2] = #pixels of entry i's label box by raw category (other / raw 2 / raw 0), written;
// the same entry check, upload and one launch
int launch_label_box_counts(DeviceTable& table, int n, const fu_scene_train_entry* entries, int64_t* counts, hipStream_t s);
// fu_band_stats: the caller's per-channel accumulators (all ADDED to) and the histogram's geometry
struct BandAccum {
  int64_t* count; double* sum; double* sumsq; float* vmin; float* vmax; int64_t* n_nonfinite;
  int64_t* hist; int n_bins; float lo, hi;
};
int64_t band_stats_workspace_bytes(int n_channels, int n_bins);
int launch_band_stats(const float* const* srcs, const int* src_channels, int n_src, int B, int H, int W, const int* vh,
                      const int* vw, int mask_mode, const BandAccum& acc, void* workspace, int64_t workspace_bytes,
                      hipStream_t s);
int launch_resize_lanczos4_tiles(const float* win, int B, int C, int win_h, int win_w, const int* iy, const float* wy,
                                 const int* ix, const float* wx, int TH, int TW, int scale_mode, float* out, hipStream_t s);
int launch_augment(const float* img, const int64_t* tgt, float* img_o, int64_t* tgt_o, const int* flags,
                   const float* angle, int B, int C, int H, int W, int64_t target_fill, hipStream_t s);

}  // namespace fu
