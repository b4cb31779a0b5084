// Device helpers shared by the elementwise NHWC kernels (fu_bn.hip, fu_resample.hip, fu_head.hip); private to csrc.
#pragma once
#include "fu_common.h"

#ifdef __HIPCC__
namespace fu {

// fixed-shape xor tree over the 32 lanes of a half wave (deterministic); every lane ends with the total
__device__ __forceinline__ double half_wave_sum(double v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T, int V>
__device__ __forceinline__ void load_act(const T* p, const float (&av)[V], const float (&bv)[V], bool bn, float (&z)[V]) {
  VecIO<T>::load(p, z);
  if (bn) {
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = bn_act(av[j], z[j], bv[j]);
  }
}
template <int V>
__device__ __forceinline__ void load_coef(const float* a, const float* b, int c0, float (&av)[V], float (&bv)[V]) {
#pragma unroll
  for (int j = 0; j < V; j += 4) {
    const float4 x = *reinterpret_cast<const float4*>(a + c0 + j);
    const float4 y = *reinterpret_cast<const float4*>(b + c0 + j);
    av[j] = x.x; av[j + 1] = x.y; av[j + 2] = x.z; av[j + 3] = x.w;
    bv[j] = y.x; bv[j + 1] = y.y; bv[j + 2] = y.z; bv[j + 3] = y.w;
  }
}

// The row kernels (max-pool, bilinear resize, head) share one indexing scheme: grid = (items of one output row / 256, rows, batch), one
// 16-byte channel vector (VecIO: 4 fp32 / 8 bf16 or fp16) per thread, 32-bit index math.  (The first versions decoded a flat
// 64-bit index with four 64-bit divisions per 8-byte vector and ran 2-5x off the HBM roofline on index math alone.)
// Their launch geometry:
template <typename T>
static bool row_grid(int C, int items_w, int rows, int B, dim3* grid, int* CV, unsigned* rcp) {
  constexpr int V = 16 / (int)sizeof(T);
  if (C % V != 0 || rows > 65535 || B > 65535) return false;
  *CV = C / V;
  *rcp = host_rcp(*CV);
  *grid = dim3(ceil_div(items_w * *CV, 256), rows, B);
  return true;
}

// block size of the per-channel partial-sum kernels (BatchNorm backward, k_channel_partial_sums)
static constexpr int BNB_THREADS = 256;

// ------------------------------------------------------------------------------------------------
// BatchNorm + ReLU backward core (fu_bn.hip).  g = dL/d relu(bn(y)):
//   m = [a*y+b > 0], xh = (y-mean)*invstd
//   s1 = sum g*m, s2 = sum g*m*xh   (dbeta, dgamma)
//   dy = a * (g*m - s1/N - xh*s2/N)
// xh here is (y - mean) * invstd, two roundings.  The producers that emit s1 / s2 from their own epilogues (k_head_bwd, the
// dgrad kernels: BnbFuse) accumulate against fmaf(y, invstd, -mean * invstd), one rounding: each side keeps its expression,
// unifying them would move the bits of one path.
// The reduce kernels accumulate s2 as fmaf(gm, xh, s2), written out: the compiler contracted `s2 += gm * xh` to that in every
// instantiation anyway, but only where its vectoriser left the multiply next to the add, so the bits hung on code shape.
// ------------------------------------------------------------------------------------------------
// one thread's V channels [c0, c0 + V): a, b, mean, invstd and, for the apply pass, c1 = s1/N, c2 = s2/N from coef [C][2]
template <int V, bool APPLY>
struct BnbCoef {
  float a[V], b[V], mean[V], invstd[V], c1[V], c2[V];
  __device__ __forceinline__ void load(const float* ap, const float* bp, const float* meanp, const float* invstdp,
                                       const float* coef, int c0) {
    load_coef<V>(ap, bp, c0, a, b);
    load_coef<V>(meanp, invstdp, c0, mean, invstd);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      c1[j] = APPLY ? coef[(c0 + j) * 2 + 0] : 0.f;
      c2[j] = APPLY ? coef[(c0 + j) * 2 + 1] : 0.f;
    }
  }
  __device__ __forceinline__ float pre(int j, float y) const { return bn_act_pre(a[j], y, b[j]); }
  __device__ __forceinline__ float masked(int j, float g, float y) const { return pre(j, y) > 0.f ? g : 0.f; }
  __device__ __forceinline__ float xhat(int j, float y) const { return (y - mean[j]) * invstd[j]; }
  __device__ __forceinline__ float dy(int j, float gm, float y) const { return a[j] * (gm - c1[j] - xhat(j, y) * c2[j]); }
};

// Block epilogue of the per-channel partial-sum kernels: thread (row, channels [c0, c0 + V)) puts its NS running sums per channel
// into sm [rows][C][NS]; after the barrier thread c adds the rows in order (deterministic) and writes out [block][C][NS].
// Every thread of the block calls it; threads past the last whole row (row >= rows) only take part in the second half.
template <int NS, int V>
__device__ __forceinline__ void block_rows_to_partials(float* sm, int row, int rows, int C, int c0, const float (&s)[NS][V],
                                                       float* __restrict__ out) {
  if (row < rows) {
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int v = 0; v < NS; ++v) sm[(row * C + c0 + j) * NS + v] = s[v][j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += BNB_THREADS) {
    float t[NS];
#pragma unroll
    for (int v = 0; v < NS; ++v) t[v] = 0.f;
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int v = 0; v < NS; ++v) t[v] += sm[(r * C + c) * NS + v];
    }
#pragma unroll
    for (int v = 0; v < NS; ++v) out[((int64_t)blockIdx.x * C + c) * NS + v] = t[v];
  }
}

// channel c's forward statistics from S = sum y, Q = sum y*y over `count` elements (fp64): mean / invstd / a / b, running statistics
__device__ __forceinline__ void bn_fwd_finish(double S, double Q, double count, int c, const BnFwdOut& o) {
  const double m0 = S / count;
  double var = Q / count - m0 * m0;
  if (var < 0.0) var = 0.0;
  const double mean = m0 + (o.conv_bias ? (double)o.conv_bias[c] : 0.0);
  const float invstd = (float)(1.0 / sqrt(var + (double)o.eps));
  const float meanf = (float)mean;
  const float a = o.gamma[c] * invstd;
  o.mean[c] = meanf;
  o.invstd[c] = invstd;
  o.a[c] = a;
  o.b[c] = o.beta[c] - meanf * a;
  if (o.rmean) {
    const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
    o.rmean[c] = (1.f - o.momentum) * o.rmean[c] + o.momentum * meanf;
    o.rvar[c] = (1.f - o.momentum) * o.rvar[c] + o.momentum * (float)unbiased;
  }
  if (o.nbt && c == 0) *o.nbt += 1;
}

// channel c's backward sums S1 = sum g*m, S2 = sum g*m*xh over `count` elements -> dbeta / dgamma / coef.  Exact data-parallel
// mode: the sums cover all ranks and the parameter gradients are summed over the ranks afterwards, so each rank contributes
// grad_share = 1/world of them (1.0 otherwise, an exact factor).
__device__ __forceinline__ void bn_bwd_finish(double S1, double S2, double count, double grad_share, int c,
                                              const BnBwdOut& o) {
  const double us = o.unscale ? (double)*o.unscale : 1.0;  // fp16 mode: g carries the loss scale, the parameters' gradients do not
  if (o.dbeta) o.dbeta[c] = (float)(S1 * grad_share * us);
  if (o.dgamma) o.dgamma[c] = (float)(S2 * grad_share * us);
  o.coef[c * 2 + 0] = (float)(S1 / count);
  o.coef[c * 2 + 1] = (float)(S2 / count);
}

}  // namespace fu
#endif  // __HIPCC__
