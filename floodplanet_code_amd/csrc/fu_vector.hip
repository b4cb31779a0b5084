// Vector output of class maps on the device: the crack edges of the selected values (fu_map_edge_offsets) and their rings
// (fu_map_edge_rings).  floodplanet_code_amd/vectorize.py holds the numpy statements (edge_offsets_host, edge_rings_host);
// integer work only, every result is exact, canonical and independent of scheduling.
//
// A selected pixel owns a directed unit edge on every side (0 top, 1 right, 2 bottom, 3 left; side s heads E, S, W, N)
// where the neighbour lies outside the map or has another value; edges are numbered by owner pixel, then side.
//   k_edge_count_scan  a workgroup takes SCAN_PIX consecutive pixels, SCAN_PER_THREAD next to each other per thread: the
//                      side counts, a serial scan in the thread, a shuffle scan in the wave, LDS across the four waves;
//                      block-local exclusive offsets and the block's total go out
//   k_scan_totals      ONE workgroup scans the block totals in place, chunk after chunk with a carry
//   k_scan_add         adds the block's prefix; the last element, offsets[h * w], becomes n_edges
// The phases are ordered by kernel boundaries on the one stream; no workgroup ever waits for another.
//   k_edge_emit        one thread per pixel: start vertex and component of its edges, and for each its successor next[e]
//                      (the rule of vectorize.py; the neighbour's side mask is recomputed from the map) together with the
//                      successor's flags word -- heading | corner << 2 -- which its one predecessor alone writes
//   k_ring_round       ring by min-doubling: r[e] = min(r[e], r[nxt[e]]), nxt[e] = nxt[nxt[e]]
//   k_rank_init        cuts every cycle in front of its leader (the edge whose index is the ring id)
//   k_rank_round       Wyllie: dist[e] += dist[nxt[e]], nxt[e] = nxt[nxt[e]]; the tail points at itself with distance 0
//   k_rank_final       rank = dist[leader] - dist[e] = length - 1 - distance
// Every round reads one pair of buffers and writes the other, and runs ceil(log2(max(capacity, 2))) times: both
// recurrences stay put once converged, so nothing is read back.  All edge kernels take n = offsets[h * w] on the device,
// write nothing when n > capacity, and guard every store and every gather through next by n: a stale offsets array can
// give wrong rings but no access outside the buffers.
#include "fu_common.h"

#include "../../include/floodunet.h"

namespace fu {

namespace {

constexpr int VEC_BLOCK = 256;
constexpr int SCAN_PER_THREAD = 8, SCAN_PIX = VEC_BLOCK * SCAN_PER_THREAD;

struct SelectBits { unsigned w[8]; };              // 256 flags, by value in the kernel arguments

__device__ __forceinline__ bool selected(const SelectBits& sel, int v) { return (sel.w[v >> 5] >> (v & 31)) & 1u; }

// the 4-bit side mask of pixel i = (y, x) of value v (selection not looked at)
__device__ __forceinline__ int side_mask(const unsigned char* map, int H, int W, int i, int y, int x, int v) {
  int m = 0;
  if (y == 0 || map[i - W] != v) m |= 1;
  if (x == W - 1 || map[i + 1] != v) m |= 2;
  if (y == H - 1 || map[i + W] != v) m |= 4;
  if (x == 0 || map[i - 1] != v) m |= 8;
  return m;
}

// inclusive scan over the workgroup's VEC_BLOCK threads -> the thread's inclusive value; *total = the workgroup's sum.
// wave_sums: LDS int [VEC_BLOCK / 64].  Every thread of the workgroup calls it.
__device__ __forceinline__ int block_inclusive_scan(int v, int* wave_sums, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  __syncthreads();                                 // the previous use of wave_sums is over
  if (lane == 63) wave_sums[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < VEC_BLOCK / 64; ++k) {
    const int s = wave_sums[k];
    if (k < wave) before += s;
    all += s;
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_edge_count_scan(const unsigned char* map, int H, int W, SelectBits sel, int* offsets,
                                                               int* block_totals) {
  __shared__ int wave_sums[VEC_BLOCK / 64];
  const int n = H * W;
  const int i0 = blockIdx.x * SCAN_PIX + threadIdx.x * SCAN_PER_THREAD;      // < 2^28 + SCAN_PIX
  int cnt[SCAN_PER_THREAD];
  int sum = 0;
  if (i0 < n) {
    int y = i0 / W, x = i0 - y * W;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
      const int i = i0 + k;
      int c = 0;
      if (i < n) {
        const int v = map[i];
        if (selected(sel, v)) c = __popc(side_mask(map, H, W, i, y, x, v));
        if (++x == W) { x = 0; ++y; }
      }
      cnt[k] = sum;                                // exclusive inside the thread
      sum += c;
    }
  }
  int total;
  const int before = block_inclusive_scan(sum, wave_sums, &total) - sum;
  if (i0 < n) {
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
      if (i0 + k < n) offsets[i0 + k] = before + cnt[k];
  }
  if (threadIdx.x == 0) block_totals[blockIdx.x] = total;
}

// ONE workgroup: totals[0..n_blocks) -> their exclusive prefix sums, in place; totals[n_blocks] = the grand total
__global__ __launch_bounds__(VEC_BLOCK) void k_scan_totals(int* totals, int n_blocks) {
  __shared__ int wave_sums[VEC_BLOCK / 64];
  int carry = 0;
  for (int base = 0; base < n_blocks; base += VEC_BLOCK) {       // uniform
    const int j = base + threadIdx.x;
    const int v = j < n_blocks ? totals[j] : 0;
    int total;
    const int incl = block_inclusive_scan(v, wave_sums, &total);
    if (j < n_blocks) totals[j] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) totals[n_blocks] = carry;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_scan_add(int* offsets, int n, const int* totals, int n_blocks) {
  const int add = totals[blockIdx.x];
  const int i0 = blockIdx.x * SCAN_PIX + threadIdx.x;
#pragma unroll
  for (int k = 0; k < SCAN_PER_THREAD; ++k) {
    const int i = i0 + k * VEC_BLOCK;
    if (i < n) offsets[i] += add;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = totals[n_blocks];
}

// ---- rings -----------------------------------------------------------------------------------------------------------
// n_edges as the kernels take it: offsets[h * w] when it lies in 0..capacity, else -1 (nothing is written)
__device__ __forceinline__ int edges_on_device(const int* offsets, int n_pix, int64_t capacity) {
  const int n = offsets[n_pix];
  return n >= 0 && n <= capacity ? n : -1;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_edge_emit(const unsigned char* map, const int* labels, int H, int W, SelectBits sel,
                                                         int conn8, const int* offsets, int64_t capacity, int* start, int* comp,
                                                         int* flags, int* nxt) {
  const int n_pix = H * W;
  const int N = edges_on_device(offsets, n_pix, capacity);
  const int i = blockIdx.x * VEC_BLOCK + threadIdx.x;
  if (N <= 0 || i >= n_pix) return;
  const int v = map[i];
  if (!selected(sel, v)) return;
  const int y = i / W, x = i - y * W;
  const int mask = side_mask(map, H, W, i, y, x, v);
  if (!mask) return;
  const int label = labels[i];
  int e = offsets[i];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (!((mask >> d) & 1)) continue;
    // headings E, S, W, N: (dx, dy) = (1, 0), (0, 1), (-1, 0), (0, -1); the left of d is (d + 3) % 4
    const int dx = d == 0 ? 1 : d == 2 ? -1 : 0, dy = d == 1 ? 1 : d == 3 ? -1 : 0;
    const int dl = (d + 3) & 3;
    const int lx_ = dl == 0 ? 1 : dl == 2 ? -1 : 0, ly_ = dl == 1 ? 1 : dl == 3 ? -1 : 0;
    const int rx = x + dx, ry = y + dy;            // R: ahead-right of the end vertex
    const int px = rx + lx_, py = ry + ly_;        // Lp: ahead-left
    const bool r_in = rx >= 0 && rx < W && ry >= 0 && ry < H && map[ry * W + rx] == v;
    const bool l_in = px >= 0 && px < W && py >= 0 && py < H && map[py * W + px] == v;
    int qx, qy, s;
    if (l_in && (r_in || conn8)) { qx = px; qy = py; s = dl; }
    else if (r_in) { qx = rx; qy = ry; s = d; }
    else { qx = x; qy = y; s = (d + 1) & 3; }
    const int q = qy * W + qx;
    const int qmask = q == i ? mask : side_mask(map, H, W, q, qy, qx, v);
    int nx = offsets[q] + __popc(qmask & ((1 << s) - 1));
    if (e >= 0 && e < N) {
      if (nx < 0 || nx >= N) nx = e;               // only under a stale offsets array: wrong, but inside the buffers
      const int sx = x + (d == 1 || d == 2), sy = y + (d >= 2);
      start[e] = sy * (W + 1) + sx;
      comp[e] = label;
      nxt[e] = nx;
      flags[nx] = s | ((s != d) << 2);             // every edge has exactly one predecessor: one writer per word
    }
    ++e;
  }
}

// r_in == nullptr: the identity (the first round)
__global__ __launch_bounds__(VEC_BLOCK) void k_ring_round(const int* offsets, int n_pix, int64_t capacity, const int* r_in,
                                                          const int* n_in, int* r_out, int* n_out) {
  const int N = edges_on_device(offsets, n_pix, capacity);
  const int e = blockIdx.x * VEC_BLOCK + threadIdx.x;
  if (e >= N) return;
  int j = n_in[e];
  if (j < 0 || j >= N) j = e;
  const int re = r_in ? r_in[e] : e, rj = r_in ? r_in[j] : j;
  int jj = n_in[j];
  if (jj < 0 || jj >= N) jj = e;
  r_out[e] = min(re, rj);
  n_out[e] = jj;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_rank_init(const int* offsets, int n_pix, int64_t capacity, const int* ring,
                                                         const int* nxt, int* ring_out, int* d_out, int* n_out) {
  const int N = edges_on_device(offsets, n_pix, capacity);
  const int e = blockIdx.x * VEC_BLOCK + threadIdx.x;
  if (e >= N) return;
  const int r = ring[e], j = nxt[e];
  const bool tail = j == r;                        // the leader comes next: the cycle is cut here
  ring_out[e] = r;
  d_out[e] = tail ? 0 : 1;
  n_out[e] = tail ? e : j;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_rank_round(const int* offsets, int n_pix, int64_t capacity, const int* d_in,
                                                          const int* n_in, int* d_out, int* n_out) {
  const int N = edges_on_device(offsets, n_pix, capacity);
  const int e = blockIdx.x * VEC_BLOCK + threadIdx.x;
  if (e >= N) return;
  int j = n_in[e];
  if (j < 0 || j >= N) j = e;
  int jj = n_in[j];
  if (jj < 0 || jj >= N) jj = e;
  d_out[e] = d_in[e] + d_in[j];                    // the tail: 0 + 0
  n_out[e] = jj;
}

__global__ __launch_bounds__(VEC_BLOCK) void k_rank_final(const int* offsets, int n_pix, int64_t capacity, const int* ring,
                                                          const int* dist, int* rank) {
  const int N = edges_on_device(offsets, n_pix, capacity);
  const int e = blockIdx.x * VEC_BLOCK + threadIdx.x;
  if (e >= N) return;
  int r = ring[e];
  if (r < 0 || r >= N) r = e;
  rank[e] = dist[r] - dist[e];
}

SelectBits select_bits(const unsigned char* select) {
  SelectBits s = {};
  for (int v = 0; v < 256; ++v)
    if (select[v]) s.w[v >> 5] |= 1u << (v & 31);
  return s;
}

bool map_size_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= FU_MAP_MAX_PIXELS; }

int64_t ring_array_bytes(int64_t capacity) { return ceil_div64(capacity * 4, 16) * 16; }

int rounds_for(int64_t capacity) {
  int r = 1;
  while (((int64_t)1 << r) < capacity) ++r;
  return r;                                        // ceil(log2(max(capacity, 2)))
}

}  // namespace

int64_t map_edges_workspace_bytes(int h, int w) {
  if (!map_size_ok(h, w)) return 0;
  return ceil_div64(((int64_t)ceil_div(h * w, SCAN_PIX) + 1) * 4, 16) * 16;   // the block totals and the grand total
}

int64_t map_rings_workspace_bytes(int64_t capacity) {
  if (capacity < 0 || capacity > 4 * (int64_t)FU_MAP_MAX_PIXELS) return 0;
  return 5 * ring_array_bytes(capacity);           // next, and two pairs of ping-pong buffers
}

int launch_map_edge_offsets(const unsigned char* map, int h, int w, const unsigned char* select, int* offsets, void* workspace,
                            int64_t workspace_bytes, hipStream_t s) {
  const char* fn = "fu_map_edge_offsets";
  FU_REQUIRE(map && select && offsets, "%s: null map / select / offsets_out", fn);
  FU_REQUIRE(map_size_ok(h, w), "%s: map %dx%d is empty or has more than 2^28 pixels", fn, h, w);
  FU_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= map_edges_workspace_bytes(h, w),
             "%s: workspace missing, not 16-byte aligned or smaller than fu_map_edges_workspace_bytes = %lld", fn,
             (long long)map_edges_workspace_bytes(h, w));
  const int n = h * w, n_blocks = ceil_div(n, SCAN_PIX);
  int* totals = static_cast<int*>(workspace);
  hipLaunchKernelGGL(k_edge_count_scan, dim3(n_blocks), dim3(VEC_BLOCK), 0, s, map, h, w, select_bits(select), offsets, totals);
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(VEC_BLOCK), 0, s, totals, n_blocks);
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_scan_add, dim3(n_blocks), dim3(VEC_BLOCK), 0, s, offsets, n, totals, n_blocks);
  FU_LAUNCH_CHECK();
  return 0;
}

int launch_map_edge_rings(const unsigned char* map, const int* labels, int h, int w, const unsigned char* select, int connectivity,
                          const int* offsets, int64_t capacity, int* start, int* comp, int* ring, int* rank, int* flags,
                          void* workspace, int64_t workspace_bytes, hipStream_t s) {
  const char* fn = "fu_map_edge_rings";
  FU_REQUIRE(map && labels && select && offsets, "%s: null map / labels / select / offsets", fn);
  FU_REQUIRE(map_size_ok(h, w), "%s: map %dx%d is empty or has more than 2^28 pixels", fn, h, w);
  FU_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  FU_REQUIRE(capacity >= 0 && capacity <= 4 * (int64_t)FU_MAP_MAX_PIXELS, "%s: capacity %lld not in 0..2^30", fn,
             (long long)capacity);
  if (capacity == 0) return 0;
  FU_REQUIRE(start && comp && ring && rank && flags, "%s: null output", fn);
  FU_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= map_rings_workspace_bytes(capacity),
             "%s: workspace missing, not 16-byte aligned or smaller than fu_map_rings_workspace_bytes = %lld", fn,
             (long long)map_rings_workspace_bytes(capacity));
  const int n_pix = h * w;
  const int64_t stride = ring_array_bytes(capacity) / 4;
  int* nxt = static_cast<int*>(workspace);
  int* nbuf[2] = {nxt + stride, nxt + 2 * stride};
  int* vbuf[2] = {nxt + 3 * stride, nxt + 4 * stride};
  const dim3 eblocks((unsigned)ceil_div64(capacity, VEC_BLOCK)), block(VEC_BLOCK);
  const int rounds = rounds_for(capacity);
  hipLaunchKernelGGL(k_edge_emit, dim3(ceil_div(n_pix, VEC_BLOCK)), block, 0, s, map, labels, h, w, select_bits(select),
                     connectivity == 8 ? 1 : 0, offsets, capacity, start, comp, flags, nxt);
  FU_LAUNCH_CHECK();
  for (int k = 0; k < rounds; ++k) {               // round k reads buffers (k + 1) & 1 (round 0: the identity and next)
    const int in = (k + 1) & 1, out = k & 1;
    hipLaunchKernelGGL(k_ring_round, eblocks, block, 0, s, offsets, n_pix, capacity, k == 0 ? (const int*)nullptr : vbuf[in],
                       k == 0 ? (const int*)nxt : nbuf[in], vbuf[out], nbuf[out]);
    FU_LAUNCH_CHECK();
  }
  const int done = (rounds - 1) & 1;               // the ring ids lie in vbuf[done]; the distances start in the other one
  hipLaunchKernelGGL(k_rank_init, eblocks, block, 0, s, offsets, n_pix, capacity, vbuf[done], nxt, ring, vbuf[done ^ 1],
                     nbuf[done ^ 1]);
  FU_LAUNCH_CHECK();
  int cur = done ^ 1;
  for (int k = 0; k < rounds; ++k, cur ^= 1) {
    hipLaunchKernelGGL(k_rank_round, eblocks, block, 0, s, offsets, n_pix, capacity, vbuf[cur], nbuf[cur], vbuf[cur ^ 1],
                       nbuf[cur ^ 1]);
    FU_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_rank_final, eblocks, block, 0, s, offsets, n_pix, capacity, ring, vbuf[cur], rank);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace fu
