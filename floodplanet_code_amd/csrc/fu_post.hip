// Post-processing of class maps on the device: connected-component labelling (fu_map_components) and the
// connected-component sieve (fu_map_sieve).  Integer work only; every result is exact and order-free.
//
// Labelling is union-find over the pixel grid, the label array being the parent array: parent[i] <= i always, a root
// has parent[i] == i, and a link always hangs the larger root under the smaller one (atomicMin), so the root a
// component ends with is its smallest linear index -- the canonical label of postprocess.label_components_host.
//   k_ccl_tile     one workgroup per 32 x 32 tile: union of the in-tile neighbours in LDS (LDS atomics, no global
//                  traffic), then every pixel's in-tile root goes out as a global index
//   k_ccl_seams    the neighbour pairs that straddle a tile border, united in global memory
//   k_ccl_flatten  every pixel walks to its root and stores it; the sieve also counts the component sizes here
// The sieve adds k_sieve_donor (a small component's pixels offer their foreign edge neighbours' components to a 64-bit
// atomicMax at the component's root) and k_sieve_apply (re-value, stats).  Five launches per pass, none for the host to
// wait on.
//
// Every loop walks a label index towards its root and so has a strictly decreasing quantity: find's index, and in
// unite the larger of the two indices.  No thread waits for another thread's write; the value an atomicMin returns is
// taken as the truth about the word it hit.  Inside the launches that change the label array with atomics it is read
// with agent-scope relaxed atomic loads (the XCDs' L2s are not coherent for plain loads inside a launch, and a plain
// load could be hoisted out of find's loop); between the launches the kernel boundary on one stream orders everything.
#include "fu_common.h"

namespace fu {

namespace {

constexpr int CCL_TILE = 32;                       // tile edge; 256 threads, four rows apart by 8 per thread
constexpr int CCL_TILE_PIX = CCL_TILE * CCL_TILE;
constexpr int POST_BLOCK = 256;

// ---- union-find in LDS -----------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* L, int a) {
  for (;;) {
    const int p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p >= a) return a;                          // p == a: a root (p > a never happens; it would also end the walk)
    a = p;
  }
}

__device__ __forceinline__ void lds_unite(int* L, int a, int b) {
  a = lds_find(L, a);
  b = lds_find(L, b);
  while (a != b) {                                 // max(a, b) falls strictly
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old >= a) break;                           // a was a root and now hangs under b
    a = lds_find(L, old);                          // a already hung under old < a: unite that with b instead
  }
}

// ---- union-find in global memory -------------------------------------------------------------------------------------
__device__ __forceinline__ int glb_find(int* L, int a) {
  for (;;) {
    const int p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= a) return a;
    a = p;
  }
}

__device__ __forceinline__ void glb_unite(int* L, int a, int b) {
  a = glb_find(L, a);
  b = glb_find(L, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old >= a) break;
    a = glb_find(L, old);
  }
}

// One workgroup per tile.  labels[i] = the global index of pixel i's root inside its tile; sizes / keys (the sieve's
// arrays, or null) are zeroed on the way.
__global__ __launch_bounds__(256) void k_ccl_tile(const unsigned char* map, int H, int W, int tiles_x, int conn8, int* labels,
                                                  int* sizes, unsigned long long* keys) {
  __shared__ int L[CCL_TILE_PIX];
  __shared__ short V[CCL_TILE_PIX];                // the pixel's value, -1 outside the map
  const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * CCL_TILE, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * CCL_TILE;
  const int lx = threadIdx.x & (CCL_TILE - 1), ly0 = threadIdx.x / CCL_TILE;
  const int x = tx0 + lx;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ly = ly0 + 8 * r, y = ty0 + ly, l = ly * CCL_TILE + lx;
    const bool in = x < W && y < H;
    V[l] = in ? (short)map[(int64_t)y * W + x] : (short)-1;
    L[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ly = ly0 + 8 * r, l = ly * CCL_TILE + lx;
    const short v = V[l];
    if (v < 0) continue;
    if (lx > 0 && V[l - 1] == v) lds_unite(L, l, l - 1);
    if (ly > 0) {
      if (V[l - CCL_TILE] == v) lds_unite(L, l, l - CCL_TILE);
      if (conn8) {
        if (lx > 0 && V[l - CCL_TILE - 1] == v) lds_unite(L, l, l - CCL_TILE - 1);
        if (lx < CCL_TILE - 1 && V[l - CCL_TILE + 1] == v) lds_unite(L, l, l - CCL_TILE + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ly = ly0 + 8 * r, y = ty0 + ly, l = ly * CCL_TILE + lx;
    if (V[l] < 0) continue;
    const int root = lds_find(L, l);               // nobody writes L any more
    const int64_t i = (int64_t)y * W + x;
    labels[i] = (ty0 + root / CCL_TILE) * W + tx0 + (root & (CCL_TILE - 1));
    if (sizes) sizes[i] = 0;
    if (keys) keys[i] = 0ull;
  }
}

// One thread per pixel; only a pixel with a neighbour (left, up, and under 8-connectivity up-left / up-right) in another
// tile has work.
__global__ __launch_bounds__(POST_BLOCK) void k_ccl_seams(const unsigned char* map, int H, int W, int conn8, int* labels) {
  const int n = H * W;
  const int i = blockIdx.x * POST_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int y = i / W, x = i - y * W;
  const int lx = x & (CCL_TILE - 1), ly = y & (CCL_TILE - 1);
  const bool left = lx == 0 && x > 0, top = ly == 0 && y > 0, right = conn8 && lx == CCL_TILE - 1 && x < W - 1 && y > 0;
  if (!(left || top || right)) return;
  const unsigned char v = map[i];
  if (left && map[i - 1] == v) glb_unite(labels, i, i - 1);
  if (top && map[i - W] == v) glb_unite(labels, i, i - W);
  if (conn8 && y > 0) {
    if (x > 0 && (left || top) && map[i - W - 1] == v) glb_unite(labels, i, i - W - 1);
    if (x < W - 1 && (top || right) && map[i - W + 1] == v) glb_unite(labels, i, i - W + 1);
  }
}

// labels[i] = root(i); a workgroup takes FLAT_PIX consecutive pixels.  A concurrent reader sees pixel i's old parent or
// its root -- both ancestors of i -- so the walk stays inside the component and still falls.  With sizes: sizes[root] += 1
// per pixel, reduced twice on the way (measured: one add per run left a map of two interleaved components with 2^20 adds
// on two words, 6 ms).  The pixels of one wave that sit next to each other with the same root (a run) add once, by the
// run's first lane; that add goes to a CNT_SLOTS-entry table in LDS keyed by the root (the first root to claim a slot
// owns it, a root that finds its slot taken adds to global memory directly), and the table is flushed with one global
// add per used slot.
constexpr int FLAT_PER_THREAD = 8, FLAT_PIX = POST_BLOCK * FLAT_PER_THREAD, CNT_SLOTS = 64;

__global__ __launch_bounds__(POST_BLOCK) void k_ccl_flatten(int* labels, int n, int* sizes) {
  __shared__ int slot_root[CNT_SLOTS];
  __shared__ int slot_count[CNT_SLOTS];
  if (sizes) {                                     // uniform
    if (threadIdx.x < CNT_SLOTS) { slot_root[threadIdx.x] = -1; slot_count[threadIdx.x] = 0; }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < FLAT_PER_THREAD; ++k) {
    const int i = blockIdx.x * FLAT_PIX + k * POST_BLOCK + threadIdx.x;      // < 2^28 + FLAT_PIX
    int root = -1;
    if (i < n) {
      root = glb_find(labels, i);
      __hip_atomic_store(labels + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!sizes) continue;
    const int prev = __shfl_up(root, 1);
    const bool head = lane == 0 || prev != root;
    const unsigned long long heads = __ballot(head);
    if (head && root >= 0) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;
      const int slot = (int)(((unsigned)root * 2654435761u) >> 26);         // 6 bits
      const int owner = atomicCAS(&slot_root[slot], -1, root);
      if (owner == -1 || owner == root) atomicAdd(&slot_count[slot], len);
      else atomicAdd(sizes + root, len);
    }
  }
  if (!sizes) return;
  __syncthreads();
  if (threadIdx.x < CNT_SLOTS && slot_count[threadIdx.x] > 0) atomicAdd(sizes + slot_root[threadIdx.x], slot_count[threadIdx.x]);
}

// A pixel of a small component offers each foreign, unfrozen, not-small component across one of its four edges:
// key = (donor size << 8) | (255 - donor value), the maximum wins -- the greatest size, then the smallest value.
__global__ __launch_bounds__(POST_BLOCK) void k_sieve_donor(const unsigned char* map, int H, int W, int min_pixels, int frozen,
                                                            const int* labels, const int* sizes, unsigned long long* keys) {
  const int n = H * W;
  const int i = blockIdx.x * POST_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int root = labels[i];
  if (sizes[root] >= min_pixels) return;
  const int v = map[i];
  if (v == frozen) return;
  const int y = i / W, x = i - y * W;
  unsigned long long best = 0ull;
  const int nb[4] = {x > 0 ? i - 1 : -1, x < W - 1 ? i + 1 : -1, y > 0 ? i - W : -1, y < H - 1 ? i + W : -1};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int j = nb[d];
    if (j < 0) continue;
    const int vj = map[j];
    if (vj == v || vj == frozen) continue;         // the same value across an edge is the same component
    const int sj = sizes[labels[j]];
    if (sj < min_pixels) continue;
    const unsigned long long key = ((unsigned long long)sj << 8) | (unsigned)(255 - vj);
    best = key > best ? key : best;
  }
  if (best) atomicMax(keys + root, best);
}

// out[i] = the donor's value where the pixel's component got one, else map[i] (only the pixel's own byte of map is read:
// safe in place).  stats[0] += components re-valued (counted by the thread on the root), stats[1] += pixels changed.
__global__ __launch_bounds__(POST_BLOCK) void k_sieve_apply(const unsigned char* map, unsigned char* out, int n, const int* labels,
                                                            const unsigned long long* keys, unsigned long long* stats) {
  __shared__ unsigned int acc[2];
  if (stats) {
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
  }
  const int i = blockIdx.x * POST_BLOCK + threadIdx.x;
  bool changed = false, is_root = false;
  if (i < n) {
    const int root = labels[i];
    const unsigned long long key = keys[root];
    unsigned char v = map[i];
    if (key) {
      v = (unsigned char)(255u - (unsigned)(key & 255ull));
      changed = true;
      is_root = root == i;
    }
    out[i] = v;
  }
  if (!stats) return;
  const unsigned long long bc = __ballot(changed), br = __ballot(is_root);
  if ((threadIdx.x & 63) == 0) {
    if (br) atomicAdd(&acc[0], (unsigned)__popcll(br));
    if (bc) atomicAdd(&acc[1], (unsigned)__popcll(bc));
  }
  __syncthreads();
  if (threadIdx.x < 2 && acc[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)acc[threadIdx.x]);
}

int launch_ccl(const unsigned char* map, int h, int w, int conn8, int* labels, int* sizes, unsigned long long* keys,
               hipStream_t s) {
  const int n = h * w;
  const int tiles_x = ceil_div(w, CCL_TILE), tiles_y = ceil_div(h, CCL_TILE);
  const int blocks = ceil_div(n, POST_BLOCK);
  hipLaunchKernelGGL(k_ccl_tile, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), 0, s, map, h, w, tiles_x, conn8,
                     labels, sizes, keys);
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ccl_seams, dim3(blocks), dim3(POST_BLOCK), 0, s, map, h, w, conn8, labels);
  FU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ccl_flatten, dim3(ceil_div(n, FLAT_PIX)), dim3(POST_BLOCK), 0, s, labels, n, sizes);
  FU_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int64_t sieve_workspace_bytes(int h, int w) { return 16 * (int64_t)h * w; }

int launch_map_components(const unsigned char* map, int h, int w, int connectivity, int* labels, hipStream_t s) {
  return launch_ccl(map, h, w, connectivity == 8, labels, nullptr, nullptr, s);
}

int launch_map_sieve(const unsigned char* map, unsigned char* out, int h, int w, int connectivity, int min_pixels, int frozen,
                     int passes, void* workspace, int64_t* stats, hipStream_t s) {
  const int n = h * w;
  if (min_pixels <= 1) {                           // nothing is small: a copy, zero stats
    if (out != map) FU_HIP_CHECK(hipMemcpyAsync(out, map, (size_t)n, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);      // [n] 64-bit donor keys
  int* labels = reinterpret_cast<int*>(keys + n);                              // [n]
  int* sizes = labels + n;                                                     // [n], read at the roots
  const int blocks = ceil_div(n, POST_BLOCK);
  for (int p = 0; p < passes; ++p) {
    const unsigned char* in = p == 0 ? map : out;
    FU_TRY(launch_ccl(in, h, w, connectivity == 8, labels, sizes, keys, s));
    hipLaunchKernelGGL(k_sieve_donor, dim3(blocks), dim3(POST_BLOCK), 0, s, in, h, w, min_pixels, frozen, labels, sizes, keys);
    FU_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sieve_apply, dim3(blocks), dim3(POST_BLOCK), 0, s, in, out, n, labels, keys,
                       reinterpret_cast<unsigned long long*>(stats));
    FU_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace fu
