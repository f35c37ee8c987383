// Post-processing of hard class maps on the device: connected-component labelling and the keep-largest-component filter of an
// evaluation pipeline (include/pacingpseudo_hip.h; DESIGN.md section 7, "Largest-component filter").  The reference scores its raw
// arg-max (inference.py:159-190); class maps are integers, so there is one build of this file in every storage mode.
//
// Two pixels of one image are connected when they are neighbours (4- or 8-neighbourhood) and hold the same value.  The label of a
// pixel is the smallest row-major index of its component, so the result is unique.  Structure: a union-find forest over pixel
// indices in which a parent is never larger than its child (roots are the minima, every walk towards a root descends and ends):
//   cc_tile_kernel     one 32 x 32 tile per block: union-find in LDS, then parent[p] = the tile-local root as an image index
//   cc_merge_kernel    one thread per pixel on a tile border line: lock-free unions on the global parent array
//   cc_flatten_kernel  labels[p] = root of p; component sizes and per-class component counts with integer atomics
//   cc_select_kernel   per (image, class): 64-bit atomicMax of size << 32 | ~label -- the largest, ties to the smallest label
//   cc_apply_kernel    out = cls where the pixel's component was selected (or the value is not a foreground class), else 0
// The launch sequence depends on the shape alone.  No block ever waits for another: the union is find both roots, atomicMin the
// larger root's parent to the smaller, go on from the returned value if another thread had moved that root meanwhile -- every
// retry strictly descends, so it ends on its own.  Phases are ordered by kernel boundaries; the one launch whose blocks race on
// global memory (cc_merge_kernel) touches the parent array through relaxed agent-scope atomics only (the eight XCDs' L2s are not
// coherent for plain loads).  Integer atomics only: the same bits in every run.
#include "pp_common.h"

#define CC_TW 32
#define CC_TH 32
#define CC_TILE (CC_TW * CC_TH)
#define CC_THREADS 256
#define CC_MAX_BLOCKS (1 << 20)          // larger problems walk with a grid stride
#define CC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define CC_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

typedef unsigned long long cc_u64;

// ---- union-find in LDS (one tile) ----
__device__ __forceinline__ int cc_find_lds(int* par, int i) {
  for (;;) {
    const int p = __hip_atomic_load(par + i, CC_RLX_WG);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void cc_union_lds(int* par, int a, int b) {
  for (;;) {
    a = cc_find_lds(par, a);
    b = cc_find_lds(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, CC_RLX_WG);
    if (old == a) return;                 // a was a root and now hangs below b
    a = old;                              // a had been moved below `old` meanwhile: join old and b instead (old < a)
  }
}
// ---- the same on the global parent array, while other blocks write it ----
__device__ __forceinline__ int cc_find_agent(int* par, int i) {
  for (;;) {
    const int p = __hip_atomic_load(par + i, CC_RLX_AGENT);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void cc_union_agent(int* par, int a, int b) {
  for (;;) {
    a = cc_find_agent(par, a);
    b = cc_find_agent(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, CC_RLX_AGENT);
    if (old == a) return;
    a = old;
  }
}

// parent: [N][H*W] image-local indices.  size (COUNT): zeroed here for cc_flatten_kernel.
template <bool COUNT>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const long long* __restrict__ cls, int H, int W, int tiles_x, int tiles_y,
                                                             long long ntiles, int conn8, int* __restrict__ parent,
                                                             int* __restrict__ size) {
  __shared__ long long s_val[CC_TILE];
  __shared__ int s_par[CC_TILE];
  const int per_image = tiles_x * tiles_y;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = (int)(t / per_image), r = (int)(t % per_image);
    const int y0 = (r / tiles_x) * CC_TH, x0 = (r % tiles_x) * CC_TW;
    const size_t base = (size_t)n * H * W;
    __syncthreads();                                            // the previous tile of this block has been written out
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
      const int y = y0 + i / CC_TW, x = x0 + i % CC_TW;
      s_val[i] = (y < H && x < W) ? cls[base + (size_t)y * W + x] : 0;
      s_par[i] = i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
      const int ly = i / CC_TW, lx = i % CC_TW;
      if (y0 + ly >= H || x0 + lx >= W) continue;               // the left / upper neighbours of a pixel inside the image are inside
      const long long v = s_val[i];
      if (lx > 0 && s_val[i - 1] == v) cc_union_lds(s_par, i, i - 1);
      if (ly > 0) {
        if (s_val[i - CC_TW] == v) cc_union_lds(s_par, i, i - CC_TW);
        if (conn8) {
          if (lx > 0 && s_val[i - CC_TW - 1] == v) cc_union_lds(s_par, i, i - CC_TW - 1);
          if (lx < CC_TW - 1 && x0 + lx + 1 < W && s_val[i - CC_TW + 1] == v) cc_union_lds(s_par, i, i - CC_TW + 1);
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
      const int y = y0 + i / CC_TW, x = x0 + i % CC_TW;
      if (y >= H || x >= W) continue;
      const int root = cc_find_lds(s_par, i);                   // tile order and image order agree: the minimum stays the minimum
      const size_t g = base + (size_t)y * W + x;
      parent[g] = (y0 + root / CC_TW) * W + x0 + root % CC_TW;
      if (COUNT) size[g] = 0;
    }
  }
}

// Border lines per image: rows y = 32, 64, ... (nh of them, W pixels each: joined with the row above) and columns x = 32, 64, ...
// (nv of them, H pixels each: joined with the column to the left).  Under the 8-neighbourhood a row pixel also looks up-left and
// up-right, a column pixel up-left and down-left: together every neighbour pair that straddles a tile border.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const long long* __restrict__ cls, int H, int W, int nh, int nv,
                                                              long long total, int conn8, int* parent) {
  const int per_image = nh * W + nv * H;
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * CC_THREADS) {
    const int n = (int)(g / per_image);
    int e = (int)(g % per_image);
    const long long* c = cls + (size_t)n * H * W;
    int* par = parent + (size_t)n * H * W;
    if (e < nh * W) {
      const int y = (e / W + 1) * CC_TH, x = e % W, p = y * W + x;
      const long long v = c[p];
      if (c[p - W] == v) cc_union_agent(par, p, p - W);
      if (conn8) {
        if (x > 0 && c[p - W - 1] == v) cc_union_agent(par, p, p - W - 1);
        if (x + 1 < W && c[p - W + 1] == v) cc_union_agent(par, p, p - W + 1);
      }
    } else {
      e -= nh * W;
      const int x = (e / H + 1) * CC_TW, y = e % H, p = y * W + x;
      const long long v = c[p];
      if (c[p - 1] == v) cc_union_agent(par, p, p - 1);
      if (conn8) {
        if (y > 0 && c[p - W - 1] == v) cc_union_agent(par, p, p - W - 1);
        if (y + 1 < H && c[p + W - 1] == v) cc_union_agent(par, p, p + W - 1);
      }
    }
  }
}

// labels[g] = root of pixel g (the parent array is final: plain loads behind the kernel boundary).  COUNT: size[root] += 1 per pixel
// -- one atomic per run of equal roots inside a wave, so a component that fills rows costs one add per 64 pixels -- and
// ncomp[n][k] += 1 per root of a foreground class.
template <bool COUNT>
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const long long* __restrict__ cls, const int* __restrict__ parent, int HW,
                                                                long long total, int K, int* __restrict__ labels, int* __restrict__ size,
                                                                int* __restrict__ ncomp) {
  for (long long b0 = (long long)blockIdx.x * CC_THREADS; b0 < total; b0 += (long long)gridDim.x * CC_THREADS) {
    const long long g = b0 + threadIdx.x;
    const bool active = g < total;
    int n = 0, p = 0, root = 0;
    if (active) {
      n = (int)(g / HW);
      p = (int)(g % HW);
      const int* par = parent + (size_t)n * HW;
      root = p;
      for (;;) {
        const int q = par[root];
        if (q == root) break;
        root = q;
      }
      labels[g] = root;
    }
    if (COUNT) {
      const long long key = active ? g - p + root : -1;          // the root as an index into the whole batch
      const int lane = threadIdx.x & 63;
      const long long prev = __shfl_up(key, 1, 64);
      const bool lead = lane == 0 || prev != key;
      const cc_u64 leaders = __ballot(lead);
      if (lead && active) {
        const cc_u64 above = lane == 63 ? 0ull : leaders >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : 64 - lane;      // lanes up to the next leader
        atomicAdd(&size[key], run);
      }
      if (active && root == p) {
        const long long v = cls[g];
        if (v >= 1 && v < K) atomicAdd(&ncomp[n * K + (int)v], 1);
      }
    }
  }
}

// best[n][k] = max over the components of class k of (size << 32 | ~label): the largest, and of equals the smallest label
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(const long long* __restrict__ cls, const int* __restrict__ labels,
                                                               const int* __restrict__ size, int HW, long long total, int K,
                                                               cc_u64* __restrict__ best) {
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * CC_THREADS) {
    const int n = (int)(g / HW), p = (int)(g % HW);
    if (labels[g] != p) continue;
    const long long v = cls[g];
    if (v >= 1 && v < K) atomicMax(&best[n * K + (int)v], ((cc_u64)(unsigned)size[g] << 32) | (cc_u64)(~(unsigned)p));
  }
}

// cls and out may be the same array: every pixel is read and written by one thread
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const long long* cls, const int* __restrict__ labels,
                                                              const cc_u64* __restrict__ best, const int* __restrict__ ncomp, int HW,
                                                              long long total, long long items, int K, long long* out,
                                                              int* __restrict__ stats) {
  const long long span = total > items ? total : items;
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < span; g += (long long)gridDim.x * CC_THREADS) {
    if (g < total) {
      const long long v = cls[g];
      long long o = v;
      if (v >= 1 && v < K) {
        const cc_u64 b = best[(g / HW) * K + v];
        if (~(unsigned)b != (unsigned)labels[g]) o = 0;
      }
      out[g] = o;
    }
    if (g < items) {                                              // items = N * K; class 0 was never counted: {0, 0}
      stats[2 * g] = ncomp[g];
      stats[2 * g + 1] = (int)(best[g] >> 32);
    }
  }
}

// ---- host side ----
static inline size_t cc_pad16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline size_t cc_head_bytes(int N, int K) { return cc_pad16((size_t)N * K * (sizeof(cc_u64) + sizeof(int))); }

extern "C" size_t pp_components_workspace(int N, int K, int H, int W) {
  if (N < 1 || K < 1 || H < 1 || W < 1) return 0;
  return 16 + cc_head_bytes(N, K) + 3 * cc_pad16((size_t)N * H * W * sizeof(int));
}

struct CcWs {
  cc_u64* best;       // [N][K]
  int* ncomp;         // [N][K]
  int* parent;        // [N][H*W]
  int* size;          // [N][H*W], meaningful at roots
  int* labels;        // [N][H*W]
  size_t head;        // bytes of best + ncomp, zeroed per call
};
static CcWs cc_carve(void* workspace, int N, int K, int H, int W) {
  CcWs w;
  char* p = reinterpret_cast<char*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  const size_t px = cc_pad16((size_t)N * H * W * sizeof(int));
  w.head = cc_head_bytes(N, K);
  w.best = reinterpret_cast<cc_u64*>(p);
  w.ncomp = reinterpret_cast<int*>(p + (size_t)N * K * sizeof(cc_u64));
  w.parent = reinterpret_cast<int*>(p + w.head);
  w.size = reinterpret_cast<int*>(p + w.head + px);
  w.labels = reinterpret_cast<int*>(p + w.head + 2 * px);
  return w;
}
static inline int cc_blocks(long long threads) {
  const long long b = (threads + CC_THREADS - 1) / CC_THREADS;
  return (int)(b < CC_MAX_BLOCKS ? b : CC_MAX_BLOCKS);
}

// tile + merge launches: parent = the forest of the whole batch
template <bool COUNT>
static void cc_build_forest(const long long* cls, int N, int H, int W, int conn8, int* parent, int* size, hipStream_t s) {
  const int tiles_x = pp_cdiv(W, CC_TW), tiles_y = pp_cdiv(H, CC_TH);
  const long long ntiles = (long long)N * tiles_x * tiles_y;
  hipLaunchKernelGGL(cc_tile_kernel<COUNT>, dim3((unsigned)(ntiles < CC_MAX_BLOCKS ? ntiles : CC_MAX_BLOCKS)), dim3(CC_THREADS), 0, s, cls, H, W,
                     tiles_x, tiles_y, ntiles, conn8, parent, size);
  const int nh = (H - 1) / CC_TH, nv = (W - 1) / CC_TW;
  const long long border = (long long)N * ((long long)nh * W + (long long)nv * H);
  if (border > 0)
    hipLaunchKernelGGL(cc_merge_kernel, dim3(cc_blocks(border)), dim3(CC_THREADS), 0, s, cls, H, W, nh, nv, border, conn8, parent);
}

extern "C" int pp_label_components(const int64_t* cls, int N, int H, int W, int connectivity, int32_t* labels, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(cls && labels && workspace, "label_components: null pointer");
  PP_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "label_components: bad shape N=%d H=%d W=%d", N, H, W);
  PP_CHECK_ARG(connectivity == 1 || connectivity == 2, "label_components: connectivity=%d (1: 4-neighbourhood, 2: 8-neighbourhood)", connectivity);
  PP_CHECK_ARG((long long)N * H * W < 0x80000000LL, "label_components: N*H*W must be below 2^31");
  if (workspace_bytes < pp_components_workspace(N, 1, H, W)) {
    pp_set_error("label_components: workspace too small (%zu < %zu)", workspace_bytes, pp_components_workspace(N, 1, H, W));
    return PP_ERR_WORKSPACE;
  }
  const CcWs w = cc_carve(workspace, N, 1, H, W);
  const long long total = (long long)N * H * W;
  pp_prof_begin(PP_K_MISC, 0.0, 24.0 * (double)total, s);
  cc_build_forest<false>((const long long*)cls, N, H, W, connectivity == 2, w.parent, nullptr, s);
  hipLaunchKernelGGL(cc_flatten_kernel<false>, dim3(cc_blocks(total)), dim3(CC_THREADS), 0, s, (const long long*)cls, w.parent, H * W, total, 1,
                     labels, nullptr, nullptr);
  pp_prof_end(s);
  return pp_launch_status("label_components");
}

extern "C" int pp_keep_largest_components(const int64_t* cls, int N, int K, int H, int W, int connectivity, int64_t* out, int32_t* stats,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(cls && out && stats && workspace, "keep_largest_components: null pointer");
  PP_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "keep_largest_components: bad shape N=%d H=%d W=%d", N, H, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "keep_largest_components: K=%d (1..%d)", K, PP_MAXK);
  PP_CHECK_ARG(connectivity == 1 || connectivity == 2, "keep_largest_components: connectivity=%d (1: 4-neighbourhood, 2: 8-neighbourhood)",
               connectivity);
  PP_CHECK_ARG((long long)N * H * W < 0x80000000LL, "keep_largest_components: N*H*W must be below 2^31");
  if (workspace_bytes < pp_components_workspace(N, K, H, W)) {
    pp_set_error("keep_largest_components: workspace too small (%zu < %zu)", workspace_bytes, pp_components_workspace(N, K, H, W));
    return PP_ERR_WORKSPACE;
  }
  const CcWs w = cc_carve(workspace, N, K, H, W);
  const long long total = (long long)N * H * W, items = (long long)N * K;
  hipError_t e = hipMemsetAsync(w.best, 0, w.head, s);
  if (e != hipSuccess) {
    pp_set_error("keep_largest_components: hipMemsetAsync: %s", hipGetErrorString(e));
    return (int)e;
  }
  pp_prof_begin(PP_K_MISC, 0.0, 72.0 * (double)total, s);
  cc_build_forest<true>((const long long*)cls, N, H, W, connectivity == 2, w.parent, w.size, s);
  hipLaunchKernelGGL(cc_flatten_kernel<true>, dim3(cc_blocks(total)), dim3(CC_THREADS), 0, s, (const long long*)cls, w.parent, H * W, total, K,
                     w.labels, w.size, w.ncomp);
  hipLaunchKernelGGL(cc_select_kernel, dim3(cc_blocks(total)), dim3(CC_THREADS), 0, s, (const long long*)cls, w.labels, w.size, H * W, total, K,
                     w.best);
  hipLaunchKernelGGL(cc_apply_kernel, dim3(cc_blocks(total > items ? total : items)), dim3(CC_THREADS), 0, s, (const long long*)cls, w.labels,
                     w.best, w.ncomp, H * W, total, items, K, (long long*)out, stats);
  pp_prof_end(s);
  return pp_launch_status("keep_largest_components");
}
