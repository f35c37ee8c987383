// Post-processing of hard class maps on the device: connected-component labelling and the keep-largest-component filter of an
// evaluation pipeline (include/pacingpseudo_hip.h; DESIGN.md section 7, "Largest-component filter").  The reference scores its raw
// arg-max (inference.py:159-190); class maps are integers, so there is one build of this file in every storage mode.  The second
// half of the file holds the test-time-augmentation kernels (views, soft-max accumulation, finalize) on the fp32 logits, then
// the reduction of the surface-distance sets to the numbers HD, ASSD, surface Dice and a percentile distance are made of, the end
// the mean-field CRF refinement of the soft-max (one launch per iteration on the fp32 logits and the image).
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

// ================================================================================================================================
// Test-time augmentation over the dihedral group (include/pacingpseudo_hip.h; DESIGN.md section 7, "Test-time augmentation").
// op: bit 0 flips W, bit 1 flips H, bit 2 transposes; the forward view of a[H][W] is transpose, then flip H, then flip W, so the view
// pixel (i, j) of a view of shape (Hv, Wv) -- (W, H) under bit 2, else (H, W) -- is the source pixel
//   i2 = op & 2 ? Hv - 1 - i : i,  j2 = op & 1 ? Wv - 1 - j : j,  (y, x) = op & 4 ? (j2, i2) : (i2, j2).
//   tta_view_*_kernel   out[view pixel] = x[source pixel]                                   per plane
//   tta_acc_*_kernel    acc[k][source pixel] (+)= softmax_k(logits[.][view pixel])          the K values of a pixel in registers
//   tta_finalize_kernel acc *= 1 / views, cls = first-maximum arg-max of the scaled values
// Ops without bit 2 (*_row_kernel): a thread takes 4 consecutive pixels of a row (16-byte accesses) when W % 4 == 0 and the pointers
// are 16-byte aligned, one pixel otherwise; under a W flip lane l + 1 reads / writes the vector (or word) just below lane l's and the
// vector is reversed, so both global sides are runs of consecutive addresses.
// Ops with bit 2 (*_tile_kernel): a block owns a 32 x 32 pixel tile.  Each thread loads its pixels along the rows of the side it
// reads (32 lanes = 128 consecutive bytes), the planes go through LDS tiles of 32 rows x 33 words and come back transposed, so the
// other side is walked along ITS rows, 128 consecutive bytes per 32 lanes again.  Bank rule (ds_write_b32 / ds_read_b32: bank =
// word address % 32, conflicts inside a 32-lane half): the write of a half is row r, columns 0 .. 31 -> banks (33 r + c) % 32, 32
// different ones; the read is rows 0 .. 31 of column c -> banks (33 l + c) % 32 = (l + c) % 32, 32 different ones: 0 extra cycles
// on either side (an unpadded row of 32 words would put the whole read on one bank: 32-way).
// No atomics, no host synchronisation, a launch fixed by the shape and op; every acc element is touched by exactly one thread per
// launch and the views are added in the caller's order: the same bits in every run.
#define TTA_THREADS 256
#define TTA_TILE 32
#define TTA_LD (TTA_TILE + 1)
#define TTA_ROWS (TTA_THREADS / TTA_TILE)            // tile rows one pass of the block covers: 8
#define TTA_PER (TTA_TILE / TTA_ROWS)                // pixels per thread: 4
#define TTA_CHUNK 8                                  // planes in LDS at a time: 8 x 32 x 33 x 4 B = 33 KiB, four blocks per CU
#define TTA_MAX_BLOCKS (1 << 20)

__device__ __forceinline__ int tta_flip(int v, int n, int on) { return on ? n - 1 - v : v; }

// the soft-max of one pixel in place, the maximum subtracted
template <int MK>
__device__ __forceinline__ void tta_softmax(float (&v)[MK], int K) {
  float m = v[0];
#pragma unroll
  for (int k = 1; k < MK; ++k)
    if (k < K) m = fmaxf(m, v[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) { v[k] = expf(v[k] - m); s += v[k]; }
  const float inv = 1.f / s;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) v[k] *= inv;
}

__device__ __forceinline__ float4 tta_rev4(float4 v, int on) { return on ? make_float4(v.w, v.z, v.y, v.x) : v; }

// ---- ops 0 .. 3: rows stay rows ----
// x, out: [planes][H][W]
template <bool VEC>
__global__ __launch_bounds__(TTA_THREADS) void tta_view_row_kernel(const float* __restrict__ x, int H, int W, int op, long long total,
                                                                   float* __restrict__ out) {
  const int Wq = VEC ? W / 4 : W;                                       // items per row
  for (long long g = (long long)blockIdx.x * TTA_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * TTA_THREADS) {
    const long long row = g / Wq;                                        // plane * H + i
    const int q = (int)(g - row * Wq), i = (int)(row % H);
    const long long src_row = row - i + tta_flip(i, H, op & 2);
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(x + src_row * W + 4 * tta_flip(q, Wq, op & 1));
      *reinterpret_cast<float4*>(out + row * W + 4 * q) = tta_rev4(v, op & 1);
    } else {
      out[row * W + q] = x[src_row * W + tta_flip(q, W, op & 1)];
    }
  }
}

// logits, acc: [N][K][H][W]; total = N * H * (VEC ? W / 4 : W)
template <int MK, bool VEC>
__global__ __launch_bounds__(TTA_THREADS) void tta_acc_row_kernel(const float* __restrict__ logits, int K, int H, int W, int op, int first,
                                                                  long long total, float* __restrict__ acc) {
  const int Wq = VEC ? W / 4 : W;
  const size_t HW = (size_t)H * W;
  for (long long g = (long long)blockIdx.x * TTA_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * TTA_THREADS) {
    const long long row = g / Wq;                                        // n * H + i
    const int q = (int)(g - row * Wq), n = (int)(row / H), i = (int)(row - (long long)n * H);
    const float* src = logits + (size_t)n * K * HW + (size_t)i * W + (VEC ? 4 * q : q);
    float* dst = acc + (size_t)n * K * HW + (size_t)tta_flip(i, H, op & 2) * W + (VEC ? 4 : 1) * tta_flip(q, Wq, op & 1);
    if (VEC) {
      float a[MK], b[MK], c[MK], d[MK];
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) {
          const float4 v = *reinterpret_cast<const float4*>(src + k * HW);
          a[k] = v.x; b[k] = v.y; c[k] = v.z; d[k] = v.w;
        }
      tta_softmax(a, K); tta_softmax(b, K); tta_softmax(c, K); tta_softmax(d, K);
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) {
          float4 p = tta_rev4(make_float4(a[k], b[k], c[k], d[k]), op & 1);
          float4* o = reinterpret_cast<float4*>(dst + k * HW);
          if (!first) { const float4 t = *o; p = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w); }
          *o = p;
        }
    } else {
      float v[MK];
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) v[k] = src[k * HW];
      tta_softmax(v, K);
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) dst[k * HW] = first ? v[k] : dst[k * HW] + v[k];
    }
  }
}

// ---- ops 4 .. 7: through an LDS tile transpose ----
// x: [planes][H][W] -> out: [planes][W][H].  The block reads source rows y0 + r, columns x0 .. x0 + 31 and writes view rows: the
// source pixel (y, x) is the view pixel (i, j) with i2 = x, j2 = y.
__global__ __launch_bounds__(TTA_THREADS) void tta_view_tile_kernel(const float* __restrict__ x, int H, int W, int op, int tiles_x,
                                                                    int tiles_y, long long ntiles, float* __restrict__ out) {
  __shared__ float s[TTA_TILE * TTA_LD];
  const int tx = threadIdx.x % TTA_TILE, ty = threadIdx.x / TTA_TILE;
  const int per_plane = tiles_x * tiles_y;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long plane = t / per_plane;
    const int r = (int)(t - plane * per_plane), y0 = (r / tiles_x) * TTA_TILE, x0 = (r % tiles_x) * TTA_TILE;
    const float* src = x + (size_t)plane * H * W;
    float* dst = out + (size_t)plane * H * W;
    __syncthreads();                                                     // the previous tile of this block has been read out
#pragma unroll
    for (int e = 0; e < TTA_PER; ++e) {
      const int ly = ty + e * TTA_ROWS;
      if (y0 + ly < H && x0 + tx < W) s[ly * TTA_LD + tx] = src[(size_t)(y0 + ly) * W + x0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < TTA_PER; ++e) {
      const int lx = ty + e * TTA_ROWS;                                  // source column = view row (before the flip)
      const int sx = x0 + lx, sy = y0 + tx;
      if (sx < W && sy < H) dst[(size_t)tta_flip(sx, W, op & 2) * H + tta_flip(sy, H, op & 1)] = s[tx * TTA_LD + lx];
    }
  }
}

// logits: [N][K][W][H] (the view), acc: [N][K][H][W].  The block reads view rows i0 + r, columns j0 .. j0 + 31; the view pixel
// (i, j) lands on acc row y = j2, column x = i2.
template <int MK>
__global__ __launch_bounds__(TTA_THREADS) void tta_acc_tile_kernel(const float* __restrict__ logits, int K, int H, int W, int op,
                                                                   int first, int tiles_x, int tiles_y, long long ntiles,
                                                                   float* __restrict__ acc) {
  __shared__ float s[TTA_CHUNK * TTA_TILE * TTA_LD];
  const int Hv = W, Wv = H;
  const int tx = threadIdx.x % TTA_TILE, ty = threadIdx.x / TTA_TILE;
  const int per_image = tiles_x * tiles_y;
  const size_t HW = (size_t)H * W;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = (int)(t / per_image), r = (int)(t - (long long)n * per_image);
    const int i0 = (r / tiles_x) * TTA_TILE, j0 = (r % tiles_x) * TTA_TILE;
    const float* src = logits + (size_t)n * K * HW;
    float* dst = acc + (size_t)n * K * HW;
    float v[TTA_PER][MK];
#pragma unroll
    for (int e = 0; e < TTA_PER; ++e) {
      const int i = i0 + ty + e * TTA_ROWS, j = j0 + tx;
      const bool in = i < Hv && j < Wv;
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) v[e][k] = in ? src[k * HW + (size_t)i * Wv + j] : 0.f;
      tta_softmax(v[e], K);
    }
#pragma unroll
    for (int c0 = 0; c0 < MK; c0 += TTA_CHUNK) {
      if (c0 < K) {                                                      // uniform over the block
        __syncthreads();                                                 // the previous chunk / tile has been read out
#pragma unroll
        for (int c = 0; c < TTA_CHUNK; ++c)
          if (c0 + c < MK && c0 + c < K) {
#pragma unroll
            for (int e = 0; e < TTA_PER; ++e) s[(c * TTA_TILE + ty + e * TTA_ROWS) * TTA_LD + tx] = v[e][c0 + c];
          }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < TTA_PER; ++e) {
          const int lj = ty + e * TTA_ROWS;                              // view column = acc row (before the flip)
          const int i = i0 + tx, j = j0 + lj;
          if (i < Hv && j < Wv) {
            float* o = dst + (size_t)tta_flip(j, Wv, op & 1) * W + tta_flip(i, Hv, op & 2);
#pragma unroll
            for (int c = 0; c < TTA_CHUNK; ++c)
              if (c0 + c < MK && c0 + c < K) {
                const float p = s[(c * TTA_TILE + tx) * TTA_LD + lj];
                o[(c0 + c) * HW] = first ? p : o[(c0 + c) * HW] + p;
              }
          }
        }
      }
    }
  }
}

// acc: [N][K][HW] scaled in place; cls (nullable): [N][HW].  total = N * (VEC ? HW / 4 : HW)
template <bool VEC>
__global__ __launch_bounds__(TTA_THREADS) void tta_finalize_kernel(float* __restrict__ acc, int K, int HW, float scale, long long total,
                                                                   long long* __restrict__ cls) {
  const int per = VEC ? HW / 4 : HW;
  for (long long g = (long long)blockIdx.x * TTA_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * TTA_THREADS) {
    const int n = (int)(g / per), q = (int)(g - (long long)n * per);
    float* b = acc + (size_t)n * K * HW + (VEC ? 4 * q : q);
    if (VEC) {
      float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
      int kx = 0, ky = 0, kz = 0, kw = 0;
      for (int k = 0; k < K; ++k) {
        float4 v = *reinterpret_cast<float4*>(b + (size_t)k * HW);
        v = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
        *reinterpret_cast<float4*>(b + (size_t)k * HW) = v;
        if (k == 0) m = v;
        if (v.x > m.x) { m.x = v.x; kx = k; }
        if (v.y > m.y) { m.y = v.y; ky = k; }
        if (v.z > m.z) { m.z = v.z; kz = k; }
        if (v.w > m.w) { m.w = v.w; kw = k; }
      }
      if (cls) {
        longlong2* o = reinterpret_cast<longlong2*>(cls + (size_t)n * HW + 4 * q);      // HW % 4 == 0: 32-byte aligned with cls
        o[0] = make_longlong2(kx, ky);
        o[1] = make_longlong2(kz, kw);
      }
    } else {
      float m = 0.f;
      int best = 0;
      for (int k = 0; k < K; ++k) {
        const float v = b[(size_t)k * HW] * scale;
        b[(size_t)k * HW] = v;
        if (k == 0) m = v;
        if (v > m) { m = v; best = k; }
      }
      if (cls) cls[(size_t)n * HW + q] = best;
    }
  }
}

// ---- host side ----
static inline int tta_blocks(long long items) {
  const long long b = (items + TTA_THREADS - 1) / TTA_THREADS;
  return (int)(b < TTA_MAX_BLOCKS ? b : TTA_MAX_BLOCKS);
}
static inline bool tta_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int pp_tta_view(const float* x, int planes, int H, int W, int op, float* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(x && out, "tta_view: null pointer");
  PP_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1, "tta_view: bad shape planes=%d H=%d W=%d", planes, H, W);
  PP_CHECK_ARG(op >= 0 && op <= 7, "tta_view: op=%d (0..7: bit 0 flips W, bit 1 flips H, bit 2 transposes)", op);
  PP_CHECK_ARG((long long)planes * H * W < 0x80000000LL, "tta_view: planes*H*W must be below 2^31");
  const long long total = (long long)planes * H * W;
  PP_CHECK_ARG(out + total <= x || x + total <= out, "tta_view: out must not overlap x");
  pp_prof_begin(PP_K_MISC, 0.0, 8.0 * (double)total, s);
  if (op & 4) {
    const int tiles_x = pp_cdiv(W, TTA_TILE), tiles_y = pp_cdiv(H, TTA_TILE);
    const long long ntiles = (long long)planes * tiles_x * tiles_y;
    hipLaunchKernelGGL(tta_view_tile_kernel, dim3((unsigned)(ntiles < TTA_MAX_BLOCKS ? ntiles : TTA_MAX_BLOCKS)), dim3(TTA_THREADS), 0, s, x, H,
                       W, op, tiles_x, tiles_y, ntiles, out);
  } else if (W % 4 == 0 && tta_al16(x) && tta_al16(out)) {
    hipLaunchKernelGGL(tta_view_row_kernel<true>, dim3(tta_blocks(total / 4)), dim3(TTA_THREADS), 0, s, x, H, W, op, total / 4, out);
  } else {
    hipLaunchKernelGGL(tta_view_row_kernel<false>, dim3(tta_blocks(total)), dim3(TTA_THREADS), 0, s, x, H, W, op, total, out);
  }
  pp_prof_end(s);
  return pp_launch_status("tta_view");
}

extern "C" int pp_tta_accumulate(const float* logits, int N, int K, int H, int W, int op, int first, float* acc, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && acc, "tta_accumulate: null pointer");
  PP_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "tta_accumulate: bad shape N=%d H=%d W=%d", N, H, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "tta_accumulate: K=%d (1..%d)", K, PP_MAXK);
  PP_CHECK_ARG(op >= 0 && op <= 7, "tta_accumulate: op=%d (0..7: bit 0 flips W, bit 1 flips H, bit 2 transposes)", op);
  PP_CHECK_ARG((long long)N * K * H * W < 0x80000000LL, "tta_accumulate: N*K*H*W must be below 2^31");
  const long long px = (long long)N * H * W;
  pp_prof_begin(PP_K_MISC, 0.0, (first ? 8.0 : 12.0) * (double)px * K, s);
  if (op & 4) {
    const int tiles_x = pp_cdiv(H, TTA_TILE), tiles_y = pp_cdiv(W, TTA_TILE);      // of the view: W rows of H pixels
    const long long ntiles = (long long)N * tiles_x * tiles_y;
    const dim3 grid((unsigned)(ntiles < TTA_MAX_BLOCKS ? ntiles : TTA_MAX_BLOCKS));
    pp_by_class_bound(K, [&](auto mk) {
      hipLaunchKernelGGL(tta_acc_tile_kernel<decltype(mk)::value>, grid, dim3(TTA_THREADS), 0, s, logits, K, H, W, op, first, tiles_x, tiles_y,
                         ntiles, acc);
    });
  } else if (W % 4 == 0 && tta_al16(logits) && tta_al16(acc)) {
    pp_by_class_bound(K, [&](auto mk) {
      hipLaunchKernelGGL((tta_acc_row_kernel<decltype(mk)::value, true>), dim3(tta_blocks(px / 4)), dim3(TTA_THREADS), 0, s, logits, K, H, W, op,
                         first, px / 4, acc);
    });
  } else {
    pp_by_class_bound(K, [&](auto mk) {
      hipLaunchKernelGGL((tta_acc_row_kernel<decltype(mk)::value, false>), dim3(tta_blocks(px)), dim3(TTA_THREADS), 0, s, logits, K, H, W, op,
                         first, px, acc);
    });
  }
  pp_prof_end(s);
  return pp_launch_status("tta_accumulate");
}

extern "C" int pp_tta_finalize(float* acc, int N, int K, int H, int W, int views, int64_t* cls, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(acc, "tta_finalize: null pointer");
  PP_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "tta_finalize: bad shape N=%d H=%d W=%d", N, H, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "tta_finalize: K=%d (1..%d)", K, PP_MAXK);
  PP_CHECK_ARG(views == 1 || views == 2 || views == 4 || views == 8, "tta_finalize: views=%d (1, 2, 4 or 8)", views);
  PP_CHECK_ARG((long long)N * K * H * W < 0x80000000LL, "tta_finalize: N*K*H*W must be below 2^31");
  const long long px = (long long)N * H * W;
  const int HW = H * W;
  const float scale = 1.f / (float)views;
  pp_prof_begin(PP_K_MISC, 0.0, (8.0 * K + (cls ? 8.0 : 0.0)) * (double)px, s);
  if (HW % 4 == 0 && tta_al16(acc) && (!cls || tta_al16(cls)))
    hipLaunchKernelGGL(tta_finalize_kernel<true>, dim3(tta_blocks(px / 4)), dim3(TTA_THREADS), 0, s, acc, K, HW, scale, px / 4, (long long*)cls);
  else
    hipLaunchKernelGGL(tta_finalize_kernel<false>, dim3(tta_blocks(px)), dim3(TTA_THREADS), 0, s, acc, K, HW, scale, px, (long long*)cls);
  pp_prof_end(s);
  return pp_launch_status("tta_finalize");
}

// ================================================================================================================================
// Surface-distance reduction (include/pacingpseudo_hip.h; DESIGN.md section 7, "Surface metrics").  pp_hd95_surface_distances leaves
// two directed distance sets A and B per (slice, class) item; HD, ASSD, the surface Dice and a percentile distance are functions of
// eight numbers per item: max(S), sum(A), sum(B), |{a <= tol}|, |{b <= tol}|, S[j], S[min(j + 1, n - 1)], n with S = sort(A ++ B).
//   surface_reduce_kernel   one block of 256 threads per item, no workspace, nothing written but the 64 bytes of out[item]
// Distances are non-negative finite floats, so their bit patterns order as unsigned integers: S[j] comes from a most-significant-
// digit radix select -- four passes over the item's two segments, each a 256-bin histogram of one byte of the elements that still
// match the prefix found so far (integer LDS atomics), a block-wide scan of the bins, and the bin that holds rank j becomes the next
// byte of the prefix.  `below` = the elements strictly smaller than every value of the prefix; after the last pass the prefix is the
// bit pattern of S[j] and its bin holds the copies of that value, so S[j + 1] = S[j] when below + copies >= j + 2 and otherwise the
// minimum of the elements above S[j], which one more pass finds.  The first pass also takes the maximum (as bits), the within-
// tolerance counts (fp32 `<=`) and the two sums: per-thread strided partials in double, then a fixed halving tree through LDS.
// Integer atomics only and a fixed summation order: the same bits in every run.  The launch depends on `items` alone.
#define SR_THREADS 256
#define SR_WAVES (SR_THREADS / 64)

struct SrItem {
  const unsigned* a;      // the bit patterns of the first set
  const unsigned* b;
  int na, n;
  __device__ __forceinline__ unsigned at(int e) const { return e < na ? a[e] : b[e - na]; }
};

// Rank `rank` (counted among the elements the histogram holds) falls into the bin t with excl(t) <= rank < incl(t).  That thread
// publishes {t, excl, hist[t]}; everybody returns them.  Two barriers inside, and one in front so that the histogram is complete.
__device__ __forceinline__ void sr_select_bin(const unsigned* s_hist, unsigned* s_wave, unsigned* s_pick, unsigned rank, unsigned& bin,
                                              unsigned& excl_out, unsigned& copies) {
  __syncthreads();
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned h = s_hist[t];
  unsigned incl = h;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned base = 0;
#pragma unroll
  for (int w = 0; w < SR_WAVES; ++w)
    if (w < wave) base += s_wave[w];
  incl += base;
  const unsigned excl = incl - h;
  if (excl <= rank && rank < incl) { s_pick[0] = (unsigned)t; s_pick[1] = excl; s_pick[2] = h; }      // h > 0: exactly one thread
  __syncthreads();
  bin = s_pick[0];
  excl_out = s_pick[1];
  copies = s_pick[2];
}

__global__ __launch_bounds__(SR_THREADS) void surface_reduce_kernel(const float* __restrict__ dist, const int* __restrict__ counts, int cap,
                                                                    double quantile, float tolerance, double* __restrict__ out) {
  __shared__ unsigned s_hist[SR_THREADS];
  __shared__ double s_sum[2][SR_THREADS];
  __shared__ unsigned s_wave[SR_WAVES];
  __shared__ unsigned s_pick[3];
  __shared__ unsigned s_misc[4];                                   // max bits, count a, count b, min above S[j]
  const int item = blockIdx.x, t = threadIdx.x;
  double* o = out + (size_t)item * 8;
  SrItem it;
  it.na = min(max(counts[(size_t)item * 4], 0), cap);
  const int nb = min(max(counts[(size_t)item * 4 + 1], 0), cap);
  it.n = it.na + nb;
  it.a = reinterpret_cast<const unsigned*>(dist) + (size_t)item * 2 * cap;
  it.b = it.a + cap;
  const int n = it.n;
  if (n == 0) {                                                    // uniform over the block
    if (t < 8) o[t] = 0.0;
    return;
  }
  const double v = (double)(n - 1) * quantile;                     // numpy.percentile's virtual index; quantile <= 1, so v <= n - 1
  const int j = min(max((int)floor(v), 0), n - 1);

  // ---- pass 0: the top byte, and everything that needs every element once ----
  s_hist[t] = 0;
  if (t < 4) s_misc[t] = t == 3 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  {
    double sa = 0.0, sb = 0.0;
    unsigned mx = 0, ca = 0, cb = 0;
    for (int e = t; e < n; e += SR_THREADS) {
      const unsigned u = it.at(e);
      const float f = __uint_as_float(u);
      atomicAdd(&s_hist[u >> 24], 1u);
      mx = max(mx, u);
      if (e < it.na) { sa += (double)f; ca += f <= tolerance; }
      else { sb += (double)f; cb += f <= tolerance; }
    }
    atomicMax(&s_misc[0], mx);
    if (ca) atomicAdd(&s_misc[1], ca);
    if (cb) atomicAdd(&s_misc[2], cb);
    s_sum[0][t] = sa;
    s_sum[1][t] = sb;
  }
  unsigned prefix = 0, below = 0, bin, excl, copies;
  sr_select_bin(s_hist, s_wave, s_pick, (unsigned)j, bin, excl, copies);          // its first barrier also publishes s_sum and s_misc
  prefix = bin;
  below = excl;
  for (int half = SR_THREADS / 2; half > 0; half >>= 1) {          // the fixed tree: element t += element t + half
    if (t < half) {
      s_sum[0][t] += s_sum[0][t + half];
      s_sum[1][t] += s_sum[1][t + half];
    }
    __syncthreads();
  }

  // ---- passes 1 .. 3: the next byte of the elements under the prefix ----
  for (int shift = 16; shift >= 0; shift -= 8) {
    s_hist[t] = 0;                                                 // every thread has read its bin (the barriers of the select)
    __syncthreads();
    for (int e = t; e < n; e += SR_THREADS) {
      const unsigned u = it.at(e);
      if ((u >> (shift + 8)) == prefix) atomicAdd(&s_hist[(u >> shift) & 255u], 1u);
    }
    sr_select_bin(s_hist, s_wave, s_pick, (unsigned)j - below, bin, excl, copies);
    prefix = (prefix << 8) | bin;
    below += excl;
  }

  // ---- the upper neighbour: S[j] again when the run of equal values reaches rank j + 1 (or j is the last rank) ----
  unsigned upper = prefix;
  if (j + 1 < n && below + copies < (unsigned)j + 2u) {            // uniform over the block
    unsigned mn = 0xFFFFFFFFu;
    for (int e = t; e < n; e += SR_THREADS) {
      const unsigned u = it.at(e);
      if (u > prefix) mn = min(mn, u);
    }
    atomicMin(&s_misc[3], mn);
    __syncthreads();
    upper = s_misc[3];
  }
  if (t == 0) {
    o[0] = (double)__uint_as_float(s_misc[0]);
    o[1] = s_sum[0][0];
    o[2] = s_sum[1][0];
    o[3] = (double)s_misc[1];
    o[4] = (double)s_misc[2];
    o[5] = (double)__uint_as_float(prefix);
    o[6] = (double)__uint_as_float(upper);
    o[7] = (double)n;
  }
}

extern "C" int pp_surface_reduce(const float* dist, const int* counts, int items, int cap, double percentile, float tolerance, double* out,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(dist && counts && out, "surface_reduce: null pointer");
  PP_CHECK_ARG(items >= 1 && cap >= 1, "surface_reduce: bad shape items=%d cap=%d", items, cap);
  PP_CHECK_ARG(percentile > 0.0 && percentile <= 100.0, "surface_reduce: percentile=%g (0 < percentile <= 100)", percentile);
  PP_CHECK_ARG(tolerance >= 0.f && tolerance <= 3.4028234e38f, "surface_reduce: tolerance=%g (finite, >= 0)", (double)tolerance);
  PP_CHECK_ARG((unsigned long long)items * 2ull * (unsigned long long)cap < 0x80000000ull, "surface_reduce: items*2*cap must be below 2^31");
  // traffic: at most six passes over the live prefixes, which the host does not know: the bound for full sets
  pp_prof_begin(PP_K_LOSS, 0.0, 6.0 * 8.0 * (double)items * cap, s);
  hipLaunchKernelGGL(surface_reduce_kernel, dim3(items), dim3(SR_THREADS), 0, s, dist, counts, cap, percentile / 100.0, tolerance, out);
  pp_prof_end(s);
  return pp_launch_status("surface_reduce");
}

// ================================================================================================================================
// Mean-field CRF refinement of a soft-max with an image-dependent pairwise term (include/pacingpseudo_hip.h; DESIGN.md section 7,
// "CRF refinement").  With j = i + (dy, dx) * d, dy, dx in [-r, r] \ (0, 0), j inside the image:
//   kb_ij = exp(-(dy^2 + dx^2) / (2 sxy^2)) * exp(-|x_i - x_j|^2 / (2 srgb^2)),  ks_ij = exp(-(dy^2 + dx^2) / (2 ssm^2))
//   Q^{t+1}_i = softmax_c(u_ic + wb (sum_j kb_ij Q^t_jc) / (sum_j kb_ij + 1e-6) + ws (sum_j ks_ij Q^t_jc) / (sum_j ks_ij + 1e-6))
// with Q^0 = softmax(logits) and u = log_softmax(logits); the soft-max does not see a per-pixel shift, so the kernel adds the
// message to the logits themselves.
//   crf_refine_kernel   one launch per iteration: Q^t (iteration 0: the logits) -> Q^{t+1}; the last launch also writes cls
// The tile, the halo and the LDS layout are crf_fwd_kernel's (pp_loss.hip): a block of four waves owns a 64 x 4 tile, one pixel per
// lane, and stages tile + halo r*d pixel-major with an odd row length: a chunk of KC classes of Q^t (iteration 0: the soft-max of
// the logits with the full-K normaliser, formed while staging, so Q^0 never reaches memory), the image channels and a 1 / 0 plane
// "inside the image" (an outside j adds nothing, also not to the normalisers).  Every lane walks the (2r+1)^2 offsets ONCE for both
// kernels: the intensity factor is one exp2 of the staged channel differences, the two position factors are products of the 1-D
// Gaussians of a table that arrives with the launch arguments (uniform over the wave: scalar loads), and Gb[c], Gs[c], Sb, Ss stay
// in registers.  K <= KC: the lane forms the soft-max of its K values in registers and writes Q^{t+1}.  K > KC runs in class chunks
// (restage, walk again, k recomputed: the same additions in the same order, so Sb and Ss are the same bits in every chunk): the lane
// writes logit + message per chunk to the output and normalises over all K at the end from the addresses it wrote itself.
// Each output element is written by one lane from values of its own slice, added in the order of the walk, and a staged zero leaves
// an accumulator as it is: no atomics, no dependence on the grid -- the same bits in every run and, per slice, in every batch.
// The limits below are pp_crf_loss_fwd's (pp_loss.hip: CRF_*).
#define CRR_TW 64
#define CRR_TH 4
#define CRR_THREADS (CRR_TW * CRR_TH)
#define CRR_MAXR 8
#define CRR_MAXD 4
#define CRR_MAXHALO 16
#define CRR_MAXC 4
#define CRR_KC 8                         // largest class chunk
#define CRR_MAXITER 64
#define CRR_LDS_MAX (160 * 1024 - 256)
#define CRR_EPS 1e-6f

struct CrrTable {                        // 1-D position factors of the offsets -r .. r at index dy + r: bilateral (sigma_xy), smoothness
  float b[2 * CRR_MAXR + 1];
  float s[2 * CRR_MAXR + 1];
};

static inline size_t crr_lds_bytes(int P, int halo) {
  return (size_t)(CRR_TW + 2 * halo) * (CRR_TH + 2 * halo) * P * sizeof(float);
}

__device__ __forceinline__ void crr_softmax_norm(const float* __restrict__ zq, int K, int HW, float& mx, float& inv) {
  mx = -INFINITY;
  for (int k = 0; k < K; ++k) mx = fmaxf(mx, zq[(size_t)k * HW]);
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(zq[(size_t)k * HW] - mx);
  inv = 1.f / s;
}

// z: logits [N][K][H][W]; qin: Q^t, null in iteration 0; qout: Q^{t+1} (never qin or z); cls: null but in the last launch
template <int KC, int CT>                // CT: image channels (1 or 3), 0: any count up to CRR_MAXC at run time
__global__ __launch_bounds__(CRR_THREADS) void crf_refine_kernel(
    const float* __restrict__ z, const float* __restrict__ qin, const float* __restrict__ img, int K, int C, int H, int W, int r, int d,
    float a_rgb, float wb, float ws, int nchunks, CrrTable tab, float* __restrict__ qout, long long* __restrict__ cls) {
  extern __shared__ float crr_lds[];
  constexpr int NC = CT ? CT : CRR_MAXC, P = (KC + NC + 1) | 1;      // floats per staged pixel: [0, KC) q, [KC, KC + NC) x, [KC + NC] inside
  const int R = r * d, LW = CRR_TW + 2 * R, LH = CRR_TH + 2 * R, HW = H * W;
  const int n = blockIdx.z, x0 = blockIdx.x * CRR_TW, y0 = blockIdx.y * CRR_TH;
  const float* zn = z + (size_t)n * K * HW;
  const float* qn = qin ? qin + (size_t)n * K * HW : nullptr;
  const float* xn = img + (size_t)n * C * HW;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int gx = x0 + lx, gy = y0 + ly, q = gy * W + gx;
  const bool inside = gx < W && gy < H;
  float* on = qout + (size_t)n * K * HW + q;                         // dereferenced by inside lanes only
  const float* ci = crr_lds + ((ly + R) * LW + lx + R) * P;          // this lane's own pixel
  for (int ch = 0; ch < nchunks; ++ch) {
    const int c0 = ch * KC;
    if (ch) __syncthreads();                                         // every lane is through with the previous chunk
    for (int s = threadIdx.x; s < LW * LH; s += CRR_THREADS) {
      const int sy = s / LW, sx = s - sy * LW;
      const int py = y0 - R + sy, px = x0 - R + sx;
      float* o = crr_lds + s * P;
      if (px >= 0 && px < W && py >= 0 && py < H) {
        const int sq = py * W + px;
        if (qn) {
#pragma unroll
          for (int c = 0; c < KC; ++c) o[c] = c0 + c < K ? qn[(size_t)(c0 + c) * HW + sq] : 0.f;
        } else if (nchunks == 1) {                                   // K <= KC: one load per logit
          float v[KC];
          float mx = -INFINITY;
#pragma unroll
          for (int c = 0; c < KC; ++c) { v[c] = c < K ? zn[(size_t)c * HW + sq] : -INFINITY; mx = fmaxf(mx, v[c]); }
          float sum = 0.f;
#pragma unroll
          for (int c = 0; c < KC; ++c) { v[c] = c < K ? expf(v[c] - mx) : 0.f; sum += v[c]; }
          const float inv = 1.f / sum;
#pragma unroll
          for (int c = 0; c < KC; ++c) o[c] = v[c] * inv;
        } else {
          float mx, inv;
          crr_softmax_norm(zn + sq, K, HW, mx, inv);
#pragma unroll
          for (int c = 0; c < KC; ++c) o[c] = c0 + c < K ? expf(zn[(size_t)(c0 + c) * HW + sq] - mx) * inv : 0.f;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) o[KC + c] = c < C ? xn[(size_t)c * HW + sq] : 0.f;
        o[KC + NC] = 1.f;
      } else {
#pragma unroll
        for (int c = 0; c < KC + NC + 1; ++c) o[c] = 0.f;
      }
    }
    __syncthreads();
    float xi[NC], Gb[KC], Gs[KC];
#pragma unroll
    for (int c = 0; c < NC; ++c) xi[c] = ci[KC + c];
#pragma unroll
    for (int c = 0; c < KC; ++c) { Gb[c] = 0.f; Gs[c] = 0.f; }
    float Sb = 0.f, Ss = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const float* row = ci + dy * d * LW * P;
      const float tb = tab.b[dy + r], ts = tab.s[dy + r];
#pragma unroll 2
      for (int dx = -r; dx <= r; ++dx) {
        const float* cj = row + dx * d * P;
        float e = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float t = xi[c] - cj[KC + c]; e = __builtin_fmaf(t * t, a_rgb, e); }
        const float mj = cj[KC + NC] * ((dy | dx) ? 1.f : 0.f);      // (0, 0) is no neighbour: its plane value times a uniform 0
        const float kb = __builtin_amdgcn_exp2f(e) * (mj * (tb * tab.b[dx + r]));
        const float ks = mj * (ts * tab.s[dx + r]);
        Sb += kb;
        Ss += ks;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          Gb[c] = __builtin_fmaf(kb, cj[c], Gb[c]);
          Gs[c] = __builtin_fmaf(ks, cj[c], Gs[c]);
        }
      }
    }
    const float fb = wb / (Sb + CRR_EPS), fs = ws / (Ss + CRR_EPS);
    if (inside) {
      if (nchunks == 1) {
        float v[KC];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          v[c] = c < K ? zn[(size_t)c * HW + q] + __builtin_fmaf(Gb[c], fb, Gs[c] * fs) : -INFINITY;
          mx = fmaxf(mx, v[c]);
        }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) { v[c] = c < K ? expf(v[c] - mx) : 0.f; sum += v[c]; }
        const float inv = 1.f / sum;
        float best = -1.f;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (c < K) {
            const float p = v[c] * inv;
            on[(size_t)c * HW] = p;
            if (p > best) { best = p; arg = c; }                     // the first maximum of the values as they are stored
          }
        if (cls) cls[(size_t)n * HW + q] = arg;
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (c0 + c < K) on[(size_t)(c0 + c) * HW] = zn[(size_t)(c0 + c) * HW + q] + __builtin_fmaf(Gb[c], fb, Gs[c] * fs);
      }
    }
  }
  if (inside && nchunks > 1) {
    // same lane, same addresses as the stores above: logit + message of all K classes -> their soft-max
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, on[(size_t)k * HW]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf(on[(size_t)k * HW] - mx);
    const float inv = 1.f / sum;
    float best = -1.f;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      const float p = expf(on[(size_t)k * HW] - mx) * inv;
      on[(size_t)k * HW] = p;
      if (p > best) { best = p; arg = k; }
    }
    if (cls) cls[(size_t)n * HW + q] = arg;
  }
}

struct CrrCall {
  const float* logits; const float* image; int N, K, C, H, W, iterations, radius, dilation;
  float a_rgb, wb, ws; int nchunks; size_t lds; CrrTable tab; float* prob; long long* cls; float* work; hipStream_t s;
};

// Ping-pong between prob and the workspace so that the last launch (t = T - 1) writes prob: launch t writes prob when T - 1 - t is even.
template <int KC, int CT>
static void crr_run(const CrrCall& a) {
  auto kern = crf_refine_kernel<KC, CT>;
  pp_max_lds(reinterpret_cast<const void*>(kern), CRR_LDS_MAX);
  const dim3 grid(pp_cdiv(a.W, CRR_TW), pp_cdiv(a.H, CRR_TH), a.N);
  const float* src = nullptr;
  for (int t = 0; t < a.iterations; ++t) {
    float* dst = ((a.iterations - 1 - t) & 1) ? a.work : a.prob;
    hipLaunchKernelGGL(kern, grid, dim3(CRR_THREADS), a.lds, a.s, a.logits, src, a.image, a.K, a.C, a.H, a.W, a.radius, a.dilation, a.a_rgb,
                       a.wb, a.ws, a.nchunks, a.tab, dst, t == a.iterations - 1 ? a.cls : nullptr);
    src = dst;
  }
}
template <int KC>
static void crr_by_channels(const CrrCall& a) {
  if (a.C == 1) crr_run<KC, 1>(a);
  else if (a.C == 3) crr_run<KC, 3>(a);
  else crr_run<KC, 0>(a);
}

extern "C" size_t pp_crf_refine_workspace(int N, int K, int H, int W) {
  if (N < 1 || K < 1 || H < 1 || W < 1) return 0;
  return (size_t)N * K * H * W * sizeof(float);
}

static inline bool crr_disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p + na <= q || q + nb <= p;
}

extern "C" int pp_crf_refine(const float* logits, const float* image, int N, int K, int C, int H, int W, int iterations, int radius,
                             int dilation, float sigma_xy, float sigma_rgb, float sigma_smooth, float w_bilateral, float w_smooth,
                             float* prob, int64_t* cls, void* workspace, size_t workspace_bytes, void* stream) {
  PP_CHECK_ARG(logits && image && prob && workspace, "crf_refine: null pointer");
  // (N and the rows of tiles are grid.z and grid.y: 65535 each)
  PP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 * CRR_TH && W >= 1, "crf_refine: N=%d (1..65535) H=%d (1..%d) W=%d", N, H,
               65535 * CRR_TH, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && C >= 1 && C <= CRR_MAXC, "crf_refine: K=%d (1..%d) C=%d (1..%d)", K, PP_MAXK, C, CRR_MAXC);
  PP_CHECK_ARG((long long)H * W * K < 0x7fffffffLL, "crf_refine: K*H*W must be below 2^31");
  PP_CHECK_ARG(iterations >= 1 && iterations <= CRR_MAXITER, "crf_refine: iterations=%d (1..%d)", iterations, CRR_MAXITER);
  PP_CHECK_ARG(radius >= 1 && radius <= CRR_MAXR && dilation >= 1 && dilation <= CRR_MAXD && radius * dilation <= CRR_MAXHALO,
               "crf_refine: radius=%d (1..%d) dilation=%d (1..%d), radius * dilation <= %d", radius, CRR_MAXR, dilation, CRR_MAXD, CRR_MAXHALO);
  PP_CHECK_ARG(sigma_xy > 0.f && sigma_rgb > 0.f && sigma_smooth > 0.f && sigma_xy < INFINITY && sigma_rgb < INFINITY && sigma_smooth < INFINITY,
               "crf_refine: sigma_xy=%g sigma_rgb=%g sigma_smooth=%g (> 0, finite)", (double)sigma_xy, (double)sigma_rgb, (double)sigma_smooth);
  PP_CHECK_ARG(w_bilateral >= 0.f && w_smooth >= 0.f && w_bilateral < INFINITY && w_smooth < INFINITY,
               "crf_refine: w_bilateral=%g w_smooth=%g (>= 0, finite)", (double)w_bilateral, (double)w_smooth);
  const size_t need = pp_crf_refine_workspace(N, K, H, W), img_bytes = (size_t)N * C * H * W * sizeof(float);
  if (workspace_bytes < need) {
    pp_set_error("crf_refine: workspace too small (%zu < %zu)", workspace_bytes, need);
    return PP_ERR_WORKSPACE;
  }
  PP_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "crf_refine: workspace must be 4-byte aligned");
  PP_CHECK_ARG(crr_disjoint(prob, need, logits, need) && crr_disjoint(prob, need, image, img_bytes) && crr_disjoint(prob, need, workspace, need) &&
                   crr_disjoint(workspace, need, logits, need) && crr_disjoint(workspace, need, image, img_bytes),
               "crf_refine: prob and workspace must not overlap each other, logits or image");
  PP_CHECK_ARG(!cls || (crr_disjoint(cls, (size_t)N * H * W * sizeof(int64_t), prob, need) &&
                        crr_disjoint(cls, (size_t)N * H * W * sizeof(int64_t), workspace, need)),
               "crf_refine: cls must not overlap prob or workspace");
  CrrCall a;
  a.logits = logits; a.image = image; a.N = N; a.K = K; a.C = C; a.H = H; a.W = W; a.iterations = iterations; a.radius = radius; a.dilation = dilation;
  a.wb = w_bilateral; a.ws = w_smooth; a.prob = prob; a.cls = (long long*)cls; a.work = (float*)workspace; a.s = (hipStream_t)stream;
  const int halo = radius * dilation, NC = (C == 1 || C == 3) ? C : CRR_MAXC;
  // class chunks: as few as the LDS bound allows, of equal width (K = 9 -> 5 + 4, not 8 + 1)
  int nchunks = pp_cdiv(K, CRR_KC), KC = pp_cdiv(K, nchunks);
  while (crr_lds_bytes((KC + NC + 1) | 1, halo) > CRR_LDS_MAX) { ++nchunks; KC = pp_cdiv(K, nchunks); }
  a.nchunks = pp_cdiv(K, KC);
  a.lds = crr_lds_bytes((KC + NC + 1) | 1, halo);
  a.a_rgb = (float)(-1.4426950408889634 / (2.0 * (double)sigma_rgb * sigma_rgb));
  for (int i = 0; i < 2 * CRR_MAXR + 1; ++i) {
    const double o = (double)(i - radius) * (i - radius);
    const bool used = i <= 2 * radius;
    a.tab.b[i] = used ? (float)exp(-o / (2.0 * (double)sigma_xy * sigma_xy)) : 0.f;
    a.tab.s[i] = used ? (float)exp(-o / (2.0 * (double)sigma_smooth * sigma_smooth)) : 0.f;
  }
  const double px = (double)N * H * W, nb = (2.0 * radius + 1.0) * (2.0 * radius + 1.0) - 1.0;
  pp_prof_begin(PP_K_MISC, iterations * px * nb * a.nchunks * (4.0 * KC + 3.0 * C + 8.0), iterations * px * (12.0 * K + 4.0 * C) + 8.0 * px, a.s);
  switch (KC) {
    case 1: crr_by_channels<1>(a); break;
    case 2: crr_by_channels<2>(a); break;
    case 3: crr_by_channels<3>(a); break;
    case 4: crr_by_channels<4>(a); break;
    case 5: crr_by_channels<5>(a); break;
    case 6: crr_by_channels<6>(a); break;
    case 7: crr_by_channels<7>(a); break;
    default: crr_by_channels<8>(a); break;
  }
  pp_prof_end(a.s);
  return pp_launch_status("crf_refine");
}
