// pp_morph.hip -- libpacingpseudo_morph.so (include/pacingpseudo_morph.h): a size threshold per class and hole filling on hard class
// maps whose components are already labelled (pp_label_components in 2-D, pvol_label_components in 3-D: the label of a voxel is the
// smallest linear index of its component, so a component's root is the voxel with labels[i] == i).  No union-find here: one 32-bit
// accumulator per voxel, used at the roots and cleared by hipMemsetAsync, and two launches per call.
//
//   mor_size_kernel          size[root] += 1 per voxel of a thresholded class -- one atomic per run of equal roots inside a wave
//                            (cc_flatten_kernel's trick), so a liver-sized component costs one add per wave, not 64 -- and none once
//                            the size is seen to have reached the threshold
//   mor_small_apply_kernel   out = 0 where size[root] < min_size[class]; per block the removed components (counted at their roots)
//                            and voxels are summed in LDS, then one atomic per non-zero (class, column) into stats
//   mor_contact_kernel       per value-0 voxel a 32-bit mask: bit v = a neighbour of class v in 1 .. K - 1, bit 0 = on the item's
//                            border or a neighbour outside [0, K); OR-ed over each run of equal roots inside a wave by shuffles, then
//                            one atomic OR per run into mask[root] -- none at all for a voxel run without contacts, which is most of
//                            the background, nor for bits the root is seen to hold already
//   mor_fill_apply_kernel    a value-0 voxel becomes k iff mask[root] == 1 << k with k >= 1; masks without bit 0 and with several
//                            bits are the mixed cavities of stats row 0; counted like the removals
// Every block works on chunks of 256 consecutive voxels of ONE item, so runs and LDS sums never span two items.  The accumulators are
// written by relaxed agent-scope integer atomics in one launch and read by plain loads in the next: the kernel boundary orders them
// (the XCDs' L2s are not coherent inside a launch, which nothing here relies on: the two looks at an accumulator inside the launch
// that writes it only ever save an atomic that would change no verdict).  Adds and ORs of integers commute: the same outputs and
// statistics in every run.  A label outside [0, own index] is never an index.
// Self-contained on purpose: it shares no object code with the other libraries.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "pacingpseudo_morph.h"

#define PMOR_VERSION 100
#define PMOR_THREADS 256
#define PMOR_MAX_K 32
#define PMOR_MAX_DEPTH 4096
#define PMOR_MAX_SIDE 2048
#define PMOR_MAX_BLOCKS (1 << 20)        // larger problems walk with a grid stride
#define PMOR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PMOR_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

typedef unsigned long long pmor_u64;

struct pmor_thresholds {
  int v[PMOR_MAX_K];
};

static thread_local char g_mor_err[512] = "";

static void mor_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_mor_err, sizeof(g_mor_err), fmt, ap);
  va_end(ap);
}

#define MOR_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      mor_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int mor_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    mor_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
// The chunk loop: chunk c = (item, block of PMOR_THREADS consecutive voxels of that item); i = the voxel's index within its item,
// g = its index in the whole array, `in` = false on the tail lanes of an item's last chunk.  Every thread of the block runs every pass
// of the loop, so shuffles and barriers inside it are safe.
#define MOR_CHUNK_LOOP for (long long c = blockIdx.x; c < chunks; c += gridDim.x)
#define MOR_CHUNK_VOXEL                                                              \
  const int item = (int)(c / cpi);                                                   \
  const long long il = (c % cpi) * PMOR_THREADS + (long long)threadIdx.x;            \
  const bool in = il < n;                                                            \
  const int i = in ? (int)il : 0;                                                    \
  const long long g = (long long)item * n + i

// a label is used as an index only if it lies in [0, i]: labels point at the smallest index of the component
__device__ __forceinline__ bool mor_label_ok(int l, int i) { return l >= 0 && l <= i; }

// lanes up to the next leader of a run (leaders = ballot of the lanes that start a run)
__device__ __forceinline__ int mor_run_length(pmor_u64 leaders, int lane) {
  const pmor_u64 above = lane == 63 ? 0ull : leaders >> (lane + 1);
  return above ? __ffsll((long long)above) : 64 - lane;
}

// size[item * n + root] += 1 per voxel of a class k in 1 .. K - 1 with thr[k] > 1 (the other classes are never looked up)
__global__ __launch_bounds__(PMOR_THREADS) void mor_size_kernel(const long long* __restrict__ cls, const int* __restrict__ labels, int n,
                                                                int cpi, long long chunks, int K, pmor_thresholds thr,
                                                                int* __restrict__ size) {
  const int lane = threadIdx.x & 63;
  MOR_CHUNK_LOOP {
    MOR_CHUNK_VOXEL;
    int key = -1, limit = 0;
    if (in) {
      const long long v = cls[g];
      if (v >= 1 && v < K && thr.v[(int)v] > 1) {
        const int l = labels[g];
        if (mor_label_ok(l, i)) {
          key = l;
          limit = thr.v[(int)v];
        }
      }
    }
    const int prev = __shfl_up(key, 1, 64);
    const bool lead = lane == 0 || prev != key;
    const pmor_u64 leaders = __ballot(lead);
    if (lead && key >= 0) {
      // a size that has reached the threshold is not counted further: one root of a large organ would otherwise take an add from
      // every wave that crosses the organ.  Sizes only grow, so a final size below the threshold means no add was left out and
      // is the true size, and a true size below the threshold means none ever is: the comparison in the apply pass is exact.
      int* slot = size + ((long long)item * n + key);
      if (__hip_atomic_load(slot, PMOR_RLX_AGENT) < limit) __hip_atomic_fetch_add(slot, mor_run_length(leaders, lane), PMOR_RLX_AGENT);
    }
  }
}

// cls and out may be the same array: every voxel is read and written by one thread
__global__ __launch_bounds__(PMOR_THREADS) void mor_small_apply_kernel(const long long* cls, const int* __restrict__ labels,
                                                                       const int* __restrict__ size, int n, int cpi, long long chunks,
                                                                       int K, pmor_thresholds thr, long long* out,
                                                                       int* __restrict__ stats) {
  __shared__ int sh[2 * PMOR_MAX_K];
  const int tid = threadIdx.x;
  MOR_CHUNK_LOOP {
    MOR_CHUNK_VOXEL;
    if (tid < 2 * PMOR_MAX_K) sh[tid] = 0;
    __syncthreads();
    if (in) {
      const long long v = cls[g];
      long long o = v;
      if (v >= 1 && v < K && thr.v[(int)v] > 1) {
        const int l = labels[g];
        if (mor_label_ok(l, i) && size[(long long)item * n + l] < thr.v[(int)v]) {
          o = 0;
          __hip_atomic_fetch_add(sh + 2 * (int)v + 1, 1, PMOR_RLX_WG);
          if (l == i) __hip_atomic_fetch_add(sh + 2 * (int)v, 1, PMOR_RLX_WG);
        }
      }
      out[g] = o;
    }
    __syncthreads();
    if (tid < 2 * K && sh[tid] != 0) __hip_atomic_fetch_add(stats + ((long long)item * 2 * K + tid), sh[tid], PMOR_RLX_AGENT);
    __syncthreads();
  }
}

// mask[item * n + root] |= the contacts of every value-0 voxel.  DIMS = 2: D == 1 and only (dy, dx) offsets.
template <int DIMS>
__global__ __launch_bounds__(PMOR_THREADS) void mor_contact_kernel(const long long* __restrict__ cls, const int* __restrict__ labels, int D,
                                                                   int H, int W, int n, int cpi, long long chunks, int K, int conn,
                                                                   unsigned* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  MOR_CHUNK_LOOP {
    MOR_CHUNK_VOXEL;
    int key = -1;
    unsigned m = 0;
    if (in && cls[g] == 0) {
      const int l = labels[g];
      if (mor_label_ok(l, i)) {
        key = l;
        const int x = i % W, y = (i / W) % H, z = i / (W * H);
        const bool border = x == 0 || x == W - 1 || y == 0 || y == H - 1 || (DIMS == 3 && (z == 0 || z == D - 1));
        if (border) {
          m = 1u;                                            // bit 0 vetoes whatever else the component touches
        } else {                                             // an interior voxel: every neighbour lies inside the item
          const long long* base = cls + g;
#pragma unroll
          for (int dz = (DIMS == 3 ? -1 : 0); dz <= (DIMS == 3 ? 1 : 0); ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
              for (int dx = -1; dx <= 1; ++dx) {
                const int nz = (dz != 0) + (dy != 0) + (dx != 0);
                if (nz == 0 || nz > conn) continue;
                const long long u = base[((long long)dz * H + dy) * W + dx];
                if (u != 0) m |= (u >= 1 && u < K) ? 1u << (int)u : 1u;
              }
        }
      }
    }
    // OR over the lanes that follow with the same root: after the step of width d a lane holds its run's next 2 d lanes (a lane
    // further on with the same root but in another run belongs to the same component: taking it in changes nothing)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_down(m, d, 64);
      const int k2 = __shfl_down(key, d, 64);
      if (lane + d < 64 && k2 == key) m |= t;
    }
    const int prev = __shfl_up(key, 1, 64);
    const bool lead = lane == 0 || prev != key;
    if (lead && key >= 0 && m != 0) {
      // bits that are already there are not sent again, and nothing is once bit 0 is set (the verdict is final): the background of
      // a volume is ONE component whose root would otherwise take an OR from every wave on a face or along an organ.  A stale
      // look only costs an OR that changes nothing.
      unsigned* slot = mask + ((long long)item * n + key);
      const unsigned cur = __hip_atomic_load(slot, PMOR_RLX_AGENT);
      if (!(cur & 1u) && (cur & m) != m) __hip_atomic_fetch_or(slot, m, PMOR_RLX_AGENT);
    }
  }
}

// cls and out may be the same array: every voxel is read and written by one thread (the neighbours were read in the launch before)
__global__ __launch_bounds__(PMOR_THREADS) void mor_fill_apply_kernel(const long long* cls, const int* __restrict__ labels,
                                                                      const unsigned* __restrict__ mask, int n, int cpi, long long chunks,
                                                                      int K, long long* out, int* __restrict__ stats) {
  __shared__ int sh[2 * PMOR_MAX_K];
  const int tid = threadIdx.x;
  MOR_CHUNK_LOOP {
    MOR_CHUNK_VOXEL;
    if (tid < 2 * PMOR_MAX_K) sh[tid] = 0;
    __syncthreads();
    if (in) {
      const long long v = cls[g];
      long long o = v;
      if (v == 0) {
        const int l = labels[g];
        if (mor_label_ok(l, i)) {
          const unsigned m = mask[(long long)item * n + l];
          if (m > 1u && !(m & 1u)) {                         // a cavity: not on the border, no contact outside [0, K)
            const int k = (m & (m - 1u)) == 0u ? __ffs((int)m) - 1 : 0;       // one contact class, or row 0: mixed
            if (k != 0) o = k;
            __hip_atomic_fetch_add(sh + 2 * k + 1, 1, PMOR_RLX_WG);
            if (l == i) __hip_atomic_fetch_add(sh + 2 * k, 1, PMOR_RLX_WG);
          }
        }
      }
      out[g] = o;
    }
    __syncthreads();
    if (tid < 2 * K && sh[tid] != 0) __hip_atomic_fetch_add(stats + ((long long)item * 2 * K + tid), sh[tid], PMOR_RLX_AGENT);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static inline size_t mor_pad8(size_t b) { return (b + 7) / 8 * 8; }
static inline bool mor_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int mor_check_shape(const char* who, int N, int K, int D, int H, int W, int dims) {
  MOR_CHECK_ARG(dims == 2 || dims == 3, "%s: dims = %d, need 2 (slices) or 3 (volumes)", who, dims);
  MOR_CHECK_ARG(N >= 1, "%s: N = %d, need at least one item", who, N);
  MOR_CHECK_ARG(K >= 1 && K <= PMOR_MAX_K, "%s: K = %d, need 1 <= K <= %d", who, K, PMOR_MAX_K);
  MOR_CHECK_ARG(D >= 1 && D <= PMOR_MAX_DEPTH, "%s: D = %d, need 1 <= D <= %d", who, D, PMOR_MAX_DEPTH);
  MOR_CHECK_ARG(dims == 3 || D == 1, "%s: D = %d with dims = 2, a slice has D = 1", who, D);
  MOR_CHECK_ARG(H >= 1 && H <= PMOR_MAX_SIDE && W >= 1 && W <= PMOR_MAX_SIDE, "%s: H = %d, W = %d, need 1 <= H, W <= %d", who, H, W,
                PMOR_MAX_SIDE);
  MOR_CHECK_ARG((long long)D * H * W < (1ll << 31), "%s: D * H * W = %lld, need fewer than 2^31 voxels per item", who, (long long)D * H * W);
  MOR_CHECK_ARG((long long)N * ((long long)D * H * W) < (1ll << 31), "%s: N * D * H * W = %lld, need fewer than 2^31 voxels", who,
                (long long)N * ((long long)D * H * W));
  return 0;
}

static int mor_check_pointers(const char* who, const void* cls, const void* labels, const void* out, const void* stats, const void* ws) {
  MOR_CHECK_ARG(cls && labels && out && stats && ws, "%s: null pointer (cls %p, labels %p, out %p, stats %p, workspace %p)", who, cls, labels,
                out, stats, ws);
  MOR_CHECK_ARG(mor_al(cls, 8) && mor_al(out, 8) && mor_al(ws, 8), "%s: cls, out and the workspace must be 8-byte aligned", who);
  MOR_CHECK_ARG(mor_al(labels, 4) && mor_al(stats, 4), "%s: labels and stats must be 4-byte aligned", who);
  return 0;
}

static int mor_clear(const char* who, void* p, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  if (e != hipSuccess) {
    mor_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

extern "C" int pmor_version(void) { return PMOR_VERSION; }
extern "C" const char* pmor_last_error(void) { return g_mor_err; }

extern "C" size_t pmor_workspace(int N, int K, int D, int H, int W, int dims) {
  if (mor_check_shape("pmor_workspace", N, K, D, H, W, dims) != 0) return 0;
  return mor_pad8(4 * (size_t)N * D * H * W);
}

struct mor_grid {
  int n, cpi;
  long long chunks;
  unsigned blocks;
};
static mor_grid mor_make_grid(int N, int D, int H, int W) {
  mor_grid q;
  q.n = D * H * W;
  q.cpi = (q.n + PMOR_THREADS - 1) / PMOR_THREADS;
  q.chunks = (long long)N * q.cpi;
  q.blocks = (unsigned)(q.chunks < PMOR_MAX_BLOCKS ? q.chunks : PMOR_MAX_BLOCKS);
  return q;
}

extern "C" int pmor_remove_small(const int64_t* cls, const int32_t* labels, int N, int K, int D, int H, int W, int dims,
                                 const int32_t* min_size, int64_t* out, int32_t* stats, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "pmor_remove_small";
  int rc = mor_check_pointers(who, cls, labels, out, stats, workspace);
  if (rc != 0) return rc;
  MOR_CHECK_ARG(min_size, "%s: null pointer (min_size: K thresholds in host memory)", who);
  rc = mor_check_shape(who, N, K, D, H, W, dims);
  if (rc != 0) return rc;
  const size_t need = mor_pad8(4 * (size_t)N * D * H * W);
  MOR_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pmor_workspace)", who, workspace_bytes, need);
  pmor_thresholds thr;
  for (int k = 0; k < PMOR_MAX_K; ++k) thr.v[k] = k >= 1 && k < K ? min_size[k] : 0;
  hipStream_t st = (hipStream_t)stream;
  const mor_grid q = mor_make_grid(N, D, H, W);
  rc = mor_clear(who, workspace, need, st);
  if (rc != 0) return rc;
  rc = mor_clear(who, stats, (size_t)N * K * 2 * sizeof(int32_t), st);
  if (rc != 0) return rc;
  mor_size_kernel<<<dim3(q.blocks), dim3(PMOR_THREADS), 0, st>>>((const long long*)cls, labels, q.n, q.cpi, q.chunks, K, thr,
                                                                  (int*)workspace);
  mor_small_apply_kernel<<<dim3(q.blocks), dim3(PMOR_THREADS), 0, st>>>((const long long*)cls, labels, (const int*)workspace, q.n, q.cpi,
                                                                         q.chunks, K, thr, (long long*)out, stats);
  return mor_launched("pmor_remove_small (size / apply)");
}

extern "C" int pmor_fill_holes(const int64_t* cls, const int32_t* labels, int N, int K, int D, int H, int W, int dims, int connectivity,
                               int64_t* out, int32_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pmor_fill_holes";
  int rc = mor_check_pointers(who, cls, labels, out, stats, workspace);
  if (rc != 0) return rc;
  rc = mor_check_shape(who, N, K, D, H, W, dims);
  if (rc != 0) return rc;
  MOR_CHECK_ARG(connectivity >= 1 && connectivity <= dims, "%s: connectivity = %d, need 1 .. %d with dims = %d", who, connectivity, dims,
                dims);
  const size_t need = mor_pad8(4 * (size_t)N * D * H * W);
  MOR_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pmor_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const mor_grid q = mor_make_grid(N, D, H, W);
  rc = mor_clear(who, workspace, need, st);
  if (rc != 0) return rc;
  rc = mor_clear(who, stats, (size_t)N * K * 2 * sizeof(int32_t), st);
  if (rc != 0) return rc;
  if (dims == 2)
    mor_contact_kernel<2><<<dim3(q.blocks), dim3(PMOR_THREADS), 0, st>>>((const long long*)cls, labels, D, H, W, q.n, q.cpi, q.chunks, K,
                                                                          connectivity, (unsigned*)workspace);
  else
    mor_contact_kernel<3><<<dim3(q.blocks), dim3(PMOR_THREADS), 0, st>>>((const long long*)cls, labels, D, H, W, q.n, q.cpi, q.chunks, K,
                                                                          connectivity, (unsigned*)workspace);
  mor_fill_apply_kernel<<<dim3(q.blocks), dim3(PMOR_THREADS), 0, st>>>((const long long*)cls, labels, (const unsigned*)workspace, q.n, q.cpi,
                                                                        q.chunks, K, (long long*)out, stats);
  return mor_launched("pmor_fill_holes (contacts / apply)");
}
