// pp_volume.hip -- libpacingpseudo_vol.so (include/pacingpseudo_vol.h): volume-wise evaluation of hard class maps.  Three kernel
// families and a counting kernel, each family the 3-D re-thinking of a 2-D one of this project (pp_post.hip: components;
// distance/pp_distance.hip: the exact EDT; pp_loss.hip: the surface-distance sets of HD95):
//
// Components.  A union-find forest over linear voxel indices in which a parent is never larger than its child (roots are the minima,
// every walk towards a root descends and ends).
//   vol_brick_kernel    one brick of 4 x 16 x 32 voxels per block: values (16 KiB) and parents (8 KiB) in LDS -- 24 KiB, six blocks
//                       per CU -- every voxel joins its "backward" neighbours (the 3 / 9 / 13 of the 6- / 18- / 26-neighbourhood that
//                       precede it in linear order) inside the brick, then parent[p] = the brick-local root as a volume index
//   vol_merge_kernel    one thread per voxel; a voxel on a face of its brick joins those backward neighbours that lie in ANOTHER brick
//                       (faces, and for 18 / 26 edges and corners) on the global parent array; interior voxels leave at once
//   vol_flatten_kernel  labels[p] = root of p; component sizes and per-class component counts with integer atomics
//   vol_select_kernel   per root of a foreground class: 64-bit atomicMax of size << 32 | ~label, and the class's voxel total
//   vol_apply_kernel    out = cls where the voxel's component was selected (or the value is no foreground class), else 0
// No block ever waits for another: a union is find both roots, atomicMin the larger root's parent to the smaller, go on from the
// returned value if another thread had moved that root meanwhile -- every retry strictly descends.  The one launch whose blocks race
// on global memory (vol_merge_kernel) touches the parent array through relaxed agent-scope atomics only (the XCDs' L2s are not
// coherent for plain loads); phases are ordered by kernel boundaries.
//
// EDT.  vol_edt_z_kernel: one thread per (y, x) column, threads along x (every load and store of a wave is to consecutive elements),
// two sweeps along z, the distance in voxels to the column's nearest zero voxel as 16 bits (0xFFFF: none).  vol_edt_y_kernel: one
// thread per voxel, threads along x again, an outward scan over y' of (g sz)^2 + ((y - y') sy)^2 read straight from the 16-bit field
// (a wave's loads are 128 consecutive bytes, served by L1 / L2) that stops once ((y - y') sy)^2 alone reaches the best candidate.
// vol_edt_x_kernel: one block per row, the row of the fp32 squared field staged in LDS, the same scan along x, in place.
//
// Surfaces.  Per class, one after another in one workspace (no one-hot volumes): vol_surface_kernel marks both surfaces as byte masks
// (0 = surface voxel, so that a mask is the input of the EDT as it stands) and counts per block of 4096 consecutive voxels;
// vol_scan_kernel (one block) turns the block counts into offsets and the four totals; then per direction the EDT of the other
// surface's complement, the x pass only at this surface's voxels, and vol_gather_kernel compacts those distances in linear-index
// order (ballot + population count inside a wave, the waves' totals through LDS, the blocks' offsets from the scan).  No atomics.
// vol_dice_kernel counts |P and T|, |P|, |T| per class for the volume Dice.
// Self-contained on purpose: it shares no object code with the other libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "pacingpseudo_vol.h"

#define PVOL_VERSION 100
#define PVOL_THREADS 256
#define PVOL_MAX_K 32
#define PVOL_MAX_DEPTH 4096
#define PVOL_MAX_SIDE 2048
#define PVOL_NONE 0xFFFF
#define PVOL_BD 4
#define PVOL_BH 16
#define PVOL_BW 32
#define PVOL_BRICK (PVOL_BD * PVOL_BH * PVOL_BW)
#define PVOL_MAX_BLOCKS (1 << 20)        // larger problems walk with a grid stride
#define PVOL_CHUNK 4096                  // voxels per block of the surface, scan and gather kernels
#define PVOL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PVOL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

typedef unsigned long long pvol_u64;

static thread_local char g_vol_err[512] = "";

static void vol_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_vol_err, sizeof(g_vol_err), fmt, ap);
  va_end(ap);
}

#define VOL_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      vol_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int vol_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    vol_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- union-find
__device__ __forceinline__ int vol_find_lds(int* par, int i) {
  for (;;) {
    const int p = __hip_atomic_load(par + i, PVOL_RLX_WG);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void vol_union_lds(int* par, int a, int b) {
  for (;;) {
    a = vol_find_lds(par, a);
    b = vol_find_lds(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, PVOL_RLX_WG);
    if (old == a) return;                 // a was a root and now hangs below b
    a = old;                              // a had been moved below `old` meanwhile: join old and b instead (old < a)
  }
}
__device__ __forceinline__ int vol_find_agent(int* par, int i) {
  for (;;) {
    const int p = __hip_atomic_load(par + i, PVOL_RLX_AGENT);
    if (p == i) return i;
    i = p;
  }
}
__device__ __forceinline__ void vol_union_agent(int* par, int a, int b) {
  for (;;) {
    a = vol_find_agent(par, a);
    b = vol_find_agent(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, PVOL_RLX_AGENT);
    if (old == a) return;
    a = old;
  }
}

// The backward neighbours: offsets (dz, dy, dx) in {-1, 0, 1}^3 that precede (0, 0, 0) in linear order, of which `conn` admits those
// with at most `conn` non-zero components.  The loops below are unrolled over the 13 of them.
#define VOL_FOR_BACKWARD(dz, dy, dx)     \
  _Pragma("unroll") for (int dz = -1; dz <= 0; ++dz) \
  _Pragma("unroll") for (int dy = -1; dy <= 1; ++dy) \
  _Pragma("unroll") for (int dx = -1; dx <= 1; ++dx) \
    if (!(dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))))

// parent: [D*H*W] linear indices.  size (COUNT): zeroed here for vol_flatten_kernel.
template <bool COUNT>
__global__ __launch_bounds__(PVOL_THREADS) void vol_brick_kernel(const long long* __restrict__ cls, int D, int H, int W, int bx, int by,
                                                                 long long nbricks, int conn, int* __restrict__ parent,
                                                                 int* __restrict__ size) {
  __shared__ long long s_val[PVOL_BRICK];
  __shared__ int s_par[PVOL_BRICK];
  const size_t HW = (size_t)H * W;
  for (long long t = blockIdx.x; t < nbricks; t += gridDim.x) {
    const int r = (int)(t % ((long long)bx * by));
    const int z0 = (int)(t / ((long long)bx * by)) * PVOL_BD, y0 = (r / bx) * PVOL_BH, x0 = (r % bx) * PVOL_BW;
    __syncthreads();                                            // the previous brick of this block has been written out
    for (int i = threadIdx.x; i < PVOL_BRICK; i += PVOL_THREADS) {
      const int z = z0 + i / (PVOL_BH * PVOL_BW), y = y0 + (i / PVOL_BW) % PVOL_BH, x = x0 + i % PVOL_BW;
      s_val[i] = (z < D && y < H && x < W) ? cls[(size_t)z * HW + (size_t)y * W + x] : 0;
      s_par[i] = i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PVOL_BRICK; i += PVOL_THREADS) {
      const int lz = i / (PVOL_BH * PVOL_BW), ly = (i / PVOL_BW) % PVOL_BH, lx = i % PVOL_BW;
      if (z0 + lz >= D || y0 + ly >= H || x0 + lx >= W) continue;
      const long long v = s_val[i];
      VOL_FOR_BACKWARD(dz, dy, dx) {
        if ((dz != 0) + (dy != 0) + (dx != 0) <= conn) {
          // inside the brick, and (for the offsets that go up in y or x) inside the volume
          const bool in = lz + dz >= 0 && ly + dy >= 0 && ly + dy < PVOL_BH && lx + dx >= 0 && lx + dx < PVOL_BW &&
                          y0 + ly + dy < H && x0 + lx + dx < W;
          if (in) {
            const int j = i + dz * (PVOL_BH * PVOL_BW) + dy * PVOL_BW + dx;
            if (s_val[j] == v) vol_union_lds(s_par, i, j);
          }
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PVOL_BRICK; i += PVOL_THREADS) {
      const int z = z0 + i / (PVOL_BH * PVOL_BW), y = y0 + (i / PVOL_BW) % PVOL_BH, x = x0 + i % PVOL_BW;
      if (z >= D || y >= H || x >= W) continue;
      const int root = vol_find_lds(s_par, i);                  // brick order and volume order agree: the minimum stays the minimum
      const size_t g = (size_t)z * HW + (size_t)y * W + x;
      parent[g] = (int)((size_t)(z0 + root / (PVOL_BH * PVOL_BW)) * HW + (size_t)(y0 + (root / PVOL_BW) % PVOL_BH) * W +
                        (size_t)(x0 + root % PVOL_BW));
      if (COUNT) size[g] = 0;
    }
  }
}

__global__ __launch_bounds__(PVOL_THREADS) void vol_merge_kernel(const long long* __restrict__ cls, int D, int H, int W, long long total,
                                                                 int conn, int* parent) {
  const int HW = H * W;
  for (long long g = (long long)blockIdx.x * PVOL_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * PVOL_THREADS) {
    const int z = (int)(g / HW), rem = (int)(g % HW), y = rem / W, x = rem % W;
    const int lz = z % PVOL_BD, ly = y % PVOL_BH, lx = x % PVOL_BW;
    if (lz != 0 && ly != 0 && ly != PVOL_BH - 1 && lx != 0 && lx != PVOL_BW - 1) continue;      // every backward neighbour is in the brick
    const long long v = cls[g];
    VOL_FOR_BACKWARD(dz, dy, dx) {
      if ((dz != 0) + (dy != 0) + (dx != 0) <= conn) {
        const bool in_volume = z + dz >= 0 && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W;
        const bool other_brick = lz + dz < 0 || ly + dy < 0 || ly + dy >= PVOL_BH || lx + dx < 0 || lx + dx >= PVOL_BW;
        if (in_volume && other_brick) {
          const long long q = g + (long long)dz * HW + dy * W + dx;
          if (cls[q] == v) vol_union_agent(parent, (int)g, (int)q);
        }
      }
    }
  }
}

// labels[g] = root of voxel g (the parent array is final: plain loads behind the kernel boundary).  COUNT: size[root] += 1 per voxel
// -- one atomic per run of equal roots inside a wave -- and ncomp[k] += 1 per root of a foreground class.
template <bool COUNT>
__global__ __launch_bounds__(PVOL_THREADS) void vol_flatten_kernel(const long long* __restrict__ cls, const int* __restrict__ parent,
                                                                   long long total, int K, int* __restrict__ labels,
                                                                   int* __restrict__ size, int* __restrict__ ncomp) {
  for (long long b0 = (long long)blockIdx.x * PVOL_THREADS; b0 < total; b0 += (long long)gridDim.x * PVOL_THREADS) {
    const long long g = b0 + threadIdx.x;
    const bool active = g < total;
    int root = -1;
    if (active) {
      root = (int)g;
      for (;;) {
        const int q = parent[root];
        if (q == root) break;
        root = q;
      }
      labels[g] = root;
    }
    if (COUNT) {
      const int lane = threadIdx.x & 63;
      const int prev = __shfl_up(root, 1, 64);
      const bool lead = lane == 0 || prev != root;
      const pvol_u64 leaders = __ballot(lead);
      if (lead && active) {
        const pvol_u64 above = lane == 63 ? 0ull : leaders >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : 64 - lane;      // lanes up to the next leader
        atomicAdd(&size[root], run);
      }
      if (active && root == (int)g) {
        const long long v = cls[g];
        if (v >= 1 && v < K) atomicAdd(&ncomp[(int)v], 1);
      }
    }
  }
}

// best[k] = max over the components of class k of (size << 32 | ~label): the largest, and of equals the smallest label; nvox[k] = the
// class's voxels
__global__ __launch_bounds__(PVOL_THREADS) void vol_select_kernel(const long long* __restrict__ cls, const int* __restrict__ labels,
                                                                  const int* __restrict__ size, long long total, int K,
                                                                  pvol_u64* __restrict__ best, int* __restrict__ nvox) {
  for (long long g = (long long)blockIdx.x * PVOL_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * PVOL_THREADS) {
    if (labels[g] != (int)g) continue;
    const long long v = cls[g];
    if (v >= 1 && v < K) {
      atomicMax(&best[(int)v], ((pvol_u64)(unsigned)size[g] << 32) | (pvol_u64)(~(unsigned)g));
      atomicAdd(&nvox[(int)v], size[g]);
    }
  }
}

// cls and out may be the same array: every voxel is read and written by one thread
__global__ __launch_bounds__(PVOL_THREADS) void vol_apply_kernel(const long long* cls, const int* __restrict__ labels,
                                                                 const pvol_u64* __restrict__ best, const int* __restrict__ ncomp,
                                                                 const int* __restrict__ nvox, long long total, int K, long long* out,
                                                                 int* __restrict__ stats) {
  const long long span = total > K ? total : K;
  for (long long g = (long long)blockIdx.x * PVOL_THREADS + threadIdx.x; g < span; g += (long long)gridDim.x * PVOL_THREADS) {
    if (g < total) {
      const long long v = cls[g];
      long long o = v;
      if (v >= 1 && v < K) {
        const pvol_u64 b = best[(int)v];
        if (~(unsigned)b != (unsigned)labels[g]) o = 0;
      }
      out[g] = o;
    }
    if (g < K) {                                                  // class 0 was never counted: {0, 0}
      stats[2 * g] = ncomp[g];
      stats[2 * g + 1] = nvox[g] - (int)(best[g] >> 32);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- EDT
// g[z][y][x] = |z - z'| to the nearest zero voxel (z', y, x) of the column, PVOL_NONE if the column has none
__global__ __launch_bounds__(PVOL_THREADS) void vol_edt_z_kernel(const unsigned char* __restrict__ mask, int D, int HW,
                                                                 unsigned short* __restrict__ g) {
  const int c = blockIdx.x * PVOL_THREADS + threadIdx.x;
  if (c >= HW) return;
  int last = -1;
  for (int z = 0; z < D; ++z) {
    const size_t i = (size_t)z * HW + c;
    if (mask[i] == 0) last = z;
    g[i] = (unsigned short)(last >= 0 ? z - last : PVOL_NONE);
  }
  last = -1;
  for (int z = D - 1; z >= 0; --z) {
    const size_t i = (size_t)z * HW + c;
    if (mask[i] == 0) last = z;
    const int d = last >= 0 ? last - z : PVOL_NONE;
    if (d < (int)g[i]) g[i] = (unsigned short)d;
  }
}

__device__ __forceinline__ float vol_z_cost(int gv, float sz) {
#pragma clang fp contract(off)
  if (gv == PVOL_NONE) return INFINITY;
  const float gz = (float)gv * sz;
  return gz * gz;
}

// f[z][y][x] = min over y' of (g[z][y'][x] sz)^2 + ((y - y') sy)^2.  fl(a + b) >= b for a >= 0, so once (dy sy)^2 >= best no
// candidate further out can be smaller: the scan is exact.  An index past an end of the column is clamped to it: that voxel was met
// before at a smaller offset, so its candidate cannot win.
__global__ __launch_bounds__(PVOL_THREADS) void vol_edt_y_kernel(const unsigned short* __restrict__ g, int H, int W, long long total,
                                                                 float sz, float sy, float* __restrict__ f) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * PVOL_THREADS + threadIdx.x;
  if (i >= total) return;
  const int HW = H * W;
  const int rem = (int)(i % HW), y = rem / W;
  const unsigned short* __restrict__ col = g + (i - (long long)y * W);          // (z, 0, x)
  float best = vol_z_cost(g[i], sz);
  float df = 0.f;
  for (int d = 1; d < H; ++d) {
    df += 1.f;
    const float dy = df * sy;
    const float dy2 = dy * dy;
    if (dy2 >= best) break;
    const int yl = y - d > 0 ? y - d : 0, yr = y + d < H - 1 ? y + d : H - 1;
    best = fminf(best, fminf(vol_z_cost(col[(size_t)yl * W], sz), vol_z_cost(col[(size_t)yr * W], sz)) + dy2);
  }
  f[i] = best;
}

// One block per row (z, y): the row of f staged in LDS, the same scan along x, the result written over f.  want != NULL: only
// voxels with want[i] == 0 are computed and written (the surface voxels whose distances are gathered), the rest of f is left as it is.
__global__ __launch_bounds__(PVOL_THREADS) void vol_edt_x_kernel(float* __restrict__ f, int W, float sx, int squared,
                                                                 const unsigned char* __restrict__ want) {
#pragma clang fp contract(off)
  __shared__ float cost[PVOL_MAX_SIDE];
  const size_t base = (size_t)blockIdx.x * W;
  for (int x = threadIdx.x; x < W; x += PVOL_THREADS) cost[x] = f[base + x];
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += PVOL_THREADS) {
    if (want && want[base + x] != 0) continue;
    float best = cost[x];
    float df = 0.f;
    for (int d = 1; d < W; ++d) {
      df += 1.f;
      const float dx = df * sx;
      const float dx2 = dx * dx;
      if (dx2 >= best) break;
      const int xl = x - d > 0 ? x - d : 0, xr = x + d < W - 1 ? x + d : W - 1;
      best = fminf(best, fminf(cost[xl], cost[xr]) + dx2);
    }
    f[base + x] = squared ? best : sqrtf(best);
  }
}

// ---------------------------------------------------------------------------------------------------------------- surfaces
__device__ __forceinline__ int vol_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// na / nb: 0 at a surface voxel of pred == k / label == k, 1 elsewhere.  cnt[j][block], j = {surface a, surface b, |a|, |b|}: the
// counts of this block's PVOL_CHUNK consecutive voxels.
__global__ __launch_bounds__(PVOL_THREADS) void vol_surface_kernel(const long long* __restrict__ A, const long long* __restrict__ B,
                                                                   int k, int D, int H, int W, long long total, int nblocks,
                                                                   unsigned char* __restrict__ na, unsigned char* __restrict__ nb,
                                                                   int* __restrict__ cnt) {
  __shared__ int s_cnt[4][PVOL_THREADS / 64];
  const int HW = H * W;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  const long long p0 = (long long)blockIdx.x * PVOL_CHUNK;
  for (int t = threadIdx.x; t < PVOL_CHUNK; t += PVOL_THREADS) {
    const long long p = p0 + t;
    if (p >= total) break;
    const int z = (int)(p / HW), rem = (int)(p % HW), y = rem / W, x = rem % W;
    const bool a = A[p] == k, b = B[p] == k;
    const bool border = z == 0 || z == D - 1 || y == 0 || y == H - 1 || x == 0 || x == W - 1;
    const bool sa = a && (border || !(A[p - HW] == k && A[p + HW] == k && A[p - W] == k && A[p + W] == k && A[p - 1] == k && A[p + 1] == k));
    const bool sb = b && (border || !(B[p - HW] == k && B[p + HW] == k && B[p - W] == k && B[p + W] == k && B[p - 1] == k && B[p + 1] == k));
    na[p] = sa ? 0 : 1;
    nb[p] = sb ? 0 : 1;
    c0 += sa; c1 += sb; c2 += a; c3 += b;
  }
  c0 = vol_wave_sum(c0); c1 = vol_wave_sum(c1); c2 = vol_wave_sum(c2); c3 = vol_wave_sum(c3);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    s_cnt[0][w] = c0; s_cnt[1][w] = c1; s_cnt[2][w] = c2; s_cnt[3][w] = c3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < PVOL_THREADS / 64; ++w) s += s_cnt[threadIdx.x][w];
    cnt[(size_t)threadIdx.x * nblocks + blockIdx.x] = s;
  }
}

// One block: offs[j][b] = sum of cnt[j][< b] for the two surface counts, counts4[j] = the four totals.  Thread t owns the blocks
// [t per, (t + 1) per): its sums go through LDS, thread 0 scans the 256 partial sums, every thread then walks its range again.
__global__ __launch_bounds__(PVOL_THREADS) void vol_scan_kernel(const int* __restrict__ cnt, int nblocks, int* __restrict__ offs,
                                                                int* __restrict__ counts4) {
  __shared__ int s_part[4][PVOL_THREADS];
  const int t = threadIdx.x;
  const int per = (nblocks + PVOL_THREADS - 1) / PVOL_THREADS;
  const int lo = min(t * per, nblocks), hi = min(lo + per, nblocks);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int s = 0;
    for (int b = lo; b < hi; ++b) s += cnt[(size_t)j * nblocks + b];
    s_part[j][t] = s;
  }
  __syncthreads();
  if (t < 4) {
    int run = 0;
    for (int u = 0; u < PVOL_THREADS; ++u) {
      const int s = s_part[t][u];
      s_part[t][u] = run;
      run += s;
    }
    counts4[t] = run;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int run = s_part[j][t];
    for (int b = lo; b < hi; ++b) {
      offs[(size_t)j * nblocks + b] = run;
      run += cnt[(size_t)j * nblocks + b];
    }
  }
}

// out[offs[block] + rank of p among the block's surface voxels] = field[p] for every p with surf[p] == 0: linear-index order
__global__ __launch_bounds__(PVOL_THREADS) void vol_gather_kernel(const unsigned char* __restrict__ surf, const float* __restrict__ field,
                                                                  const int* __restrict__ offs, long long total,
                                                                  float* __restrict__ out) {
  __shared__ int s_w[PVOL_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const pvol_u64 lt_mask = (1ull << lane) - 1ull;
  const long long p0 = (long long)blockIdx.x * PVOL_CHUNK;
  int n = offs[blockIdx.x];                                     // entries written so far: the same in every thread
  for (int t0 = 0; t0 < PVOL_CHUNK; t0 += PVOL_THREADS) {       // uniform trip count: the barriers below are reached by all
    const long long p = p0 + t0 + threadIdx.x;
    const bool s = p < total && surf[p] == 0;
    const pvol_u64 m = __ballot(s);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int o = n;
#pragma unroll
    for (int q = 0; q < PVOL_THREADS / 64; ++q) {
      if (q < wave) o += s_w[q];
      n += s_w[q];
    }
    if (s) out[(size_t)o + __popcll(m & lt_mask)] = field[p];
    __syncthreads();                                            // s_w is rewritten by the next trip
  }
}

// ---------------------------------------------------------------------------------------------------------------- Dice counts
// counts[k] = {|pred == k and label == k|, |pred == k|, |label == k|}: a block counts in LDS, then adds its non-zero entries to the
// zeroed output.  Integer atomics: the order of the additions does not show.
__global__ __launch_bounds__(PVOL_THREADS) void vol_dice_kernel(const long long* __restrict__ A, const long long* __restrict__ B,
                                                                long long total, int K, int* __restrict__ counts) {
  __shared__ int s_c[3 * PVOL_MAX_K];
  if (threadIdx.x < 3 * PVOL_MAX_K) s_c[threadIdx.x] = 0;
  __syncthreads();
  for (long long g = (long long)blockIdx.x * PVOL_THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * PVOL_THREADS) {
    const long long a = A[g], b = B[g];
    if (a >= 0 && a < K) {
      atomicAdd(&s_c[3 * (int)a + 1], 1);
      if (a == b) atomicAdd(&s_c[3 * (int)a], 1);
    }
    if (b >= 0 && b < K) atomicAdd(&s_c[3 * (int)b + 2], 1);
  }
  __syncthreads();
  if (threadIdx.x < 3 * K && s_c[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], s_c[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------- host side
static inline size_t vol_pad8(size_t b) { return (b + 7) & ~(size_t)7; }
static inline int vol_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline unsigned vol_blocks(long long threads) {
  const long long b = (threads + PVOL_THREADS - 1) / PVOL_THREADS;
  return (unsigned)(b < PVOL_MAX_BLOCKS ? b : PVOL_MAX_BLOCKS);
}

static int vol_check_shape(const char* who, int D, int H, int W) {
  VOL_CHECK_ARG(D >= 1 && D <= PVOL_MAX_DEPTH, "%s: D = %d, need 1 <= D <= %d", who, D, PVOL_MAX_DEPTH);
  VOL_CHECK_ARG(H >= 1 && H <= PVOL_MAX_SIDE && W >= 1 && W <= PVOL_MAX_SIDE, "%s: H = %d, W = %d, need 1 <= H, W <= %d", who, H, W,
                PVOL_MAX_SIDE);
  VOL_CHECK_ARG((long long)D * H * W < (1ll << 31), "%s: D * H * W = %lld, need fewer than 2^31 voxels", who, (long long)D * H * W);
  return 0;
}
static int vol_check_classes(const char* who, int K) {
  VOL_CHECK_ARG(K >= 1 && K <= PVOL_MAX_K, "%s: K = %d, need 1 <= K <= %d", who, K, PVOL_MAX_K);
  return 0;
}
static int vol_check_connectivity(const char* who, int c) {
  VOL_CHECK_ARG(c >= 1 && c <= 3, "%s: connectivity = %d, need 1 (6 neighbours), 2 (18) or 3 (26)", who, c);
  return 0;
}
static int vol_check_spacing(const char* who, float sz, float sy, float sx) {
  VOL_CHECK_ARG(isfinite(sz) && isfinite(sy) && isfinite(sx) && sz > 0.f && sy > 0.f && sx > 0.f,
                "%s: spacing (%g, %g, %g), need finite values > 0", who, (double)sz, (double)sy, (double)sx);
  return 0;
}
static inline bool vol_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline size_t vol_head_bytes(int K) { return vol_pad8((size_t)K * (sizeof(pvol_u64) + 2 * sizeof(int))); }
static inline size_t vol_surface_blocks(long long n) { return (size_t)((n + PVOL_CHUNK - 1) / PVOL_CHUNK); }
static inline size_t vol_surface_bytes(long long n) {
  return vol_pad8(4 * (size_t)n) + vol_pad8(2 * (size_t)n) + 2 * vol_pad8((size_t)n) + vol_pad8(24 * vol_surface_blocks(n));
}

extern "C" int pvol_version(void) { return PVOL_VERSION; }
extern "C" const char* pvol_last_error(void) { return g_vol_err; }

extern "C" size_t pvol_label_workspace(int D, int H, int W) {
  if (vol_check_shape("pvol_label_workspace", D, H, W) != 0) return 0;
  return vol_pad8(4 * (size_t)D * H * W);
}
extern "C" size_t pvol_keep_largest_workspace(int K, int D, int H, int W) {
  if (vol_check_shape("pvol_keep_largest_workspace", D, H, W) != 0 || vol_check_classes("pvol_keep_largest_workspace", K) != 0) return 0;
  return vol_head_bytes(K) + 3 * vol_pad8(4 * (size_t)D * H * W);
}
extern "C" size_t pvol_edt_workspace(int D, int H, int W) {
  if (vol_check_shape("pvol_edt_workspace", D, H, W) != 0) return 0;
  return vol_pad8(2 * (size_t)D * H * W);
}
extern "C" size_t pvol_surface_workspace(int K, int D, int H, int W) {
  if (vol_check_shape("pvol_surface_workspace", D, H, W) != 0 || vol_check_classes("pvol_surface_workspace", K) != 0) return 0;
  if ((long long)K * 2 * ((long long)D * H * W) >= (1ll << 31)) {
    vol_set_error("pvol_surface_workspace: K * 2 * D * H * W = %lld, need fewer than 2^31 distances", (long long)K * 2 * ((long long)D * H * W));
    return 0;
  }
  return vol_surface_bytes((long long)D * H * W);
}

// brick + merge launches: parent = the forest of the volume
template <bool COUNT>
static void vol_build_forest(const long long* cls, int D, int H, int W, int conn, int* parent, int* size, hipStream_t s) {
  const int bx = vol_cdiv(W, PVOL_BW), by = vol_cdiv(H, PVOL_BH), bz = vol_cdiv(D, PVOL_BD);
  const long long nbricks = (long long)bx * by * bz, total = (long long)D * H * W;
  vol_brick_kernel<COUNT><<<dim3((unsigned)(nbricks < PVOL_MAX_BLOCKS ? nbricks : PVOL_MAX_BLOCKS)), dim3(PVOL_THREADS), 0, s>>>(
      cls, D, H, W, bx, by, nbricks, conn, parent, size);
  if (nbricks > 1) vol_merge_kernel<<<dim3(vol_blocks(total)), dim3(PVOL_THREADS), 0, s>>>(cls, D, H, W, total, conn, parent);
}

extern "C" int pvol_label_components(const int64_t* cls, int D, int H, int W, int connectivity, int32_t* labels, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const char* who = "pvol_label_components";
  VOL_CHECK_ARG(cls && labels && workspace, "%s: null pointer (cls %p, labels %p, workspace %p)", who, (const void*)cls, (void*)labels,
                workspace);
  VOL_CHECK_ARG(vol_al(cls, 8) && vol_al(workspace, 8), "%s: cls and the workspace must be 8-byte aligned", who);
  VOL_CHECK_ARG(vol_al(labels, 4), "%s: labels must be 4-byte aligned", who);
  int rc = vol_check_shape(who, D, H, W);
  if (rc != 0) return rc;
  rc = vol_check_connectivity(who, connectivity);
  if (rc != 0) return rc;
  const size_t need = vol_pad8(4 * (size_t)D * H * W);
  VOL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pvol_label_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)workspace;
  const long long total = (long long)D * H * W;
  vol_build_forest<false>((const long long*)cls, D, H, W, connectivity, parent, nullptr, st);
  rc = vol_launched(who);
  if (rc != 0) return rc;
  vol_flatten_kernel<false><<<dim3(vol_blocks(total)), dim3(PVOL_THREADS), 0, st>>>((const long long*)cls, parent, total, 1, labels,
                                                                                     nullptr, nullptr);
  return vol_launched("pvol_label_components (flatten)");
}

extern "C" int pvol_keep_largest_components(const int64_t* cls, int K, int D, int H, int W, int connectivity, int64_t* out, int32_t* stats,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pvol_keep_largest_components";
  VOL_CHECK_ARG(cls && out && stats && workspace, "%s: null pointer (cls %p, out %p, stats %p, workspace %p)", who, (const void*)cls,
                (void*)out, (void*)stats, workspace);
  VOL_CHECK_ARG(vol_al(cls, 8) && vol_al(out, 8) && vol_al(workspace, 8), "%s: cls, out and the workspace must be 8-byte aligned", who);
  VOL_CHECK_ARG(vol_al(stats, 4), "%s: stats must be 4-byte aligned", who);
  int rc = vol_check_classes(who, K);
  if (rc != 0) return rc;
  rc = vol_check_shape(who, D, H, W);
  if (rc != 0) return rc;
  rc = vol_check_connectivity(who, connectivity);
  if (rc != 0) return rc;
  const size_t px = vol_pad8(4 * (size_t)D * H * W), head = vol_head_bytes(K);
  const size_t need = head + 3 * px;
  VOL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pvol_keep_largest_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)workspace;
  pvol_u64* best = (pvol_u64*)p;
  int* ncomp = (int*)(p + (size_t)K * sizeof(pvol_u64));
  int* nvox = ncomp + K;
  int* parent = (int*)(p + head);
  int* size = (int*)(p + head + px);
  int* labels = (int*)(p + head + 2 * px);
  const long long total = (long long)D * H * W;
  const hipError_t e = hipMemsetAsync(p, 0, head, st);
  if (e != hipSuccess) {
    vol_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  vol_build_forest<true>((const long long*)cls, D, H, W, connectivity, parent, size, st);
  rc = vol_launched(who);
  if (rc != 0) return rc;
  vol_flatten_kernel<true><<<dim3(vol_blocks(total)), dim3(PVOL_THREADS), 0, st>>>((const long long*)cls, parent, total, K, labels, size,
                                                                                    ncomp);
  vol_select_kernel<<<dim3(vol_blocks(total)), dim3(PVOL_THREADS), 0, st>>>((const long long*)cls, labels, size, total, K, best, nvox);
  vol_apply_kernel<<<dim3(vol_blocks(total)), dim3(PVOL_THREADS), 0, st>>>((const long long*)cls, labels, best, ncomp, nvox, total, K,
                                                                            (long long*)out, stats);
  return vol_launched("pvol_keep_largest_components (flatten / select / apply)");
}

// the three passes on `mask` (0 = a zero voxel); the x pass restricted to want[i] == 0 when want is given
static int vol_edt_launch(const char* who, const unsigned char* mask, int D, int H, int W, float sz, float sy, float sx, int squared,
                          float* out, unsigned short* g, const unsigned char* want, hipStream_t st) {
  const long long total = (long long)D * H * W;
  vol_edt_z_kernel<<<dim3((unsigned)vol_cdiv(H * W, PVOL_THREADS)), dim3(PVOL_THREADS), 0, st>>>(mask, D, H * W, g);
  vol_edt_y_kernel<<<dim3((unsigned)((total + PVOL_THREADS - 1) / PVOL_THREADS)), dim3(PVOL_THREADS), 0, st>>>(g, H, W, total, sz, sy, out);
  vol_edt_x_kernel<<<dim3((unsigned)((long long)D * H)), dim3(PVOL_THREADS), 0, st>>>(out, W, sx, squared, want);
  return vol_launched(who);
}

extern "C" int pvol_edt(const unsigned char* mask, int D, int H, int W, float sz, float sy, float sx, int squared, float* out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pvol_edt";
  VOL_CHECK_ARG(mask && out && workspace, "%s: null pointer (mask %p, out %p, workspace %p)", who, (const void*)mask, (void*)out, workspace);
  VOL_CHECK_ARG(vol_al(out, 4), "%s: out must be 4-byte aligned", who);
  VOL_CHECK_ARG(vol_al(workspace, 8), "%s: the workspace must be 8-byte aligned", who);
  int rc = vol_check_shape(who, D, H, W);
  if (rc != 0) return rc;
  rc = vol_check_spacing(who, sz, sy, sx);
  if (rc != 0) return rc;
  VOL_CHECK_ARG(squared == 0 || squared == 1, "%s: squared = %d, need 0 or 1", who, squared);
  const size_t need = vol_pad8(2 * (size_t)D * H * W);
  VOL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pvol_edt_workspace)", who, workspace_bytes, need);
  return vol_edt_launch(who, mask, D, H, W, sz, sy, sx, squared, out, (unsigned short*)workspace, nullptr, (hipStream_t)stream);
}

extern "C" int pvol_surface_distances(const int64_t* pred, const int64_t* label, int K, int D, int H, int W, float sz, float sy, float sx,
                                      float* dist, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pvol_surface_distances";
  VOL_CHECK_ARG(pred && label && dist && counts && workspace, "%s: null pointer (pred %p, label %p, dist %p, counts %p, workspace %p)", who,
                (const void*)pred, (const void*)label, (void*)dist, (void*)counts, workspace);
  VOL_CHECK_ARG(vol_al(pred, 8) && vol_al(label, 8) && vol_al(workspace, 8), "%s: pred, label and the workspace must be 8-byte aligned", who);
  VOL_CHECK_ARG(vol_al(dist, 4) && vol_al(counts, 4), "%s: dist and counts must be 4-byte aligned", who);
  int rc = vol_check_classes(who, K);
  if (rc != 0) return rc;
  rc = vol_check_shape(who, D, H, W);
  if (rc != 0) return rc;
  rc = vol_check_spacing(who, sz, sy, sx);
  if (rc != 0) return rc;
  const long long n = (long long)D * H * W;
  VOL_CHECK_ARG((long long)K * 2 * n < (1ll << 31), "%s: K * 2 * D * H * W = %lld, need fewer than 2^31 distances", who, (long long)K * 2 * n);
  const size_t need = vol_surface_bytes(n);
  VOL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pvol_surface_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int nblocks = (int)vol_surface_blocks(n);
  char* p = (char*)workspace;
  float* field = (float*)p;
  p += vol_pad8(4 * (size_t)n);
  unsigned short* g = (unsigned short*)p;
  p += vol_pad8(2 * (size_t)n);
  unsigned char* na = (unsigned char*)p;
  p += vol_pad8((size_t)n);
  unsigned char* nb = (unsigned char*)p;
  p += vol_pad8((size_t)n);
  int* cnt = (int*)p;                       // [4][nblocks]
  int* offs = cnt + 4 * (size_t)nblocks;    // [2][nblocks]
  for (int k = 0; k < K; ++k) {
    vol_surface_kernel<<<dim3((unsigned)nblocks), dim3(PVOL_THREADS), 0, st>>>((const long long*)pred, (const long long*)label, k, D, H, W, n,
                                                                               nblocks, na, nb, cnt);
    vol_scan_kernel<<<dim3(1), dim3(PVOL_THREADS), 0, st>>>(cnt, nblocks, offs, counts + 4 * k);
    rc = vol_launched(who);
    if (rc != 0) return rc;
    for (int dir = 0; dir < 2; ++dir) {
      const unsigned char* from = dir == 0 ? na : nb;          // the surface whose voxels are measured
      const unsigned char* to = dir == 0 ? nb : na;            // the surface they are measured to: the zero voxels of the EDT
      rc = vol_edt_launch(who, to, D, H, W, sz, sy, sx, 0, field, g, from, st);
      if (rc != 0) return rc;
      vol_gather_kernel<<<dim3((unsigned)nblocks), dim3(PVOL_THREADS), 0, st>>>(from, field, offs + (size_t)dir * nblocks, n,
                                                                                dist + ((size_t)k * 2 + dir) * (size_t)n);
      rc = vol_launched("pvol_surface_distances (gather)");
      if (rc != 0) return rc;
    }
  }
  return 0;
}

extern "C" int pvol_dice_counts(const int64_t* pred, const int64_t* label, int K, int D, int H, int W, int32_t* counts, void* stream) {
  const char* who = "pvol_dice_counts";
  VOL_CHECK_ARG(pred && label && counts, "%s: null pointer (pred %p, label %p, counts %p)", who, (const void*)pred, (const void*)label,
                (void*)counts);
  VOL_CHECK_ARG(vol_al(pred, 8) && vol_al(label, 8), "%s: pred and label must be 8-byte aligned", who);
  VOL_CHECK_ARG(vol_al(counts, 4), "%s: counts must be 4-byte aligned", who);
  int rc = vol_check_classes(who, K);
  if (rc != 0) return rc;
  rc = vol_check_shape(who, D, H, W);
  if (rc != 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(int), st);
  if (e != hipSuccess) {
    vol_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  const long long total = (long long)D * H * W;
  const long long blocks = (total + 8 * PVOL_THREADS - 1) / (8 * PVOL_THREADS);      // about eight voxels per thread
  vol_dice_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(PVOL_THREADS), 0, st>>>((const long long*)pred,
                                                                                                  (const long long*)label, total, K, counts);
  return vol_launched(who);
}
