// pp_geodesic.hip -- libpacingpseudo_geo.so (include/pacingpseudo_geo.h): geodesic distance transforms of scribble seeds on a guide
// image and the labels taken from them (train_chaos.py --geo_scribbles; DESIGN.md section 7, "Geodesic scribbles").  Four kernels:
//   * geo_normalize_kernel  one workgroup per slice: mean and population deviation over h x w in double (per-thread strided partial
//                           sums, wave shuffle, the waves added in index order: a fixed order), g rounded to fp32 once;
//   * geo_init_kernel       one workgroup per (slice, 64 x 64 tile): reads the scribble once, writes d0 (0 at the seeds of class k,
//                           +inf elsewhere and outside h x w) of all K planes and, into the workspace, one byte per (slice, class,
//                           tile): does the tile hold a seed of the class;
//   * geo_relax_kernel      the hot path.  One workgroup of four waves per (slice, class) plane, no communication between workgroups.
//                           The plane goes through LDS tile by tile: 64 x 64 pixels of d and g with a one-pixel halo, rows padded to
//                           67 floats (an odd pitch: the row sweeps read 64 consecutive floats, the column sweeps 64 floats a pitch
//                           apart, both on distinct banks).  A tile is relaxed to ITS fixed point by rounds of four directional
//                           sweeps, one per wave, all at once: down, up, right, left; a lane owns a column (a row) and takes the three
//                           pixels behind it.  The waves share the tile without barriers inside a round: a pixel is lowered with an
//                           integer atomic minimum on its bit pattern (the values are non-negative floats, which order as their
//                           bits), so it only ever falls, and every value ever held is the fp32 length of a real path.  A round in
//                           which nothing fell saw final values in every read: the fixed point, the same bits in whatever order the
//                           waves ran.  A tile that changed is written back and marks the neighbours whose halo changed in the
//                           workgroup's dirty-tile set (LDS); a PASS is one walk over that set in raster order (odd passes forwards,
//                           even passes backwards), and the loop ends after a pass that changed no pixel;
//   * geo_labels_kernel     one thread per pixel: first arg-min, runner-up, the ratio rule.
// No floating-point atomics, no host round-trip, nothing allocated.  Static LDS: 2 x 66 x 67 x 4 B = 35 376 B plus the tile set.
// Self-contained on purpose: it shares no source with the other libraries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "pacingpseudo_geo.h"

#define PGEO_VERSION 100
#define GEO_THREADS 256
#define GEO_NORM_THREADS 1024
#define GEO_NORM_WAVES (GEO_NORM_THREADS / 64)
#define GEO_CHUNK 64                 // slices per launch: their sizes travel in the kernel arguments
#define GEO_MAX_K 32
#define GEO_MAX_DIM 1024
#define GEO_TILE 64
#define GEO_ROWS (GEO_TILE + 2)
#define GEO_PITCH (GEO_TILE + 3)     // 67: odd, see above
#define GEO_MAX_TILES ((GEO_MAX_DIM / GEO_TILE) * (GEO_MAX_DIM / GEO_TILE))
// A round moves the front at least one pixel along a shortest path inside the tile, and no path visits more than 4096 pixels: the
// bound is never reached, it only keeps a tile's loop finite by construction.  (A tile that did reach it would stay in the set.)
#define GEO_MAX_ROUNDS (GEO_TILE * GEO_TILE)
#define GEO_DIAGONAL 1.41421354f     // 0x3FB504F3

#define GEO_ANY 1u
#define GEO_TOP 2u
#define GEO_BOTTOM 4u
#define GEO_LEFT 8u
#define GEO_RIGHT 16u

static thread_local char g_geo_err[512] = "";

static void geo_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_geo_err, sizeof(g_geo_err), fmt, ap);
  va_end(ap);
}

#define GEO_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      geo_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int geo_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    geo_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

struct GeoSizes {
  unsigned short h[GEO_CHUNK], w[GEO_CHUNK];
};

// ---------------------------------------------------------------------------------------------------------------- normalisation
__device__ __forceinline__ double geo_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double geo_block_sum(double v, double* s) {
  v = geo_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < GEO_NORM_WAVES; ++i) t += s[i];
  return t;
}

__global__ __launch_bounds__(GEO_NORM_THREADS) void geo_normalize_kernel(const float* __restrict__ img, GeoSizes sz, int n0, int H, int W,
                                                                         float* __restrict__ g) {
  __shared__ double s0[GEO_NORM_WAVES], s1[GEO_NORM_WAVES];
  const int h = sz.h[blockIdx.x], w = sz.w[blockIdx.x], np = h * w, HW = H * W;
  const size_t base = (size_t)(n0 + blockIdx.x) * HW;
  img += base, g += base;
  double acc = 0.0;
  for (int i = threadIdx.x; i < np; i += GEO_NORM_THREADS) {
    const int y = i / w, x = i - y * w;
    acc += (double)img[y * W + x];
  }
  const double mean = geo_block_sum(acc, s0) / (double)np;
  acc = 0.0;
  for (int i = threadIdx.x; i < np; i += GEO_NORM_THREADS) {
    const int y = i / w, x = i - y * w;
    const double d = (double)img[y * W + x] - mean;
    acc += d * d;
  }
  const double den = sqrt(geo_block_sum(acc, s1) / (double)np) + 1e-8;
  for (int i = threadIdx.x; i < HW; i += GEO_NORM_THREADS) {
    const int y = i / W, x = i - y * W;
    g[i] = (y < h && x < w) ? (float)(((double)img[i] - mean) / den) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- d0 and the seeded tiles
__global__ __launch_bounds__(GEO_THREADS) void geo_init_kernel(const int* __restrict__ scb, GeoSizes sz, int n0, int K, int H, int W, int tX,
                                                               int T, float* __restrict__ dist, unsigned char* __restrict__ seeded) {
  __shared__ unsigned s_mask;
  const int t = blockIdx.x, n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y];
  const int y0 = (t / tX) * GEO_TILE, x0 = (t % tX) * GEO_TILE;
  const size_t HW = (size_t)H * W;
  if (threadIdx.x == 0) s_mask = 0u;
  __syncthreads();
  unsigned m = 0u;
  for (int i = threadIdx.x; i < GEO_TILE * GEO_TILE; i += GEO_THREADS) {
    const int y = y0 + (i >> 6), x = x0 + (i & 63);
    if (y >= H || x >= W) continue;
    const size_t o = (size_t)y * W + x;
    const int s = (y < h && x < w) ? scb[(size_t)n * HW + o] : K;
    if (s >= 0 && s < K) m |= 1u << s;
    for (int k = 0; k < K; ++k) dist[((size_t)n * K + k) * HW + o] = s == k ? 0.f : INFINITY;
  }
  if (m) atomicOr(&s_mask, m);
  __syncthreads();
  if ((int)threadIdx.x < K) seeded[((size_t)n * K + threadIdx.x) * T + t] = (unsigned char)((s_mask >> threadIdx.x) & 1u);
}

// ---------------------------------------------------------------------------------------------------------------- relaxation
// c(p, q) = fl(s + fl(lam |fl(g_p - g_q)|)) and fl(d_p + c): every operation rounded on its own
__device__ __forceinline__ float geo_candidate(float dp, float gp, float gq, float s, float lam) {
#pragma clang fp contract(off)
  const float diff = gp - gq;
  const float edge = lam * fabsf(diff);
  const float cost = s + edge;
  return dp + cost;
}

// pixel q takes the least of the three pixels p0, p0 + stride, p0 + 2 stride behind it (the middle one is the axis neighbour);
// returns whether q fell.  A NaN candidate is never smaller: a NaN pixel is a wall.
__device__ __forceinline__ int geo_relax3(float* sd, const float* __restrict__ sg, int q, int p0, int stride, float lam) {
  volatile float* vd = sd;
  const float cur = vd[q], gq = sg[q];
  float best = cur;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int p = p0 + j * stride;
    const float cand = geo_candidate(vd[p], sg[p], gq, j == 1 ? 1.0f : GEO_DIAGONAL, lam);
    if (cand < best) best = cand;
  }
  int fell = 0;
  if (best < cur) {
    const unsigned old = atomicMin(reinterpret_cast<unsigned*>(sd + q), __float_as_uint(best));
    fell = best < __uint_as_float(old);
  }
  return fell;
}

// what one wave's sweep wrote is in LDS before its next step reads it (one wave: its LDS operations complete in order; the fence
// keeps the compiler from moving them across the step)
__device__ __forceinline__ void geo_step_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One visit of tile t.  Returns whether a pixel of the plane changed (the same value in every thread).
__device__ __forceinline__ int geo_tile(int t, int tX, int h, int w, int W, float lam, const float* __restrict__ g, float* __restrict__ dist, float* sd,
                        float* sg, unsigned char* dirty, unsigned* s_flags) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = t / tX, tx = t - ty * tX;
  const int y0 = ty * GEO_TILE, x0 = tx * GEO_TILE;
  const int th = h - y0 < GEO_TILE ? h - y0 : GEO_TILE, tw = w - x0 < GEO_TILE ? w - x0 : GEO_TILE;
  __syncthreads();                                 // every thread has read dirty[t] and the previous visit's flags
  if (tid == 0) {
    dirty[t] = 0;
    *s_flags = 0u;
  }
  for (int i = tid; i < GEO_ROWS * GEO_ROWS; i += GEO_THREADS) {
    const int r = i / GEO_ROWS, c = i - r * GEO_ROWS;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    const bool in = y >= 0 && y < h && x >= 0 && x < w;
    sd[r * GEO_PITCH + c] = in ? dist[(size_t)y * W + x] : INFINITY;
    sg[r * GEO_PITCH + c] = in ? g[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  int changed = 0, more = 0;
  for (int round = 0; round < GEO_MAX_ROUNDS; ++round) {
    int fell = 0;
    if (wave == 0) {                               // down: row r from row r - 1
      for (int r = 1; r <= th; ++r) {
        if (lane < tw) fell |= geo_relax3(sd, sg, r * GEO_PITCH + lane + 1, (r - 1) * GEO_PITCH + lane, 1, lam);
        geo_step_fence();
      }
    } else if (wave == 1) {                        // up: row r from row r + 1
      for (int r = th; r >= 1; --r) {
        if (lane < tw) fell |= geo_relax3(sd, sg, r * GEO_PITCH + lane + 1, (r + 1) * GEO_PITCH + lane, 1, lam);
        geo_step_fence();
      }
    } else if (wave == 2) {                        // right: column c from column c - 1
      for (int c = 1; c <= tw; ++c) {
        if (lane < th) fell |= geo_relax3(sd, sg, (lane + 1) * GEO_PITCH + c, lane * GEO_PITCH + c - 1, GEO_PITCH, lam);
        geo_step_fence();
      }
    } else {                                       // left: column c from column c + 1
      for (int c = tw; c >= 1; --c) {
        if (lane < th) fell |= geo_relax3(sd, sg, (lane + 1) * GEO_PITCH + c, lane * GEO_PITCH + c + 1, GEO_PITCH, lam);
        geo_step_fence();
      }
    }
    more = __syncthreads_or(fell);
    if (!more) break;
    changed = 1;
  }
  if (changed) {
    unsigned fl = 0u;
    for (int i = tid; i < GEO_TILE * GEO_TILE; i += GEO_THREADS) {
      const int ly = i >> 6, lx = i & 63;
      if (ly >= th || lx >= tw) continue;
      const float v = sd[(ly + 1) * GEO_PITCH + lx + 1];
      const size_t o = (size_t)(y0 + ly) * W + (x0 + lx);
      if (v != dist[o]) {
        dist[o] = v;
        fl |= GEO_ANY | (ly == 0 ? GEO_TOP : 0u) | (ly == th - 1 ? GEO_BOTTOM : 0u) | (lx == 0 ? GEO_LEFT : 0u) |
              (lx == tw - 1 ? GEO_RIGHT : 0u);
      }
    }
    if (fl) atomicOr(s_flags, fl);
    __syncthreads();                               // the flags are complete, the tile is in memory for the next visit's loads
    if (tid == 0) {
      const unsigned f = *s_flags;
      const bool up = (f & GEO_TOP) && ty > 0, down = (f & GEO_BOTTOM) && y0 + GEO_TILE < h;
      const bool left = (f & GEO_LEFT) && tx > 0, right = (f & GEO_RIGHT) && x0 + GEO_TILE < w;
      if (up) dirty[t - tX] = 1;
      if (down) dirty[t + tX] = 1;
      if (left) dirty[t - 1] = 1;
      if (right) dirty[t + 1] = 1;
      if (up && left) dirty[t - tX - 1] = 1;
      if (up && right) dirty[t - tX + 1] = 1;
      if (down && left) dirty[t + tX - 1] = 1;
      if (down && right) dirty[t + tX + 1] = 1;
      if (more) dirty[t] = 1;
    }
  }
  __syncthreads();
  return (*s_flags & GEO_ANY) != 0u;
}

__global__ __launch_bounds__(GEO_THREADS) void geo_relax_kernel(const float* __restrict__ g, GeoSizes sz, int n0, int K, int H, int W,
                                                                int tX, int T, float lam, int max_sweeps,
                                                                const unsigned char* __restrict__ seeded, float* __restrict__ dist,
                                                                int* __restrict__ stats) {
  __shared__ float sd[GEO_ROWS * GEO_PITCH], sg[GEO_ROWS * GEO_PITCH];
  __shared__ unsigned char dirty[GEO_MAX_TILES];
  __shared__ unsigned s_flags;
  const int k = blockIdx.x, n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y];
  const size_t HW = (size_t)H * W, plane = (size_t)n * K + k;
  g += (size_t)n * HW, dist += plane * HW, seeded += plane * T, stats += plane * 2;
  int have = 0;
  for (int t = threadIdx.x; t < T; t += GEO_THREADS) {
    const int f = seeded[t] != 0;
    dirty[t] = (unsigned char)f;
    have |= f;
  }
  if (threadIdx.x == 0) s_flags = 0u;
  have = __syncthreads_or(have);
  if (!have) {                                     // a class without a seed: d0 = +inf is the answer, nothing runs
    if (threadIdx.x == 0) stats[0] = 0, stats[1] = 1;
    return;
  }
  int passes = 0, converged = 0;
  while (passes < max_sweeps) {
    ++passes;
    int any = 0;
    for (int i = 0; i < T; ++i) {
      const int t = (passes & 1) ? i : T - 1 - i;
      if (dirty[t]) any |= geo_tile(t, tX, h, w, W, lam, g, dist, sd, sg, dirty, &s_flags);      // uniform: geo_tile ends on a barrier
    }
    if (!any) {
      converged = 1;
      break;
    }
  }
  if (threadIdx.x == 0) stats[0] = passes, stats[1] = converged;
}

// ---------------------------------------------------------------------------------------------------------------- labels
__device__ __forceinline__ float geo_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__global__ __launch_bounds__(GEO_THREADS) void geo_labels_kernel(const float* __restrict__ dist, const int* __restrict__ scb, GeoSizes sz,
                                                                 int n0, int K, int H, int W, float max_dist, float ratio,
                                                                 int* __restrict__ out) {
  const int n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y], HW = H * W;
  const int i = blockIdx.x * GEO_THREADS + threadIdx.x;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  const size_t o = (size_t)n * HW + i;
  int lab = K;
  if (y < h && x < w) {
    const int s = scb[o];
    if (s >= 0 && s < K) {
      lab = s;
    } else {
      const float* d = dist + (size_t)n * K * HW + i;
      float best = d[0], second = INFINITY;
      int arg = 0;
      for (int k = 1; k < K; ++k) {
        const float v = d[(size_t)k * HW];
        if (v < best) {
          second = best, best = v, arg = k;
        } else if (v < second) {
          second = v;
        }
      }
      if (best < INFINITY && best <= max_dist && best <= geo_mul_rounded(ratio, second)) lab = arg;
    }
  }
  out[o] = lab;
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int geo_check_shape(const char* who, const int* sizes, int N, int K, int H, int W) {
  GEO_CHECK_ARG(N >= 1, "%s: N = %d, need N >= 1", who, N);
  GEO_CHECK_ARG(K >= 1 && K <= GEO_MAX_K, "%s: K = %d, need 1 <= K <= %d", who, K, GEO_MAX_K);
  GEO_CHECK_ARG(H >= 1 && H <= GEO_MAX_DIM && W >= 1 && W <= GEO_MAX_DIM, "%s: H = %d, W = %d, need 1 <= H, W <= %d", who, H, W,
                GEO_MAX_DIM);
  // N * K * H * W < 2^31, without overflowing on the way (H * W <= 2^20, K <= 2^5)
  GEO_CHECK_ARG((long long)N * K * ((long long)H * W) < (1ll << 31), "%s: N * K * H * W = %lld, need fewer than 2^31 elements", who,
                (long long)N * K * ((long long)H * W));
  if (sizes)
    for (int n = 0; n < N; ++n) {
      const int h = sizes[2 * n], w = sizes[2 * n + 1];
      GEO_CHECK_ARG(h >= 1 && h <= H && w >= 1 && w <= W, "%s: sizes[%d] = (%d, %d) does not lie inside the %d x %d plane", who, n, h, w,
                    H, W);
    }
  return 0;
}

static GeoSizes geo_chunk_sizes(const int* sizes, int n0, int cnt, int H, int W) {
  GeoSizes sz;
  for (int j = 0; j < GEO_CHUNK; ++j) {
    const bool in = j < cnt;
    sz.h[j] = (unsigned short)(in ? (sizes ? sizes[2 * (n0 + j)] : H) : 1);
    sz.w[j] = (unsigned short)(in ? (sizes ? sizes[2 * (n0 + j) + 1] : W) : 1);
  }
  return sz;
}

static inline int geo_tiles(int side) { return (side + GEO_TILE - 1) / GEO_TILE; }
static inline size_t geo_ws_bytes(int N, int K, int H, int W) {
  return (((size_t)N * K * geo_tiles(H) * geo_tiles(W)) + 7) & ~(size_t)7;
}

extern "C" int pgeo_version(void) { return PGEO_VERSION; }
extern "C" const char* pgeo_last_error(void) { return g_geo_err; }

extern "C" int pgeo_normalize(const float* img, const int* sizes, int N, int H, int W, float* g, void* stream) {
  const char* who = "pgeo_normalize";
  GEO_CHECK_ARG(img && g, "%s: null pointer (img %p, g %p)", who, (const void*)img, (void*)g);
  GEO_CHECK_ARG((((uintptr_t)img | (uintptr_t)g) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  const int rc = geo_check_shape(who, sizes, N, 1, H, W);
  if (rc != 0) return rc;
  for (int n0 = 0; n0 < N; n0 += GEO_CHUNK) {
    const int cnt = N - n0 < GEO_CHUNK ? N - n0 : GEO_CHUNK;
    const GeoSizes sz = geo_chunk_sizes(sizes, n0, cnt, H, W);
    geo_normalize_kernel<<<dim3(cnt), dim3(GEO_NORM_THREADS), 0, (hipStream_t)stream>>>(img, sz, n0, H, W, g);
    const int e = geo_launched(who);
    if (e != 0) return e;
  }
  return 0;
}

extern "C" size_t pgeo_distance_workspace(int N, int K, int H, int W) {
  if (geo_check_shape("pgeo_distance_workspace", nullptr, N, K, H, W) != 0) return 0;
  return geo_ws_bytes(N, K, H, W);
}

extern "C" int pgeo_distance(const float* g, const int* scb, const int* sizes, int N, int K, int H, int W, float lam, int max_sweeps,
                             float* dist, int* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pgeo_distance";
  GEO_CHECK_ARG(g && scb && dist && stats && workspace, "%s: null pointer (g %p, scb %p, dist %p, stats %p, workspace %p)", who,
                (const void*)g, (const void*)scb, (void*)dist, (void*)stats, workspace);
  GEO_CHECK_ARG((((uintptr_t)g | (uintptr_t)scb | (uintptr_t)dist | (uintptr_t)stats) & 3) == 0, "%s: pointers must be 4-byte aligned",
                who);
  GEO_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  GEO_CHECK_ARG(isfinite(lam) && lam >= 0.f, "%s: lam = %g, need a finite lam >= 0", who, (double)lam);
  GEO_CHECK_ARG(max_sweeps >= 1, "%s: max_sweeps = %d, need max_sweeps >= 1", who, max_sweeps);
  const int rc = geo_check_shape(who, sizes, N, K, H, W);
  if (rc != 0) return rc;
  const size_t need = geo_ws_bytes(N, K, H, W);
  GEO_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pgeo_distance_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* seeded = (unsigned char*)workspace;
  const int tX = geo_tiles(W), T = tX * geo_tiles(H);
  for (int n0 = 0; n0 < N; n0 += GEO_CHUNK) {
    const int cnt = N - n0 < GEO_CHUNK ? N - n0 : GEO_CHUNK;
    const GeoSizes sz = geo_chunk_sizes(sizes, n0, cnt, H, W);
    geo_init_kernel<<<dim3(T, cnt), dim3(GEO_THREADS), 0, st>>>(scb, sz, n0, K, H, W, tX, T, dist, seeded);
    int e = geo_launched("pgeo_distance (seeds)");
    if (e != 0) return e;
    geo_relax_kernel<<<dim3(K, cnt), dim3(GEO_THREADS), 0, st>>>(g, sz, n0, K, H, W, tX, T, lam, max_sweeps, seeded, dist, stats);
    e = geo_launched(who);
    if (e != 0) return e;
  }
  return 0;
}

extern "C" int pgeo_labels(const float* dist, const int* scb, const int* sizes, int N, int K, int H, int W, float max_dist, float ratio,
                           int* out, void* stream) {
  const char* who = "pgeo_labels";
  GEO_CHECK_ARG(dist && scb && out, "%s: null pointer (dist %p, scb %p, out %p)", who, (const void*)dist, (const void*)scb, (void*)out);
  GEO_CHECK_ARG((((uintptr_t)dist | (uintptr_t)scb | (uintptr_t)out) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  GEO_CHECK_ARG(max_dist > 0.f, "%s: max_dist = %g, need max_dist > 0 (+inf allowed)", who, (double)max_dist);
  GEO_CHECK_ARG(ratio > 0.f && ratio <= 1.f, "%s: ratio = %g, need 0 < ratio <= 1", who, (double)ratio);
  const int rc = geo_check_shape(who, sizes, N, K, H, W);
  if (rc != 0) return rc;
  const int HW = H * W;
  for (int n0 = 0; n0 < N; n0 += GEO_CHUNK) {
    const int cnt = N - n0 < GEO_CHUNK ? N - n0 : GEO_CHUNK;
    const GeoSizes sz = geo_chunk_sizes(sizes, n0, cnt, H, W);
    geo_labels_kernel<<<dim3((HW + GEO_THREADS - 1) / GEO_THREADS, cnt), dim3(GEO_THREADS), 0, (hipStream_t)stream>>>(
        dist, scb, sz, n0, K, H, W, max_dist, ratio, out);
    const int e = geo_launched(who);
    if (e != 0) return e;
  }
  return 0;
}
