// pp_distance.hip -- libpacingpseudo_dist.so (include/pacingpseudo_dist.h): exact Euclidean distance transforms and the boundary
// loss (Kervadec et al., MIDL 2019).  Four kernels and a one-block reduction:
//   * dist_column_kernel   one thread per column segment (threads across x: every load and store of a wave is to 64 consecutive
//                          elements), two sweeps along y; for every class k the distance IN PIXELS to the nearest pixel of the
//                          column whose membership of S_k differs, as 16 bits (0xFFFF: none).  No one-hot planes: the K planes
//                          come from the K pairs of "last row inside / last row outside" a thread keeps in registers;
//   * dist_row_kernel      one block per row of one (n, k) plane: the row of (g sy)^2 staged in LDS as a pixel inside and as a
//                          pixel outside S sees it, then an outward scan per pixel that stops once (dx sx)^2 >= the best candidate -- exact, and short
//                          on real labels.  A row whose pixels all share one membership and have no finite g is not scanned;
//   * dist_bl_fwd_kernel   one thread per pixel, the K logits in registers (class bounds 8 / 16 / 32 as in the loss kernels), the
//                          pixel's term and the block's partial sum in double;
//   * dist_bl_reduce_kernel one block adds the partial sums in a fixed order: no atomics, same bits in every run;
//   * dist_bl_bwd_kernel   the soft-max recomputed, dz written.
// Self-contained on purpose: the per-step library's symbol list is fixed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "pacingpseudo_dist.h"

#define PDIST_VERSION 100
#define PDIST_THREADS 256
#define PDIST_COL_THREADS 64
#define PDIST_MAX_K 32
#define PDIST_MAX_SIDE 2048
#define PDIST_NONE 0xFFFF
#define PDIST_MIN_SEGMENT 16
#define PDIST_MAX_SEGMENTS 16

static thread_local char g_dist_err[512] = "";

static void dist_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_dist_err, sizeof(g_dist_err), fmt, ap);
  va_end(ap);
}

#define DIST_CHECK_ARG(cond, ...)   \
  do {                              \
    if (!(cond)) {                  \
      dist_set_error(__VA_ARGS__);  \
      return -1;                    \
    }                               \
  } while (0)

static int dist_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dist_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- membership
// EDT: the one set of a plane is its non-zero pixels (class 0), a zero pixel belongs to no class.  Signed maps: the pixel's class,
// -1 for a value outside [0, K).
template <bool EDT>
__device__ __forceinline__ int dist_class_at(const void* __restrict__ src, size_t i, int K) {
  if (EDT) return reinterpret_cast<const unsigned char*>(src)[i] != 0 ? 0 : -1;
  const long long v = reinterpret_cast<const long long*>(src)[i];
  return (v >= 0 && v < (long long)K) ? (int)v : -1;
}

// ---------------------------------------------------------------------------------------------------------------- column pass
// A column is cut into `nseg` segments of `seg` rows, one thread per (image, segment, column).  What a sweep carries from row to
// row -- per class the last row inside and the last row outside -- a thread rebuilds for its segment by reading the class map from
// the column's end up to the segment (loads only, no stores: they pipeline, and the map stays in L2), then it sweeps its own rows.
// At most PDIST_MAX_SEGMENTS segments, so the map is read at most that many times over.
template <int MK>
__device__ __forceinline__ void dist_note(int c, int y, int K, int lastin[MK], int lastout[MK]) {
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    if (k < K) {
      if (c == k) lastin[k] = y; else lastout[k] = y;
    }
  }
}

template <int MK, bool EDT>
__global__ __launch_bounds__(PDIST_COL_THREADS) void dist_column_kernel(const void* __restrict__ src, int N, int K, int H, int W,
                                                                        int seg, int nseg, unsigned short* __restrict__ g) {
  const long long t = (long long)blockIdx.x * PDIST_COL_THREADS + threadIdx.x;
  if (t >= (long long)N * nseg * W) return;
  const int x = (int)(t % W);
  const int ns = (int)(t / W);
  const int n = ns / nseg, y0 = (ns - n * nseg) * seg;
  const int y1 = y0 + seg < H ? y0 + seg : H;
  const size_t HW = (size_t)H * W;
  const size_t sbase = (size_t)n * HW + (size_t)x;
  unsigned short* __restrict__ gp = g + (size_t)n * K * HW + (size_t)x;
  int lastin[MK], lastout[MK];
#pragma unroll
  for (int k = 0; k < MK; ++k) lastin[k] = lastout[k] = -1;
#pragma unroll 4
  for (int y = 0; y < y0; ++y) dist_note<MK>(dist_class_at<EDT>(src, sbase + (size_t)y * W, K), y, K, lastin, lastout);
  for (int y = y0; y < y1; ++y) {
    const int c = dist_class_at<EDT>(src, sbase + (size_t)y * W, K);
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      if (k < K) {
        const int lo = c == k ? lastout[k] : lastin[k];
        gp[(size_t)k * HW + (size_t)y * W] = (unsigned short)(lo >= 0 ? y - lo : PDIST_NONE);
      }
    }
    dist_note<MK>(c, y, K, lastin, lastout);
  }
#pragma unroll
  for (int k = 0; k < MK; ++k) lastin[k] = lastout[k] = -1;
#pragma unroll 4
  for (int y = H - 1; y >= y1; --y) dist_note<MK>(dist_class_at<EDT>(src, sbase + (size_t)y * W, K), y, K, lastin, lastout);
  for (int y = y1 - 1; y >= y0; --y) {
    const int c = dist_class_at<EDT>(src, sbase + (size_t)y * W, K);
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      if (k < K) {
        const int lo = c == k ? lastout[k] : lastin[k];
        const int d = lo >= 0 ? lo - y : PDIST_NONE;
        const size_t at = (size_t)k * HW + (size_t)y * W;
        const int up = gp[at];
        if (d < up) gp[at] = (unsigned short)d;
      }
    }
    dist_note<MK>(c, y, K, lastin, lastout);
  }
}

// ---------------------------------------------------------------------------------------------------------------- row pass
// With g2(x') = (g(y, x') sy)^2 (+inf where the column has no pixel of the other membership), the candidate that column x' offers a
// pixel at x is g2(x') when both pixels have the same membership and 0 otherwise (the pixel (y, x') itself is of the other
// membership), plus ((x - x') sx)^2.  Both views of the row are staged: cost[1] as a pixel inside S sees it, cost[0] as a pixel
// outside does.  fl(a + b) >= b for a >= 0, so once (dx sx)^2 >= best no candidate further out can be smaller: the scan is exact.
// An index past an end of the row is clamped to it: that column was met before at a smaller dx, so its candidate cannot win.
template <bool EDT>
__global__ __launch_bounds__(PDIST_THREADS) void dist_row_kernel(const void* __restrict__ src, int K, int H, int W,
                                                                 const unsigned short* __restrict__ g, float sy, float sx, float off,
                                                                 int squared, float* __restrict__ out) {
  __shared__ float cost[2][PDIST_MAX_SIDE];
  const unsigned b = blockIdx.x;
  const int y = (int)(b % (unsigned)H);
  const unsigned pk = b / (unsigned)H;
  const int k = (int)(pk % (unsigned)K);
  const size_t n = pk / (unsigned)K;
  const size_t sbase = (n * H + (size_t)y) * W;
  const size_t obase = ((size_t)pk * H + (size_t)y) * W;
  const bool in0 = dist_class_at<EDT>(src, sbase, K) == k;
  int busy = 0;
  for (int x = threadIdx.x; x < W; x += PDIST_THREADS) {
    const bool in = dist_class_at<EDT>(src, sbase + x, K) == k;
    const int gv = g[obase + x];
    float g2 = INFINITY;
    if (gv != PDIST_NONE) {
      const float gy = (float)gv * sy;
      g2 = gy * gy;
    }
    cost[1][x] = in ? g2 : 0.f;
    cost[0][x] = in ? 0.f : g2;
    busy |= (gv != PDIST_NONE) | (in != in0);
  }
  busy = __syncthreads_or(busy);      // the barrier behind the stores to cost[] as well
  for (int x = threadIdx.x; x < W; x += PDIST_THREADS) {
    const bool in = dist_class_at<EDT>(src, sbase + x, K) == k;
    const float* __restrict__ c = cost[in ? 1 : 0];
    float best = c[x];
    if (busy && (!EDT || in)) {
      float df = 0.f;
      for (int d = 1; d < W; ++d) {
        df += 1.f;
        const float dx = df * sx;
        const float dx2 = dx * dx;
        if (dx2 >= best) break;
        const int xl = x - d > 0 ? x - d : 0, xr = x + d < W - 1 ? x + d : W - 1;
        best = fminf(best, fminf(c[xl], c[xr]) + dx2);
      }
    }
    float v;
    if (EDT) {
      v = in ? (squared ? best : sqrtf(best)) : 0.f;
    } else if (best == INFINITY) {
      v = 0.f;                          // S empty or the whole image: no boundary, no force
    } else {
      const float r = sqrtf(best);
      v = in ? -(r - off) : r;
    }
    out[obase + x] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- boundary loss
__device__ __forceinline__ double dist_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the soft-max numerators e[k] (max-subtracted) of pixel `base`, their sum in s; returns sum_{k in I} e_k phi_k in double
template <int MK>
__device__ __forceinline__ double dist_pixel(const float* __restrict__ z, const float* __restrict__ phi, size_t base, int K, int HW,
                                             int k0, float e[MK], float f[MK], float* s_out) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    e[k] = k < K ? z[base + (size_t)k * HW] : -INFINITY;
    f[k] = (k < K && k >= k0) ? phi[base + (size_t)k * HW] : 0.f;
    mx = fmaxf(mx, e[k]);
  }
  float s = 0.f;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    e[k] = k < K ? expf(e[k] - mx) : 0.f;
    s += e[k];
    acc += (double)e[k] * (double)f[k];
  }
  *s_out = s;
  return acc;
}

template <int MK>
__global__ __launch_bounds__(PDIST_THREADS) void dist_bl_fwd_kernel(const float* __restrict__ z, const float* __restrict__ phi, int K,
                                                                    int HW, long long total, int k0, double* __restrict__ partial) {
  const long long i = (long long)blockIdx.x * PDIST_THREADS + threadIdx.x;      // pixel index in (N, HW)
  double term = 0.0;
  if (i < total) {
    const long long n = i / HW, px = i - n * HW;
    float e[MK], f[MK], s;
    const double acc = dist_pixel<MK>(z, phi, (size_t)n * K * HW + (size_t)px, K, HW, k0, e, f, &s);
    term = acc / (double)s;
  }
  __shared__ double sh[PDIST_THREADS / 64];
  const double w = dist_wave_sum_d(term);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(PDIST_THREADS) void dist_bl_reduce_kernel(const double* __restrict__ partial, int nblocks, double inv_count,
                                                                       float* __restrict__ loss) {
  __shared__ double sh[PDIST_THREADS / 64];
  double a = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += PDIST_THREADS) a += partial[i];
  a = dist_wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) * inv_count);
}

template <int MK>
__global__ __launch_bounds__(PDIST_THREADS) void dist_bl_bwd_kernel(const float* __restrict__ z, const float* __restrict__ phi, int K,
                                                                    int HW, long long total, int k0, float inv_count,
                                                                    const float* __restrict__ grad, float* __restrict__ dz) {
  const long long i = (long long)blockIdx.x * PDIST_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long n = i / HW, px = i - n * HW;
  const size_t base = (size_t)n * K * HW + (size_t)px;
  float e[MK], f[MK], s;
  const double acc = dist_pixel<MK>(z, phi, base, K, HW, k0, e, f, &s);
  const float inv = 1.f / s;
  const float mean = (float)(acc / (double)s);      // sum_{k in I} p_k phi_k
  const float scale = grad[0] * inv_count;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) dz[base + (size_t)k * HW] = scale * (e[k] * inv) * (f[k] - mean);      // f[k] is 0 outside I
}

// ---------------------------------------------------------------------------------------------------------------- host side
template <typename F>
static inline void dist_by_class_bound(int K, F&& f) {
  if (K <= 8) f(std::integral_constant<int, 8>());
  else if (K <= 16) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, PDIST_MAX_K>());
}

static int dist_check_shape(const char* who, int N, int K, int H, int W) {
  DIST_CHECK_ARG(K >= 1 && K <= PDIST_MAX_K, "%s: K = %d, need 1 <= K <= %d", who, K, PDIST_MAX_K);
  DIST_CHECK_ARG(N >= 1, "%s: N = %d, need N >= 1", who, N);
  DIST_CHECK_ARG(H >= 1 && H <= PDIST_MAX_SIDE && W >= 1 && W <= PDIST_MAX_SIDE, "%s: H = %d, W = %d, need 1 <= H, W <= %d", who, H, W,
                 PDIST_MAX_SIDE);
  // N * K * H * W < 2^31, without overflowing on the way (H * W <= 2^22, K <= 2^5)
  DIST_CHECK_ARG((long long)N * K * ((long long)H * W) < (1ll << 31), "%s: N * K * H * W = %lld, need fewer than 2^31 elements", who,
                 (long long)N * K * ((long long)H * W));
  return 0;
}

static int dist_check_spacing(const char* who, float sy, float sx) {
  DIST_CHECK_ARG(isfinite(sy) && isfinite(sx) && sy > 0.f && sx > 0.f, "%s: spacing (%g, %g), need finite values > 0", who, (double)sy,
                 (double)sx);
  return 0;
}

static inline size_t dist_g_bytes(int N, int K, int H, int W) { return (((size_t)N * K * H * W * sizeof(unsigned short)) + 7) & ~(size_t)7; }
// rows per segment of the column pass and the number of segments: at least PDIST_MIN_SEGMENT rows, at most PDIST_MAX_SEGMENTS segments
static inline void dist_segments(int H, int* seg, int* nseg) {
  int s = (H + PDIST_MAX_SEGMENTS - 1) / PDIST_MAX_SEGMENTS;
  if (s < PDIST_MIN_SEGMENT) s = PDIST_MIN_SEGMENT;
  *seg = s;
  *nseg = (H + s - 1) / s;
}
static inline long long dist_pixel_blocks(int N, int H, int W) { return ((long long)N * H * W + PDIST_THREADS - 1) / PDIST_THREADS; }

extern "C" int pdist_version(void) { return PDIST_VERSION; }
extern "C" const char* pdist_last_error(void) { return g_dist_err; }

extern "C" size_t pdist_edt_workspace(int P, int H, int W) {
  if (dist_check_shape("pdist_edt_workspace", P, 1, H, W) != 0) return 0;
  return dist_g_bytes(P, 1, H, W);
}

extern "C" size_t pdist_signed_maps_workspace(int N, int K, int H, int W) {
  if (dist_check_shape("pdist_signed_maps_workspace", N, K, H, W) != 0) return 0;
  return dist_g_bytes(N, K, H, W);
}

extern "C" size_t pdist_boundary_loss_workspace(int N, int K, int H, int W) {
  if (dist_check_shape("pdist_boundary_loss_workspace", N, K, H, W) != 0) return 0;
  return (size_t)dist_pixel_blocks(N, H, W) * sizeof(double);
}

extern "C" int pdist_edt(const unsigned char* mask, int P, int H, int W, float sy, float sx, int squared, float* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const char* who = "pdist_edt";
  DIST_CHECK_ARG(mask && out && workspace, "%s: null pointer (mask %p, out %p, workspace %p)", who, (const void*)mask, (void*)out,
                 workspace);
  DIST_CHECK_ARG(((uintptr_t)out & 3) == 0, "%s: out must be 4-byte aligned", who);
  DIST_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  int rc = dist_check_shape(who, P, 1, H, W);
  if (rc != 0) return rc;
  rc = dist_check_spacing(who, sy, sx);
  if (rc != 0) return rc;
  DIST_CHECK_ARG(squared == 0 || squared == 1, "%s: squared = %d, need 0 or 1", who, squared);
  const size_t need = dist_g_bytes(P, 1, H, W);
  DIST_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pdist_edt_workspace)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* g = (unsigned short*)workspace;
  int seg, nseg;
  dist_segments(H, &seg, &nseg);
  const unsigned cblocks = (unsigned)(((long long)P * nseg * W + PDIST_COL_THREADS - 1) / PDIST_COL_THREADS);
  dist_column_kernel<1, true><<<dim3(cblocks), dim3(PDIST_COL_THREADS), 0, st>>>(mask, P, 1, H, W, seg, nseg, g);
  rc = dist_launched(who);
  if (rc != 0) return rc;
  dist_row_kernel<true><<<dim3((unsigned)((long long)P * H)), dim3(PDIST_THREADS), 0, st>>>(mask, 1, H, W, g, sy, sx, 0.f, squared, out);
  return dist_launched("pdist_edt (row pass)");
}

extern "C" int pdist_signed_maps(const long long* class_map, int N, int K, int H, int W, float sy, float sx, float* phi,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pdist_signed_maps";
  DIST_CHECK_ARG(class_map && phi && workspace, "%s: null pointer (class_map %p, phi %p, workspace %p)", who, (const void*)class_map,
                 (void*)phi, workspace);
  DIST_CHECK_ARG(((uintptr_t)phi & 3) == 0, "%s: phi must be 4-byte aligned", who);
  DIST_CHECK_ARG((((uintptr_t)class_map | (uintptr_t)workspace) & 7) == 0, "%s: class_map and the workspace must be 8-byte aligned", who);
  int rc = dist_check_shape(who, N, K, H, W);
  if (rc != 0) return rc;
  rc = dist_check_spacing(who, sy, sx);
  if (rc != 0) return rc;
  const size_t need = dist_g_bytes(N, K, H, W);
  DIST_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pdist_signed_maps_workspace)", who, workspace_bytes,
                 need);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* g = (unsigned short*)workspace;
  int seg, nseg;
  dist_segments(H, &seg, &nseg);
  const unsigned cblocks = (unsigned)(((long long)N * nseg * W + PDIST_COL_THREADS - 1) / PDIST_COL_THREADS);
  dist_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    dist_column_kernel<MK, false><<<dim3(cblocks), dim3(PDIST_COL_THREADS), 0, st>>>(class_map, N, K, H, W, seg, nseg, g);
  });
  rc = dist_launched(who);
  if (rc != 0) return rc;
  const float off = sy < sx ? sy : sx;
  dist_row_kernel<false><<<dim3((unsigned)((long long)N * K * H)), dim3(PDIST_THREADS), 0, st>>>(class_map, K, H, W, g, sy, sx, off, 0,
                                                                                                phi);
  return dist_launched("pdist_signed_maps (row pass)");
}

extern "C" int pdist_boundary_loss_fwd(const float* logits, const float* phi, int N, int K, int H, int W, float* loss, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  const char* who = "pdist_boundary_loss_fwd";
  DIST_CHECK_ARG(logits && phi && loss && workspace, "%s: null pointer (logits %p, phi %p, loss %p, workspace %p)", who,
                 (const void*)logits, (const void*)phi, (void*)loss, workspace);
  DIST_CHECK_ARG((((uintptr_t)logits | (uintptr_t)phi | (uintptr_t)loss) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  DIST_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  const int rc = dist_check_shape(who, N, K, H, W);
  if (rc != 0) return rc;
  const long long blocks = dist_pixel_blocks(N, H, W);
  const size_t need = (size_t)blocks * sizeof(double);
  DIST_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (pdist_boundary_loss_workspace)", who, workspace_bytes,
                 need);
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)N * H * W;
  const int k0 = K > 1 ? 1 : 0;
  double* partial = (double*)workspace;
  dist_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    dist_bl_fwd_kernel<MK><<<dim3((unsigned)blocks), dim3(PDIST_THREADS), 0, st>>>(logits, phi, K, H * W, total, k0, partial);
  });
  const int e = dist_launched(who);
  if (e != 0) return e;
  const double inv_count = 1.0 / ((double)total * (double)(K - k0));
  dist_bl_reduce_kernel<<<dim3(1), dim3(PDIST_THREADS), 0, st>>>(partial, (int)blocks, inv_count, loss);
  return dist_launched("pdist_boundary_loss_fwd (reduce)");
}

extern "C" int pdist_boundary_loss_bwd(const float* logits, const float* phi, int N, int K, int H, int W, const float* grad,
                                       float* dlogits, void* stream) {
  const char* who = "pdist_boundary_loss_bwd";
  DIST_CHECK_ARG(logits && phi && grad && dlogits, "%s: null pointer (logits %p, phi %p, grad %p, dlogits %p)", who, (const void*)logits,
                 (const void*)phi, (const void*)grad, (void*)dlogits);
  DIST_CHECK_ARG((((uintptr_t)logits | (uintptr_t)phi | (uintptr_t)grad | (uintptr_t)dlogits) & 3) == 0,
                 "%s: pointers must be 4-byte aligned", who);
  const int rc = dist_check_shape(who, N, K, H, W);
  if (rc != 0) return rc;
  const long long total = (long long)N * H * W;
  const int k0 = K > 1 ? 1 : 0;
  const float inv_count = (float)(1.0 / ((double)total * (double)(K - k0)));
  dist_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    dist_bl_bwd_kernel<MK><<<dim3((unsigned)dist_pixel_blocks(N, H, W)), dim3(PDIST_THREADS), 0, (hipStream_t)stream>>>(
        logits, phi, K, H * W, total, k0, inv_count, grad, dlogits);
  });
  return dist_launched(who);
}
