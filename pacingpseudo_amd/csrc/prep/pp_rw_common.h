// What the two random-walker libraries share (pp_random_walker.hip -> libpacingpseudo_prep.so, pp_rw_prior.hip ->
// libpacingpseudo_rwp.so): the size tables, the fixed-order block sums, the edge weights with their kernel, and the host-side
// argument checks.  Everything is static or inline: each library compiles its own copy, none exports a symbol of this file.
#ifndef PP_RW_COMMON_H
#define PP_RW_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define PPREP_ERR_ARG (-1)
#define PPREP_ERR_UNSUPPORTED (-2)

#define RW_THREADS 1024
#define RW_WAVES (RW_THREADS / 64)
#define RW_CHUNK 64                 // slices per launch: their sizes travel in the kernel arguments
#define RW_MAX_K 32
#define RW_MAX_DIM 1024

static thread_local char g_prep_err[512] = "";

static void prep_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_prep_err, sizeof(g_prep_err), fmt, ap);
  va_end(ap);
}

#define PREP_CHECK_ARG(cond, ...)    \
  do {                               \
    if (!(cond)) {                   \
      prep_set_error(__VA_ARGS__);   \
      return PPREP_ERR_ARG;          \
    }                                \
  } while (0)
#define PREP_CHECK_SIZE(cond, ...)   \
  do {                               \
    if (!(cond)) {                   \
      prep_set_error(__VA_ARGS__);   \
      return PPREP_ERR_UNSUPPORTED;  \
    }                                \
  } while (0)

struct RwSizes {
  unsigned short h[RW_CHUNK], w[RW_CHUNK];
};

// ---- fixed-order block sums ----
__device__ __forceinline__ double rw_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;                                                     // lane 0 holds the wave's sum
}
// `s`: RW_WAVES doubles of LDS that no thread may still be reading (the callers alternate between arrays with a barrier between
// the last read of one and its next write)
__device__ __forceinline__ double rw_block_sum(double v, double* s) {
  v = rw_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < RW_WAVES; ++i) t += s[i];
  return t;
}
__device__ __forceinline__ void rw_block_sum2(double a, double b, double* sa, double* sb, double* out_a, double* out_b) {
  a = rw_wave_sum(a);
  b = rw_wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sa[threadIdx.x >> 6] = a;
    sb[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  double ta = 0.0, tb = 0.0;
  for (int i = 0; i < RW_WAVES; ++i) {
    ta += sa[i];
    tb += sb[i];
  }
  *out_a = ta;
  *out_b = tb;
}

// w_ij of two pixel values: symmetric bit for bit (the difference only changes sign)
__device__ __forceinline__ float rw_edge(float a, float b, double inv, float beta, float eps) {
  const float d = (float)(((double)a - (double)b) * inv);
  return expf(-(beta * (d * d))) + eps;
}

// One block per slice: mean and population std of the image (double, two passes), the two weight planes, the diagonal and the
// mask of seeded classes.  `shift` is added to the diagonal of the unknown pixels: 0 for the plain walker (x + 0 = x, the same
// bits), gamma for the walker with priors.  The diagonal is written as 0 at seeds.
static __global__ __launch_bounds__(RW_THREADS) void rw_weights_kernel(const float* __restrict__ img, const int* __restrict__ scb, RwSizes sz,
                                                                        int n0, int K, int H, int W, float beta, float eps, float shift,
                                                                        float* __restrict__ w_right, float* __restrict__ w_down,
                                                                        float* __restrict__ diag, unsigned* __restrict__ mask) {
  __shared__ double s0[RW_WAVES], s1[RW_WAVES];
  __shared__ unsigned s_mask;
  const int n = n0 + blockIdx.x, h = sz.h[blockIdx.x], w = sz.w[blockIdx.x], np = h * w;
  const size_t base = (size_t)n * H * W;
  img += base, scb += base, w_right += base, w_down += base, diag += base;
  if (threadIdx.x == 0) s_mask = 0u;
  double acc = 0.0;
  unsigned m = 0u;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, x = i - y * w, o = y * W + x;
    acc += (double)img[o];
    const int s = scb[o];
    if (s >= 0 && s < K) m |= 1u << s;
  }
  const double mean = rw_block_sum(acc, s0) / (double)np;       // its barrier also orders the reset of s_mask before the ORs
  if (m) atomicOr(&s_mask, m);
  acc = 0.0;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, x = i - y * w;
    const double d = (double)img[y * W + x] - mean;
    acc += d * d;
  }
  const double var = rw_block_sum(acc, s1) / (double)np;        // ... and the ORs before the read below
  const double inv = 1.0 / (sqrt(var) + 1e-8);
  if (threadIdx.x == 0) mask[n] = s_mask;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, x = i - y * w, o = y * W + x;
    const float c = img[o];
    const float wl = x > 0 ? rw_edge(c, img[o - 1], inv, beta, eps) : 0.f;
    const float wr = x + 1 < w ? rw_edge(c, img[o + 1], inv, beta, eps) : 0.f;
    const float wu = y > 0 ? rw_edge(c, img[o - W], inv, beta, eps) : 0.f;
    const float wd = y + 1 < h ? rw_edge(c, img[o + W], inv, beta, eps) : 0.f;
    const int s = scb[o];
    w_right[o] = wr;
    w_down[o] = wd;
    diag[o] = (s >= 0 && s < K) ? 0.f : (((wl + wr) + wu) + wd) + shift;
  }
}

// ---- host side ----
static size_t rw_mask_bytes(int N) { return (((size_t)N * sizeof(unsigned)) + 255) & ~(size_t)255; }

static int rw_check_shape(const char* who, const int* sizes, int N, int K, int H, int W) {
  PREP_CHECK_ARG(N >= 1, "%s: N = %d, need N >= 1", who, N);
  PREP_CHECK_ARG(K >= 1, "%s: K = %d, need K >= 1", who, K);
  PREP_CHECK_ARG(H >= 1 && W >= 1, "%s: H = %d, W = %d, need H, W >= 1", who, H, W);
  PREP_CHECK_SIZE(K <= RW_MAX_K, "%s: K = %d, the kernels run K <= %d", who, K, RW_MAX_K);
  PREP_CHECK_SIZE(H <= RW_MAX_DIM && W <= RW_MAX_DIM, "%s: H = %d, W = %d, the kernels run H, W <= %d", who, H, W, RW_MAX_DIM);
  if (sizes)
    for (int n = 0; n < N; ++n) {
      const int h = sizes[2 * n], w = sizes[2 * n + 1];
      PREP_CHECK_ARG(h >= 1 && h <= H && w >= 1 && w <= W, "%s: sizes[%d] = (%d, %d) does not lie inside the %d x %d plane", who, n, h,
                     w, H, W);
    }
  return 0;
}

static RwSizes rw_chunk_sizes(const int* sizes, int n0, int cnt, int H, int W) {
  RwSizes sz;
  for (int j = 0; j < RW_CHUNK; ++j) {
    const bool in = j < cnt;
    sz.h[j] = (unsigned short)(in ? (sizes ? sizes[2 * (n0 + j)] : H) : 1);
    sz.w[j] = (unsigned short)(in ? (sizes ? sizes[2 * (n0 + j) + 1] : W) : 1);
  }
  return sz;
}

static int rw_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    prep_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

#endif
