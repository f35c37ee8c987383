// pp_uncertainty.hip -- libpacingpseudo_unc.so (include/pacingpseudo_unc.h): the uncertainty mask of the mean-teacher consistency
// term.  Three streaming kernels and a one-block reduction:
//   * unc_noise_kernel      x_t = x + clamp(sigma n_t, -c, +c): one Philox-4x32-10 block per element quad, counter-based, so a value
//                           depends on (seed, step, pass, element index) alone; (seed, step) are READ FROM DEVICE MEMORY, which is
//                           what lets a replayed hipGraph draw fresh noise;
//   * unc_accumulate_kernel one thread per pixel, the K logits of a pixel in registers (class bounds 8 / 16 / 32 as in the loss
//                           kernels): max-subtracted soft-max, acc = / += p, and on the last pass pbar, the entropy, the mask and
//                           the per-block partial sums of the three statistics;
//   * unc_reduce_kernel     one block adds the partial sums in a fixed order (as crf_reduce_kernel does): no atomics, same bits
//                           in every run;
//   * unc_advance_kernel    step += 1.
// Self-contained on purpose (its own copy of the generator pp_augment.hip also uses): the per-step library's symbol list is fixed.
// Memory-bound kernels: every access of a wave is to 64 consecutive floats (or 64 consecutive float4 in the noise kernel).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "pacingpseudo_unc.h"

#define PUNC_VERSION 100
#define PUNC_THREADS 256
#define PUNC_MAX_K 32
#define PUNC_MAX_PASSES 16

static thread_local char g_unc_err[512] = "";

static void unc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_unc_err, sizeof(g_unc_err), fmt, ap);
  va_end(ap);
}

#define UNC_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      unc_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int unc_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    unc_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- noise
__device__ __forceinline__ void unc_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                  unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// d[j] = clamp(sigma * n_j, -clip, +clip) of quad q: the ONE expression both access widths store, so their bits agree
__device__ __forceinline__ void unc_quad_noise(unsigned q, unsigned pass, unsigned long long seed, unsigned long long step, float sigma,
                                               float clip, float d[4]) {
  unsigned r[4];
  unc_philox4x32_10(q, pass, (unsigned)step, (unsigned)(step >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u0 = ((float)(r[2 * h] >> 8) + 0.5f) * 5.9604644775390625e-8f;      // (0, 1): 24 bits, never 0 or 1
    const float u1 = ((float)(r[2 * h + 1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float rad = sqrtf(-2.f * logf(u0));
    const float ang = 6.283185307179586f * u1;
    d[2 * h] = fminf(fmaxf(sigma * (rad * cosf(ang)), -clip), clip);
    d[2 * h + 1] = fminf(fmaxf(sigma * (rad * sinf(ang)), -clip), clip);
  }
}

template <bool VEC>
__global__ __launch_bounds__(PUNC_THREADS) void unc_noise_kernel(const float* __restrict__ image, long long n, float sigma, float clip,
                                                                 const unsigned long long* __restrict__ state, unsigned pass,
                                                                 float* __restrict__ out) {
  const unsigned long long seed = state[0], step = state[1];
  const long long quads = (n + 3) >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
    float d[4];
    unc_quad_noise((unsigned)q, pass, seed, step, sigma, clip, d);
    const long long e0 = q << 2;
    if (VEC && e0 + 4 <= n) {
      const float4 x = reinterpret_cast<const float4*>(image)[q];
      float4 y;
      y.x = x.x + d[0]; y.y = x.y + d[1]; y.z = x.z + d[2]; y.w = x.w + d[3];
      reinterpret_cast<float4*>(out)[q] = y;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < n) out[e0 + j] = image[e0 + j] + d[j];
    }
  }
}

__global__ void unc_advance_kernel(unsigned long long* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = state[1] + 1ull;
}

// ---------------------------------------------------------------------------------------------------------------- accumulate
__device__ __forceinline__ double unc_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// MODE 0: first of several passes (acc = p); 1: a middle pass (acc += p); 2: the last pass (pbar from acc + p, or p alone when
// passes == 1: `first`), which writes mask / unc and the block's partial sums partial[block * 3 + {0, 1, 2}].
template <int MK, int MODE>
__global__ __launch_bounds__(PUNC_THREADS) void unc_accumulate_kernel(const float* __restrict__ logits, int K, int HW, long long total,
                                                                      int first, float inv_passes, const float* __restrict__ valid,
                                                                      float threshold, float* __restrict__ acc, float* __restrict__ mask,
                                                                      float* __restrict__ unc, double* __restrict__ partial) {
  const long long i = (long long)blockIdx.x * PUNC_THREADS + threadIdx.x;      // pixel index in (N, HW)
  const bool live = i < total;
  float m = 0.f, u = 0.f, v = 0.f;
  if (live) {
    const long long n = i / HW, px = i - n * HW;
    const size_t base = (size_t)n * K * HW + (size_t)px;
    float p[MK];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      p[k] = k < K ? logits[base + (size_t)k * HW] : -INFINITY;
      mx = fmaxf(mx, p[k]);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      p[k] = k < K ? expf(p[k] - mx) : 0.f;
      s += p[k];
    }
    const float inv = 1.f / s;
    if (MODE == 0) {
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) acc[base + (size_t)k * HW] = p[k] * inv;
    } else if (MODE == 1) {
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) acc[base + (size_t)k * HW] += p[k] * inv;
    } else {
      float h = 0.f;
#pragma unroll
      for (int k = 0; k < MK; ++k) {
        if (k < K) {
          float pb = p[k] * inv;
          if (!first) pb = (acc[base + (size_t)k * HW] + pb) * inv_passes;
          if (pb > 0.f) h -= pb * logf(pb);
        }
      }
      u = h;
      v = valid ? valid[i] : 1.f;
      m = (u < threshold) ? v : 0.f;
      mask[i] = m;
      if (unc) unc[i] = u;
    }
  }
  if (MODE == 2) {
    __shared__ double sh[3][PUNC_THREADS / 64];
    const double a = unc_wave_sum_d((double)m), b = unc_wave_sum_d((double)v * (double)u), c = unc_wave_sum_d((double)v);
    if ((threadIdx.x & 63) == 0) {
      sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; sh[2][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const double* r = sh[threadIdx.x];
      partial[(size_t)blockIdx.x * 3 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
  }
}

__global__ __launch_bounds__(PUNC_THREADS) void unc_reduce_kernel(const double* __restrict__ partial, int nblocks,
                                                                  double* __restrict__ stats) {
  __shared__ double sh[3][PUNC_THREADS / 64];
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += PUNC_THREADS) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] += partial[(size_t)i * 3 + j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a[j] = unc_wave_sum_d(a[j]);
    if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = a[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = sh[threadIdx.x];
    stats[threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
template <typename F>
static inline void unc_by_class_bound(int K, F&& f) {
  if (K <= 8) f(std::integral_constant<int, 8>());
  else if (K <= 16) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, PUNC_MAX_K>());
}

static int unc_check_shape(const char* who, int N, int K, int HW) {
  UNC_CHECK_ARG(K >= 2 && K <= PUNC_MAX_K, "%s: K = %d, need 2 <= K <= %d", who, K, PUNC_MAX_K);
  UNC_CHECK_ARG(N >= 1 && HW >= 1, "%s: N = %d, HW = %d, need N >= 1 and HW >= 1", who, N, HW);
  UNC_CHECK_ARG((long long)N * HW < (1ll << 31), "%s: N * HW = %lld, need fewer than 2^31 pixels", who, (long long)N * HW);
  return 0;
}

static inline long long unc_blocks(int N, int HW) { return ((long long)N * HW + PUNC_THREADS - 1) / PUNC_THREADS; }

extern "C" int punc_version(void) { return PUNC_VERSION; }
extern "C" const char* punc_last_error(void) { return g_unc_err; }

extern "C" size_t punc_workspace_bytes(int N, int K, int HW) {
  if (unc_check_shape("punc_workspace_bytes", N, K, HW) != 0) return 0;
  return (size_t)unc_blocks(N, HW) * 3 * sizeof(double);
}

extern "C" int punc_noise_add(const float* image, long long n, float sigma, float clip, const unsigned long long* state, int pass,
                              float* out, void* stream) {
  const char* who = "punc_noise_add";
  UNC_CHECK_ARG(image && state && out, "%s: null pointer (image %p, state %p, out %p)", who, (const void*)image, (const void*)state,
                (void*)out);
  UNC_CHECK_ARG((((uintptr_t)image | (uintptr_t)out) & 3) == 0, "%s: image and out must be 4-byte aligned", who);
  UNC_CHECK_ARG(((uintptr_t)state & 7) == 0, "%s: state must be 8-byte aligned", who);
  UNC_CHECK_ARG(n >= 1 && n <= (1ll << 34), "%s: n = %lld, need 1 <= n <= 2^34", who, n);
  UNC_CHECK_ARG(sigma >= 0.f && isfinite(sigma), "%s: sigma = %g, need a finite sigma >= 0", who, (double)sigma);
  UNC_CHECK_ARG(clip >= 0.f && isfinite(clip), "%s: clip = %g, need a finite clip >= 0", who, (double)clip);
  UNC_CHECK_ARG(pass >= 0 && pass < PUNC_MAX_PASSES, "%s: pass = %d, need 0 <= pass < %d", who, pass, PUNC_MAX_PASSES);
  const long long quads = (n + 3) >> 2;
  long long blocks = (quads + PUNC_THREADS - 1) / PUNC_THREADS;
  if (blocks > 8192) blocks = 8192;      // grid-stride beyond: 256 CUs x 8 blocks x 4 rounds
  const bool vec = ((((uintptr_t)image | (uintptr_t)out) & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    unc_noise_kernel<true><<<dim3((unsigned)blocks), dim3(PUNC_THREADS), 0, st>>>(image, n, sigma, clip, state, (unsigned)pass, out);
  else
    unc_noise_kernel<false><<<dim3((unsigned)blocks), dim3(PUNC_THREADS), 0, st>>>(image, n, sigma, clip, state, (unsigned)pass, out);
  return unc_launched(who);
}

extern "C" int punc_accumulate(const float* logits, int N, int K, int HW, int pass, int passes, const float* valid_mask,
                               float threshold, float* acc, float* mask, float* unc, double* stats, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const char* who = "punc_accumulate";
  UNC_CHECK_ARG(logits && acc && mask && stats && workspace,
                "%s: null pointer (logits %p, acc %p, mask %p, stats %p, workspace %p)", who, (const void*)logits, (void*)acc,
                (void*)mask, (void*)stats, workspace);
  UNC_CHECK_ARG((((uintptr_t)logits | (uintptr_t)acc | (uintptr_t)mask | (uintptr_t)unc | (uintptr_t)valid_mask) & 3) == 0,
                "%s: pointers must be 4-byte aligned", who);
  UNC_CHECK_ARG((((uintptr_t)stats | (uintptr_t)workspace) & 7) == 0, "%s: stats and the workspace must be 8-byte aligned", who);
  const int rc = unc_check_shape(who, N, K, HW);
  if (rc != 0) return rc;
  UNC_CHECK_ARG(passes >= 1 && passes <= PUNC_MAX_PASSES, "%s: passes = %d, need 1 <= passes <= %d", who, passes, PUNC_MAX_PASSES);
  UNC_CHECK_ARG(pass >= 0 && pass < passes, "%s: pass = %d, need 0 <= pass < passes = %d", who, pass, passes);
  UNC_CHECK_ARG(isfinite(threshold), "%s: threshold = %g, need a finite threshold", who, (double)threshold);
  const size_t need = (size_t)unc_blocks(N, HW) * 3 * sizeof(double);
  UNC_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (punc_workspace_bytes)", who, workspace_bytes, need);
  const long long total = (long long)N * HW;
  const unsigned blocks = (unsigned)unc_blocks(N, HW);
  hipStream_t st = (hipStream_t)stream;
  const bool last = pass == passes - 1;
  double* partial = (double*)workspace;
  const float inv_passes = 1.f / (float)passes;
  unc_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    if (last)
      unc_accumulate_kernel<MK, 2><<<dim3(blocks), dim3(PUNC_THREADS), 0, st>>>(logits, K, HW, total, passes == 1 ? 1 : 0, inv_passes,
                                                                                valid_mask, threshold, acc, mask, unc, partial);
    else if (pass == 0)
      unc_accumulate_kernel<MK, 0><<<dim3(blocks), dim3(PUNC_THREADS), 0, st>>>(logits, K, HW, total, 0, inv_passes, valid_mask,
                                                                                threshold, acc, mask, unc, partial);
    else
      unc_accumulate_kernel<MK, 1><<<dim3(blocks), dim3(PUNC_THREADS), 0, st>>>(logits, K, HW, total, 0, inv_passes, valid_mask,
                                                                                threshold, acc, mask, unc, partial);
  });
  int e = unc_launched(who);
  if (e != 0 || !last) return e;
  unc_reduce_kernel<<<dim3(1), dim3(PUNC_THREADS), 0, st>>>(partial, (int)blocks, stats);
  return unc_launched("punc_accumulate (reduce)");
}

extern "C" int punc_advance(unsigned long long* state, void* stream) {
  const char* who = "punc_advance";
  UNC_CHECK_ARG(state, "%s: null pointer (state)", who);
  UNC_CHECK_ARG(((uintptr_t)state & 7) == 0, "%s: state must be 8-byte aligned", who);
  unc_advance_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(state);
  return unc_launched(who);
}
