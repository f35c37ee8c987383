// libpacingpseudo_opt.so (include/pacingpseudo_opt.h, entry points popt_*, binding pacingpseudo_amd/_opt.py): fused AdamW over one
// flat fp32 parameter slab -- torch.optim.AdamW (non-amsgrad, maximize=False) semantics: the weight decay is DECOUPLED from the
// gradient (p <- p * (1 - lr * wd) before the Adam move, the moments never see it), and a byte mask laid over the slab exempts single
// elements from it (norm affine parameters and biases: FusedAdamW(exempt_1d=True)).  The step count, the learning rate, the overflow
// guard, the clip coefficient and the EMA shadow slab are handled as the pp_adam_step_dev / _clip / _ema entry points of the per-step
// library handle them (pp_optim.hip, which this file leaves alone: that library's symbol list and version are fixed by its tests).
//
// Self-contained: no header of the per-step library, no environment variable, no allocation, no copy, no synchronisation.
// HBM-bound: 16 B per lane, reads p, g, m, v and writes p, m, v once (28 B / parameter, 36 with the shadow slab), plus ONE 4-byte load
// of the mask per lane (1 B / parameter) when a mask is given.  A byte per element rather than a bit: a tensor boundary can fall
// inside a lane (FlatSlab aligns segments, not parameters), and with bytes the lane's four decisions are the four bytes of one
// aligned word whatever the boundary does; a bit mask would save 7/8 B per parameter of 29 and need a shifted two-word read per lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "pacingpseudo_opt.h"

#define POPT_VERSION 100
#define POPT_THREADS 256
#define POPT_MAX_BLOCKS 4096          // the cap of adam_step_impl: one trip of the grid covers 4 * 256 * 4096 elements

static thread_local char g_opt_err[512] = "";

static void opt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_opt_err, sizeof(g_opt_err), fmt, ap);
  va_end(ap);
}

#define OPT_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      opt_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int opt_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    opt_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// gc = fl32(g * coef), rounded on its own: what torch.nn.utils.clip_grad_norm_ leaves in the gradient before the optimizer reads it.
__device__ __forceinline__ float opt_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// pd = fl32(p * f), rounded on its own -- torch's p.mul_(1 - lr * wd); contracted into the Adam move it would round differently.
// f = 1 (no decay, or an exempt element) gives p back exactly.
__device__ __forceinline__ float opt_decay_rounded(float p, float f) {
#pragma clang fp contract(off)
  return p * f;
}

// e <- e + fl32(w * fl32(p - e)): three separately rounded fp32 operations, the torch fp32 chain e + w * (p - e) bit for bit.
__device__ __forceinline__ float opt_ema_rounded(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = w * d;
  return e + s;
}

// w = fl32(1 - min(D, (1 + t) / (10 + t))) in double, t = updates applied to the segment so far.  Rounded once.
__device__ __forceinline__ float opt_ema_weight(double decay, double t) {
  const double warm = (1.0 + t) / (10.0 + t);
  return (float)(1.0 - (decay < warm ? decay : warm));
}

// One element.  f = the decay factor of THIS element (1 where exempt).
#define OPT_ADAMW1(P, G, M, V, E, F)                                     \
  {                                                                      \
    const float gc = CLIP ? opt_mul_rounded((G), coef) : (G);            \
    const float pd = opt_decay_rounded((P), (F));                        \
    (M) = b1 * (M) + (1.f - b1) * gc;                                    \
    (V) = b2 * (V) + (1.f - b2) * gc * gc;                               \
    (P) = pd - step * ((M) / (sqrtf((V)) / sqrt_bc2 + eps));             \
    if constexpr (EMA) (E) = opt_ema_rounded((E), (P), ew);              \
  }

// CLIP: every gradient element is first scaled by the device scalar clip_dev[0].  EMA: the shadow slab e is loaded up front with
// p, g, m, v, moved towards the p held in registers and stored.  MASK: one aligned 4-byte load per lane of `exempt`, byte j of the
// word (little endian) decides element 4 i + j; MASK = false reads no mask at all (the kernel a run without exemption gets).
// A skipped step (skip[0] != 0: the gradients are not finite) returns before any load: p, m, v, e keep their bits, decay included.
template <bool CLIP, bool EMA, bool MASK>
__global__ __launch_bounds__(POPT_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                                             float wd, const int* __restrict__ skip, const int* __restrict__ step_dev,
                                                             const float* __restrict__ lr_dev, const float* __restrict__ clip_dev,
                                                             const unsigned char* __restrict__ exempt, float* __restrict__ e,
                                                             double ema_decay) {
  if (skip && skip[0]) return;          // counted once per optimizer step by opt_commit_kernel
  const int t0 = step_dev[0];           // updates applied to this segment so far; the commit kernel advances it behind this launch
  const double t = (double)(t0 + 1);
  const float bc1 = (float)(1.0 - pow((double)b1, t));
  const float sqrt_bc2 = (float)sqrt(1.0 - pow((double)b2, t));
  if (lr_dev) lr = lr_dev[0];
  const float f = (float)(1.0 - (double)lr * (double)wd);
  const float coef = CLIP ? clip_dev[0] : 1.f;
  const float ew = EMA ? opt_ema_weight(ema_decay, (double)t0) : 0.f;
  const float step = lr / bc1;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EMA) ee = reinterpret_cast<float4*>(e)[i];
    unsigned int mk = 0u;
    if constexpr (MASK) mk = reinterpret_cast<const unsigned int*>(exempt)[i];
    OPT_ADAMW1(pp.x, gg.x, mm.x, vv.x, ee.x, (mk & 0x000000ffu) ? 1.f : f)
    OPT_ADAMW1(pp.y, gg.y, mm.y, vv.y, ee.y, (mk & 0x0000ff00u) ? 1.f : f)
    OPT_ADAMW1(pp.z, gg.z, mm.z, vv.z, ee.z, (mk & 0x00ff0000u) ? 1.f : f)
    OPT_ADAMW1(pp.w, gg.w, mm.w, vv.w, ee.w, (mk & 0xff000000u) ? 1.f : f)
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<float4*>(e)[i] = ee;
  }
  // tail (n not a multiple of 4): the first block's first n % 4 threads, one byte of the mask each
  const long long r = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) {
    float p1 = p[r], m1 = m[r], v1 = v[r], e1 = 0.f;
    if constexpr (EMA) e1 = e[r];
    bool ex = false;
    if constexpr (MASK) ex = exempt[r] != 0;
    OPT_ADAMW1(p1, g[r], m1, v1, e1, ex ? 1.f : f)
    p[r] = p1;
    m[r] = m1;
    v[r] = v1;
    if constexpr (EMA) e[r] = e1;
  }
}

// behind the update kernel of one segment: advance its device-side step counter, or -- skipped step -- count it once (count_skip:
// only the first segment's call of an optimizer step counts, so one skipped step is one count in skip[1])
__global__ void opt_commit_kernel(int* __restrict__ step_dev, int* __restrict__ skip, int count_skip) {
  if (skip && skip[0]) {
    if (count_skip) skip[1] += 1;
    return;
  }
  step_dev[0] += 1;
}

template <bool CLIP, bool EMA>
static void adamw_launch(bool mask, int blocks, hipStream_t s, float* p, const float* g, float* m, float* v, long long n, float lr, float b1,
                         float b2, float eps, float wd, const int* skip, const int* step_dev, const float* lr_dev, const float* clip_dev,
                         const unsigned char* exempt, float* ema, double ema_decay) {
  if (mask)
    hipLaunchKernelGGL((adamw_kernel<CLIP, EMA, true>), dim3(blocks), dim3(POPT_THREADS), 0, s, p, g, m, v, n, lr, b1, b2, eps, wd, skip,
                       step_dev, lr_dev, clip_dev, exempt, ema, ema_decay);
  else
    hipLaunchKernelGGL((adamw_kernel<CLIP, EMA, false>), dim3(blocks), dim3(POPT_THREADS), 0, s, p, g, m, v, n, lr, b1, b2, eps, wd, skip,
                       step_dev, lr_dev, clip_dev, exempt, ema, ema_decay);
}

static int adamw_step_impl(const char* who, float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev,
                           float beta1, float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                           const unsigned char* exempt, const float* clip_dev, float* ema, double ema_decay, void* stream) {
  OPT_CHECK_ARG(p && g && m && v && step_dev, "%s: null pointer (p, g, m, v and step_dev are required)", who);
  OPT_CHECK_ARG(n > 0, "%s: need n >= 1, got %lld", who, n);
  OPT_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                "%s: slabs must be 16-byte aligned", who);
  OPT_CHECK_ARG(((uintptr_t)exempt & 3) == 0, "%s: exempt must be 4-byte aligned (one word of it is read per 16-byte lane)", who);
  OPT_CHECK_ARG((((uintptr_t)step_dev | (uintptr_t)skip | (uintptr_t)lr_dev | (uintptr_t)clip_dev) & 3) == 0,
                "%s: step_dev, skip, lr_dev and clip_dev must be 4-byte aligned", who);
  OPT_CHECK_ARG(lr >= 0.f && isfinite(lr), "%s: lr must be finite and >= 0, got %g", who, (double)lr);
  OPT_CHECK_ARG(eps >= 0.f && isfinite(eps), "%s: eps must be finite and >= 0, got %g", who, (double)eps);
  OPT_CHECK_ARG(weight_decay >= 0.f && isfinite(weight_decay), "%s: weight_decay must be finite and >= 0, got %g", who,
                (double)weight_decay);
  OPT_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: betas must lie in [0, 1), got (%g, %g)", who,
                (double)beta1, (double)beta2);
  if (ema) OPT_CHECK_ARG(ema_decay > 0.0 && ema_decay < 1.0, "%s: ema_decay must lie in (0, 1), got %g", who, ema_decay);
  hipStream_t s = (hipStream_t)stream;
  long long want = (n / 4 + 1 + POPT_THREADS - 1) / POPT_THREADS;
  const int blocks = (int)(want > POPT_MAX_BLOCKS ? POPT_MAX_BLOCKS : want);
  const bool mask = exempt != nullptr;
  if (ema && clip_dev)
    adamw_launch<true, true>(mask, blocks, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, skip, step_dev, lr_dev, clip_dev, exempt,
                             ema, ema_decay);
  else if (ema)
    adamw_launch<false, true>(mask, blocks, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, skip, step_dev, lr_dev, clip_dev, exempt,
                              ema, ema_decay);
  else if (clip_dev)
    adamw_launch<true, false>(mask, blocks, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, skip, step_dev, lr_dev, clip_dev, exempt,
                              ema, ema_decay);
  else
    adamw_launch<false, false>(mask, blocks, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, skip, step_dev, lr_dev, clip_dev,
                               exempt, ema, ema_decay);
  hipLaunchKernelGGL(opt_commit_kernel, dim3(1), dim3(1), 0, s, step_dev, skip, count_skip);
  return opt_launched(who);
}

extern "C" int popt_version(void) { return POPT_VERSION; }
extern "C" const char* popt_last_error(void) { return g_opt_err; }
extern "C" long long popt_trip_elements(void) { return 4LL * POPT_THREADS * POPT_MAX_BLOCKS; }

extern "C" int popt_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                               float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                               const unsigned char* exempt, void* stream) {
  return adamw_step_impl("popt_adamw_step", p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step_dev, skip, count_skip, exempt,
                         nullptr, nullptr, 0.0, stream);
}

extern "C" int popt_adamw_step_clip(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                                    float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                                    const unsigned char* exempt, const float* clip_dev, void* stream) {
  OPT_CHECK_ARG(clip_dev, "popt_adamw_step_clip: null pointer (clip_dev is required)");
  return adamw_step_impl("popt_adamw_step_clip", p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step_dev, skip, count_skip,
                         exempt, clip_dev, nullptr, 0.0, stream);
}

extern "C" int popt_adamw_step_ema(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                                   float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                                   const unsigned char* exempt, float* ema, double ema_decay, const float* clip_dev, void* stream) {
  OPT_CHECK_ARG(ema, "popt_adamw_step_ema: null pointer (ema is required)");
  return adamw_step_impl("popt_adamw_step_ema", p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step_dev, skip, count_skip,
                         exempt, clip_dev, ema, ema_decay, stream);
}
