// Fused Adam over one flat fp32 parameter slab (torch.optim.Adam(lr, betas=(.9,.999), eps=1e-8,
// weight_decay=wd) semantics: L2-coupled decay, bias correction as PyTorch) -- train_chaos.py:219,315.
// HBM-bound: 16 B per lane, reads p,g,m,v and writes p,m,v once (28 B / parameter).
#include "pp_common.h"

// gc = fl32(g * coef): the gradient-norm clip of FusedAdam / FusedSGD.  The product is ROUNDED before anything else uses it --
// `gc + wd * p` must stay the existing fma(wd, p, g') on g' = gc, exactly what the unclipped kernel computes on a slab that
// torch.nn.utils.clip_grad_norm_ had scaled in place; contracted into fma(g, coef, wd * p) it would round differently.
__device__ __forceinline__ float pp_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// EMA of the weights (FusedAdam / FusedSGD ema_decay): e <- e + fl32(w * fl32(p - e)), three separately rounded fp32 operations --
// the torch fp32 chain e + w * (p - e), bit for bit; contracted into fma(w, p - e, e) it would round differently.
__device__ __forceinline__ float pp_ema_rounded(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = w * d;
  return e + s;
}

// w = fl32(1 - d_t), d_t = min(D, (1 + t) / (10 + t)) in double: t = updates applied to the segment so far (0 for the first one);
// the warm-up keeps a short run from averaging mostly its initial weights.  Rounded once.
__device__ __forceinline__ float pp_ema_weight(double decay, double t) {
  const double warm = (1.0 + t) / (10.0 + t);
  return (float)(1.0 - (decay < warm ? decay : warm));
}

__device__ __forceinline__ float* pp_ema_slab(float* e, double) { return e; }
__device__ __forceinline__ double pp_ema_decay(float*, double decay) { return decay; }

// CLIP = false is the kernel as it always was (clip_dev is not read); CLIP = true scales every gradient element by the device
// scalar clip_dev[0] first (the coefficient grad_clip_finalize_kernel writes).
// EMA = false reads neither of E...; EMA = true (E... = float* e, double decay; needs step_dev) also loads the shadow slab e up
// front with p, g, m, v, moves it towards the p held in registers and stores it: 8 B / parameter on top of the 28, instead of the
// 12 B / parameter and the launch of a pass of its own.  A skipped step returns before any of it.
template <bool CLIP, bool EMA, typename... E>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n,
                                                   float lr, float b1, float b2, float eps, float wd, float bc1,
                                                   float sqrt_bc2, int* __restrict__ skip, const int* __restrict__ step_dev,
                                                   const float* __restrict__ lr_dev, const float* __restrict__ clip_dev,
                                                   E... ema_args) {
  static_assert(sizeof...(E) == (EMA ? 2 : 0), "adam_kernel: EMA takes (float* e, double decay)");
  // skip (nullable): skip[0] != 0 -> the gradients of this step are not finite (16-bit storage: loss-scale overflow, found by
  // pp_scale_guard): leave p, m, v untouched.  The skipped update is counted in skip[1] by the caller's form: the *_guard entry
  // points count here (once per launch), the *_dev entry points in their commit kernel (once per optimizer step).
  if (skip && skip[0]) {
    if (!step_dev && blockIdx.x == 0 && threadIdx.x == 0) skip[1] += 1;
    return;
  }
  // step_dev (nullable): number of updates applied to this segment so far, kept ON THE DEVICE -- the bias corrections follow the
  // updates that really happened (a skipped step does not advance them) and a captured hipGraph replays with the live count;
  // lr_dev (nullable): the learning rate as a device scalar, for the same reason
  if (step_dev) {
    const double t = (double)(step_dev[0] + 1);
    bc1 = (float)(1.0 - pow((double)b1, t));
    sqrt_bc2 = (float)sqrt(1.0 - pow((double)b2, t));
  }
  if (lr_dev) lr = lr_dev[0];
  const float coef = CLIP ? clip_dev[0] : 1.f;
  float* __restrict__ e = nullptr;
  float ew = 0.f;
  if constexpr (EMA) {
    e = pp_ema_slab(ema_args...);
    ew = pp_ema_weight(pp_ema_decay(ema_args...), (double)step_dev[0]);
  }
  const long long n4 = n >> 2;
  const float step = lr / bc1;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee;
    if constexpr (EMA) ee = reinterpret_cast<float4*>(e)[i];
#define PP_ADAM1(f)                                              \
    {                                                            \
      const float gc = CLIP ? pp_mul_rounded(gg.f, coef) : gg.f; \
      const float gr = gc + wd * pp.f;                           \
      mm.f = b1 * mm.f + (1.f - b1) * gr;                        \
      vv.f = b2 * vv.f + (1.f - b2) * gr * gr;                   \
      pp.f -= step * (mm.f / (sqrtf(vv.f) / sqrt_bc2 + eps));    \
      if constexpr (EMA) ee.f = pp_ema_rounded(ee.f, pp.f, ew);  \
    }
    PP_ADAM1(x) PP_ADAM1(y) PP_ADAM1(z) PP_ADAM1(w)
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<float4*>(e)[i] = ee;
  }
  // tail (n not a multiple of 4)
  const long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const float gc = CLIP ? pp_mul_rounded(g[t], coef) : g[t];
    const float gr = gc + wd * p[t];
    const float m1 = b1 * m[t] + (1.f - b1) * gr;
    const float v1 = b2 * v[t] + (1.f - b2) * gr * gr;
    m[t] = m1; v[t] = v1;
    if constexpr (EMA) {
      const float p1 = p[t] - step * (m1 / (sqrtf(v1) / sqrt_bc2 + eps));
      p[t] = p1;
      e[t] = pp_ema_rounded(e[t], p1, ew);
    } else {
      p[t] -= step * (m1 / (sqrtf(v1) / sqrt_bc2 + eps));
    }
  }
}

// after the update kernel(s) of one optimizer step: advance the device-side step counter of a segment, or -- skipped step --
// count it once (count_skip: only the first segment's commit counts, so one skipped step is one count)
__global__ void optim_commit_kernel(int* __restrict__ step_dev, int* __restrict__ skip, int count_skip) {
  if (skip && skip[0]) {
    if (count_skip) skip[1] += 1;
    return;
  }
  step_dev[0] += 1;
}

static int adam_step_impl(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int step, int* skip, void* stream,
                          int* step_dev = nullptr, const float* lr_dev = nullptr, int count_skip = 0,
                          const float* clip_dev = nullptr, float* ema = nullptr, double ema_decay = 0.0) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(p && g && m && v && n > 0 && (step >= 1 || step_dev), "adam_step: bad arguments");
  PP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0, "adam_step: slabs must be 16-byte aligned");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  int blocks = pp_cdiv(n / 4 + 1, 256);
  if (blocks > 4096) blocks = 4096;
  pp_prof_begin(PP_K_OPTIM, 0.0, (ema ? 36.0 : 28.0) * (double)n, s);
  if (ema && clip_dev)
    hipLaunchKernelGGL((adam_kernel<true, true, float*, double>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)sqrt(bc2), skip, (const int*)step_dev, lr_dev, clip_dev, ema, ema_decay);
  else if (ema)
    hipLaunchKernelGGL((adam_kernel<false, true, float*, double>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)sqrt(bc2), skip, (const int*)step_dev, lr_dev, clip_dev, ema, ema_decay);
  else if (clip_dev)
    hipLaunchKernelGGL((adam_kernel<true, false>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                       (float)bc1, (float)sqrt(bc2), skip, (const int*)step_dev, lr_dev, clip_dev);
  else
    hipLaunchKernelGGL((adam_kernel<false, false>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                       (float)bc1, (float)sqrt(bc2), skip, (const int*)step_dev, lr_dev, clip_dev);
  if (step_dev) hipLaunchKernelGGL(optim_commit_kernel, dim3(1), dim3(1), 0, s, step_dev, skip, count_skip);
  pp_prof_end(s);
  return pp_launch_status("adam_step");
}

extern "C" int pp_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int step, void* stream) {
  return adam_step_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, nullptr, stream);
}
// the same, skipped (and counted in skip[1]) when skip[0] != 0: see pp_scale_guard
extern "C" int pp_adam_step_guard(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int step, int* skip, void* stream) {
  return adam_step_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, skip, stream);
}

// The form the fused optimizers use (round 5): the step count of the segment lives on the device (step_dev[0] =
// updates applied so far; the kernel uses step_dev[0] + 1 for the bias corrections and a one-thread commit kernel advances it
// afterwards unless the step was skipped), lr_dev (nullable) overrides lr with a device scalar, skip as in pp_adam_step_guard
// except that a skipped STEP is counted once: only the call with count_skip != 0 adds to skip[1].
extern "C" int pp_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                                float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip, void* stream) {
  PP_CHECK_ARG(step_dev, "adam_step_dev: step_dev is null");
  return adam_step_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 1, skip, stream, step_dev, lr_dev, count_skip);
}
// pp_adam_step_dev on gradients scaled by the clip coefficient clip_dev[0] (out2 + 1 of pp_grad_clip_finalize): every
// element is first rounded to fl32(g * coef), the rest is the arithmetic above.  The gradient slab itself is not written.
extern "C" int pp_adam_step_clip(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                                 float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                                 const float* clip_dev, void* stream) {
  PP_CHECK_ARG(step_dev && clip_dev, "adam_step_clip: step_dev or clip_dev is null");
  return adam_step_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 1, skip, stream, step_dev, lr_dev, count_skip, clip_dev);
}
// pp_adam_step_dev (clip_dev null) or pp_adam_step_clip (clip_dev set) that also keeps the exponential moving average `ema` of p
// (fp32, laid out as p): in the same kernel, for the p it has just computed, ema <- ema + fl32(w * fl32(p - ema)) with
// w = fl32(1 - min(ema_decay, (1 + t) / (10 + t))), t = step_dev[0] before this update.  A skipped step leaves ema alone.
extern "C" int pp_adam_step_ema(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                                float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip, float* ema,
                                double ema_decay, const float* clip_dev, void* stream) {
  PP_CHECK_ARG(step_dev && ema, "adam_step_ema: step_dev or ema is null");
  PP_CHECK_ARG(ema_decay > 0.0 && ema_decay < 1.0, "adam_step_ema: ema_decay must lie in (0, 1)");
  return adam_step_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 1, skip, stream, step_dev, lr_dev, count_skip, clip_dev,
                        ema, ema_decay);
}

// torch.optim.SGD(lr, momentum, weight_decay) (train_chaos.py:220-221, --optimizer momentum): g += wd*p;
// buf = g on the first step, momentum*buf + g afterwards (dampening 0, no Nesterov); p -= lr*buf.  20 B / parameter.
template <bool CLIP, bool EMA, typename... E>
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ buf, long long n, float lr, float mom,
                                                           float wd, int first, int* __restrict__ skip,
                                                           const int* __restrict__ step_dev, const float* __restrict__ lr_dev,
                                                           const float* __restrict__ clip_dev, E... ema_args) {
  static_assert(sizeof...(E) == (EMA ? 2 : 0), "sgd_momentum_kernel: EMA takes (float* e, double decay)");
  if (skip && skip[0]) {                      // non-finite gradients this step (see adam_kernel)
    if (!step_dev && blockIdx.x == 0 && threadIdx.x == 0) skip[1] += 1;
    return;
  }
  if (step_dev) first = step_dev[0] == 0;
  if (lr_dev) lr = lr_dev[0];
  const float coef = CLIP ? clip_dev[0] : 1.f;          // see adam_kernel
  float* __restrict__ e = nullptr;                      // EMA: see adam_kernel
  float ew = 0.f;
  if constexpr (EMA) {
    e = pp_ema_slab(ema_args...);
    ew = pp_ema_weight(pp_ema_decay(ema_args...), (double)step_dev[0]);
  }
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 bb = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<float4*>(buf)[i];
    float4 ee;
    if constexpr (EMA) ee = reinterpret_cast<float4*>(e)[i];
#define PP_SGD1(f)                                   \
    {                                                \
      const float gc = CLIP ? pp_mul_rounded(gg.f, coef) : gg.f; \
      const float gr = gc + wd * pp.f;               \
      bb.f = first ? gr : mom * bb.f + gr;           \
      pp.f -= lr * bb.f;                             \
      if constexpr (EMA) ee.f = pp_ema_rounded(ee.f, pp.f, ew);  \
    }
    PP_SGD1(x) PP_SGD1(y) PP_SGD1(z) PP_SGD1(w)
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(buf)[i] = bb;
    if constexpr (EMA) reinterpret_cast<float4*>(e)[i] = ee;
  }
  const long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const float gc = CLIP ? pp_mul_rounded(g[t], coef) : g[t];
    const float gr = gc + wd * p[t];
    const float b1 = first ? gr : mom * buf[t] + gr;
    buf[t] = b1;
    if constexpr (EMA) {
      const float p1 = p[t] - lr * b1;
      p[t] = p1;
      e[t] = pp_ema_rounded(e[t], p1, ew);
    } else {
      p[t] -= lr * b1;
    }
  }
}

static int sgd_step_impl(float* p, const float* g, float* buf, long long n, float lr, float momentum,
                         float weight_decay, int step, int* skip, void* stream, int* step_dev = nullptr,
                         const float* lr_dev = nullptr, int count_skip = 0, const float* clip_dev = nullptr,
                         float* ema = nullptr, double ema_decay = 0.0) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(p && g && buf && n > 0 && (step >= 1 || step_dev), "sgd_momentum_step: bad arguments");
  PP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf | (uintptr_t)ema) & 15) == 0, "sgd_momentum_step: slabs must be 16-byte aligned");
  int blocks = pp_cdiv(n / 4 + 1, 256);
  if (blocks > 4096) blocks = 4096;
  pp_prof_begin(PP_K_OPTIM, 0.0, (ema ? 28.0 : 20.0) * (double)n, s);
  if (ema && clip_dev)
    hipLaunchKernelGGL((sgd_momentum_kernel<true, true, float*, double>), dim3(blocks), dim3(256), 0, s, p, g, buf, n, lr, momentum,
                       weight_decay, 0, skip, (const int*)step_dev, lr_dev, clip_dev, ema, ema_decay);
  else if (ema)
    hipLaunchKernelGGL((sgd_momentum_kernel<false, true, float*, double>), dim3(blocks), dim3(256), 0, s, p, g, buf, n, lr, momentum,
                       weight_decay, 0, skip, (const int*)step_dev, lr_dev, clip_dev, ema, ema_decay);
  else if (clip_dev)
    hipLaunchKernelGGL((sgd_momentum_kernel<true, false>), dim3(blocks), dim3(256), 0, s, p, g, buf, n, lr, momentum, weight_decay,
                       step == 1 ? 1 : 0, skip, (const int*)step_dev, lr_dev, clip_dev);
  else
    hipLaunchKernelGGL((sgd_momentum_kernel<false, false>), dim3(blocks), dim3(256), 0, s, p, g, buf, n, lr, momentum, weight_decay,
                       step == 1 ? 1 : 0, skip, (const int*)step_dev, lr_dev, clip_dev);
  if (step_dev) hipLaunchKernelGGL(optim_commit_kernel, dim3(1), dim3(1), 0, s, step_dev, skip, count_skip);
  pp_prof_end(s);
  return pp_launch_status("sgd_momentum_step");
}

extern "C" int pp_sgd_momentum_step(float* p, const float* g, float* buf, long long n, float lr, float momentum,
                                    float weight_decay, int step, void* stream) {
  return sgd_step_impl(p, g, buf, n, lr, momentum, weight_decay, step, nullptr, stream);
}
extern "C" int pp_sgd_momentum_step_guard(float* p, const float* g, float* buf, long long n, float lr, float momentum,
                                          float weight_decay, int step, int* skip, void* stream) {
  return sgd_step_impl(p, g, buf, n, lr, momentum, weight_decay, step, skip, stream);
}

extern "C" int pp_sgd_momentum_step_dev(float* p, const float* g, float* buf, long long n, float lr, const float* lr_dev,
                                        float momentum, float weight_decay, int* step_dev, int* skip, int count_skip, void* stream) {
  PP_CHECK_ARG(step_dev, "sgd_momentum_step_dev: step_dev is null");
  return sgd_step_impl(p, g, buf, n, lr, momentum, weight_decay, 2, skip, stream, step_dev, lr_dev, count_skip);
}
extern "C" int pp_sgd_momentum_step_clip(float* p, const float* g, float* buf, long long n, float lr, const float* lr_dev,
                                         float momentum, float weight_decay, int* step_dev, int* skip, int count_skip,
                                         const float* clip_dev, void* stream) {
  PP_CHECK_ARG(step_dev && clip_dev, "sgd_momentum_step_clip: step_dev or clip_dev is null");
  return sgd_step_impl(p, g, buf, n, lr, momentum, weight_decay, 2, skip, stream, step_dev, lr_dev, count_skip, clip_dev);
}
// pp_sgd_momentum_step_dev / _clip (clip_dev null / set) that also keeps the moving average `ema` of p: see pp_adam_step_ema
extern "C" int pp_sgd_momentum_step_ema(float* p, const float* g, float* buf, long long n, float lr, const float* lr_dev,
                                        float momentum, float weight_decay, int* step_dev, int* skip, int count_skip, float* ema,
                                        double ema_decay, const float* clip_dev, void* stream) {
  PP_CHECK_ARG(step_dev && ema, "sgd_momentum_step_ema: step_dev or ema is null");
  PP_CHECK_ARG(ema_decay > 0.0 && ema_decay < 1.0, "sgd_momentum_step_ema: ema_decay must lie in (0, 1)");
  return sgd_step_impl(p, g, buf, n, lr, momentum, weight_decay, 2, skip, stream, step_dev, lr_dev, count_skip, clip_dev, ema,
                       ema_decay);
}

// The unfused form of the moving average over e[0..n): e <- e + fl32(w * fl32(p - e)), w as in adam_kernel from t = step_dev[0]
// (step_dev set) or t = t_host.  12 B / parameter.  What the fused kernels are tested against; p is not written.
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ e, long long n, double decay,
                                                         const int* __restrict__ step_dev, long long t_host) {
  const float ew = pp_ema_weight(decay, step_dev ? (double)step_dev[0] : (double)t_host);
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 pp = reinterpret_cast<const float4*>(p)[i];
    float4 ee = reinterpret_cast<float4*>(e)[i];
    ee.x = pp_ema_rounded(ee.x, pp.x, ew);
    ee.y = pp_ema_rounded(ee.y, pp.y, ew);
    ee.z = pp_ema_rounded(ee.z, pp.z, ew);
    ee.w = pp_ema_rounded(ee.w, pp.w, ew);
    reinterpret_cast<float4*>(e)[i] = ee;
  }
  const long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) e[t] = pp_ema_rounded(e[t], p[t], ew);
}

extern "C" int pp_ema_update(const float* p, float* e, long long n, double ema_decay, const int* step_dev, long long t_host,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(p && e && n > 0 && (step_dev || t_host >= 0), "ema_update: bad arguments");
  PP_CHECK_ARG(ema_decay > 0.0 && ema_decay < 1.0, "ema_update: ema_decay must lie in (0, 1)");
  PP_CHECK_ARG((((uintptr_t)p | (uintptr_t)e) & 15) == 0, "ema_update: slabs must be 16-byte aligned");
  int blocks = pp_cdiv(n / 4 + 1, 256);
  if (blocks > 4096) blocks = 4096;
  pp_prof_begin(PP_K_OPTIM, 0.0, 12.0 * (double)n, s);
  hipLaunchKernelGGL(ema_update_kernel, dim3(blocks), dim3(256), 0, s, p, e, n, ema_decay, step_dev, t_host);
  pp_prof_end(s);
  return pp_launch_status("ema_update");
}

// a[0..n) <-> b[0..n) in place: every element is read into registers and written to the other slab by the same thread, no
// temporary.  16 B / parameter.  (optimizer.ema_weights(): evaluate the averaged weights where the live ones were.)
__global__ __launch_bounds__(256) void slab_swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<float4*>(a)[i];
    const float4 y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y;
    reinterpret_cast<float4*>(b)[i] = x;
  }
  const long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const float x = a[t], y = b[t];
    a[t] = y;
    b[t] = x;
  }
}

extern "C" int pp_slab_swap(float* a, float* b, long long n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(a && b && n > 0, "slab_swap: bad arguments");
  PP_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "slab_swap: slabs must be 16-byte aligned");
  PP_CHECK_ARG(a + n <= b || b + n <= a, "slab_swap: the ranges overlap");
  int blocks = pp_cdiv(n / 4 + 1, 256);
  if (blocks > 4096) blocks = 4096;
  pp_prof_begin(PP_K_OPTIM, 0.0, 16.0 * (double)n, s);
  hipLaunchKernelGGL(slab_swap_kernel, dim3(blocks), dim3(256), 0, s, a, b, n);
  pp_prof_end(s);
  return pp_launch_status("slab_swap");
}

// ---- global gradient-norm clipping (torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) semantics) ----
// Sum of squares of one slab segment, 4 B per parameter read once.  Every element is converted to double BEFORE it is squared
// and added, so the only fp32 rounding of the norm is the final conversion.  No floating-point atomics: the grid is a pure
// function of n (pp_grad_sumsq_rows), every block writes ONE double to its own row and grad_clip_finalize_kernel adds the rows
// in a fixed order -- the norm of a slab is the same bits in every run, eager or replayed from a hipGraph.
#define PP_SUMSQ_UNROLL 4          // independent 16-byte loads in flight per thread before the first use
#define PP_SUMSQ_MAX_ROWS 1024     // 4 blocks of 256 threads per CU
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ partial) {
  __shared__ double sh[4];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double acc[PP_SUMSQ_UNROLL];
#pragma unroll
  for (int u = 0; u < PP_SUMSQ_UNROLL; ++u) acc[u] = 0.0;
#define PP_SUMSQ4(a, q)                                                                        \
  {                                                                                            \
    const double x = (double)(q).x, y = (double)(q).y, z = (double)(q).z, w = (double)(q).w;   \
    a = fma(x, x, a); a = fma(y, y, a); a = fma(z, z, a); a = fma(w, w, a);                    \
  }
  for (; i + (PP_SUMSQ_UNROLL - 1) * stride < n4; i += PP_SUMSQ_UNROLL * stride) {
    float4 q[PP_SUMSQ_UNROLL];
#pragma unroll
    for (int u = 0; u < PP_SUMSQ_UNROLL; ++u) q[u] = g4[i + u * stride];
#pragma unroll
    for (int u = 0; u < PP_SUMSQ_UNROLL; ++u) PP_SUMSQ4(acc[u], q[u])
  }
  for (; i < n4; i += stride) {
    const float4 q = g4[i];
    PP_SUMSQ4(acc[0], q)
  }
  // tail (n not a multiple of 4): the first block's first n % 4 threads
  const long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const double x = (double)g[t];
    acc[1] = fma(x, x, acc[1]);
  }
  double a = pp_wave_sum_d((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int pp_grad_sumsq_rows(long long n) {
  if (n <= 0) return 0;
  const long long want = ((n >> 2) + 1 + 256 * PP_SUMSQ_UNROLL - 1) / (256 * PP_SUMSQ_UNROLL);
  return (int)(want > PP_SUMSQ_MAX_ROWS ? PP_SUMSQ_MAX_ROWS : want);
}

extern "C" int pp_grad_sumsq(const float* g, long long n, double* partial, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(g && partial && n > 0, "grad_sumsq: bad arguments");
  PP_CHECK_ARG(((uintptr_t)g & 15) == 0 && ((uintptr_t)partial & 7) == 0, "grad_sumsq: g must be 16-byte aligned, partial 8-byte aligned");
  pp_prof_begin(PP_K_OPTIM, 2.0 * (double)n, 4.0 * (double)n, s);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(pp_grad_sumsq_rows(n)), dim3(256), 0, s, g, n, partial);
  pp_prof_end(s);
  return pp_launch_status("grad_sumsq");
}

// One block per optimizer step: total = sqrt(sum of all rows), coef = min(1, max_norm / (total + 1e-6)) -- torch's
// clip_coef_clamped -- both formed in double and rounded once.  out2 = [total, coef]; stats = double[4]: optimizer steps seen,
// steps with coef < 1, sum of total, max of total.  A step the overflow guard is going to skip (skip[0] != 0) leaves the
// statistics alone (its norm is not finite).
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ partial, int rows, double max_norm,
                                                                 const int* __restrict__ skip, float* __restrict__ out2,
                                                                 double* __restrict__ stats) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) a += partial[r];      // fixed order per thread, fixed butterfly, fixed wave order
  a = pp_wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double total = sqrt((sh[0] + sh[1]) + (sh[2] + sh[3]));
  const double c = max_norm / (total + 1e-6);
  const float coef = c < 1.0 ? (float)c : 1.f;
  out2[0] = (float)total;
  out2[1] = coef;
  if (skip && skip[0]) return;
  stats[0] += 1.0;
  if (coef < 1.f) stats[1] += 1.0;
  stats[2] += total;
  if (total > stats[3]) stats[3] = total;
}

extern "C" int pp_grad_clip_finalize(const double* partial, int rows, double max_norm, const int* skip, float* out2, double* stats,
                                     void* stream) {
  PP_CHECK_ARG(partial && out2 && stats && rows > 0, "grad_clip_finalize: bad arguments");
  PP_CHECK_ARG(max_norm > 0.0, "grad_clip_finalize: max_norm must be positive (+inf: measure only)");
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, rows, max_norm, skip, out2, stats);
  return pp_launch_status("grad_clip_finalize");
}

// dst (+)= src over a flat slab (gradient accumulation across bucket copies, test helper)
__global__ void fill_kernel(float* __restrict__ p, long long n, float value) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = value;
}

extern "C" int pp_fill(float* p, long long n, float value, void* stream) {
  PP_CHECK_ARG(p && n >= 0, "fill: bad arguments");
  if (n == 0) return 0;
  int blocks = pp_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, n, value);
  return pp_launch_status("fill");
}

// p *= value over a flat slab: removes the static loss scale from the gradient slab of a 16-bit-storage step (the scale is a
// power of two: exact) before the optimizer / after the all-reduce
__global__ void scale_kernel(float* __restrict__ p, long long n, float value, int* __restrict__ bad) {
  bool nf = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = p[i] * value;
    p[i] = v;
    nf |= !(fabsf(v) <= 3.4028234e38f);       // inf or NaN
  }
  if (bad && nf) atomicOr(bad, 1);            // rare; order independent
}

extern "C" int pp_scale(float* p, long long n, float value, void* stream) {
  PP_CHECK_ARG(p && n >= 0, "scale: bad arguments");
  if (n == 0) return 0;
  int blocks = pp_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, n, value, (int*)nullptr);
  return pp_launch_status("scale");
}

// the same, and bad[0] |= 1 when a scaled value is not finite: the overflow check of the 16-bit storage mode (a static loss
// scale can overflow fp16 in a bad step; pp_adam_step_guard / pp_sgd_momentum_step_guard then leave the weights alone)
extern "C" int pp_scale_guard(float* p, long long n, float value, int* bad, void* stream) {
  PP_CHECK_ARG(p && bad && n >= 0, "scale_guard: bad arguments");
  if (n == 0) return 0;
  int blocks = pp_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, n, value, bad);
  return pp_launch_status("scale_guard");
}
