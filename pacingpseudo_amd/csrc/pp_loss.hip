// Loss-side kernels of the PacingPseudo step (all HBM/latency-bound, NCHW logits with K <= 32 classes):
//   * channel arg-max (scribble one-hot -> int64 target, prediction masks)  consistency_reglur_memory.py:31
//   * fused partial-CE + entropy-minimisation + decoder-consistency sums     losses/losses.py:9-116
//   * their gradient wrt the weak and strong logits
//   * auxiliary head: bilinear x(H/h) up-sampling of the low-res logits fused with partial-CE, and the
//     gather-form gradient back to the low-res logits                        aux_path_memory.py:52, losses.py:43
//   * class-prototype memory bank update (batch sample 0 only) and the bank classification CE
//                                                                            aux_path_memory.py:61,68-116
//   * validation Dice counts                                                 utils/metrics.py:7-34
// Reductions are two-stage (per-block partials, fixed-order double finalize): deterministic, no float atomics.
// The per-pixel kernels are templates on the class bound MK (pp_by_class_bound, pp_common.h): K <= 8 runs the MK = LS_MAXK
// instantiations (and the four-pixel v4 forms for K in {2, 4, 5}), 9 <= K <= 16 and 17 <= K <= 32 the MK = 16 and 32 ones.
#include "pp_common.h"

#define LS_THREADS 256
#define LS_MAXK PP_MAXK_SMALL    // class bound of the K <= 8 kernels; the wide instantiations go to PP_MAXK

// ---------------------------------------------------------------- arg-max over channels (first maximum wins)
__global__ void argmax_channels_kernel(const float* __restrict__ x, int N, int C, int HW, long long* __restrict__ out) {
  const long long P = (long long)N * HW;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    // (32-bit division where the pixel index fits: the 64-bit form is ~150 VALU instructions of these kernels' ~870 per pixel)
    const int n = p < 0x7fffffffLL ? (int)((unsigned)p / (unsigned)HW) : (int)(p / HW), hw = (int)(p - (long long)n * HW);
    const float* b = x + (size_t)n * C * HW + hw;
    float m = b[0];
    int k = 0;
    for (int c = 1; c < C; ++c) {
      const float v = b[(size_t)c * HW];
      if (v > m) { m = v; k = c; }
    }
    out[p] = k;
  }
}

static inline int ls_blocks(long long total, int cap = 4096) {
  int b = pp_cdiv(total, LS_THREADS);
  return b > cap ? cap : (b < 1 ? 1 : b);
}

extern "C" int pp_argmax_channels(const float* x, int N, int C, int HW, int64_t* out, void* stream) {
  PP_CHECK_ARG(x && out && N > 0 && C > 0 && HW > 0, "argmax_channels: bad arguments");
  hipLaunchKernelGGL(argmax_channels_kernel, dim3(ls_blocks((long long)N * HW)), dim3(LS_THREADS), 0,
                     (hipStream_t)stream, x, N, C, HW, (long long*)out);
  return pp_launch_status("argmax_channels");
}

// ---------------------------------------------------------------- softmax helpers
template <int MK>
struct SM { float p[MK]; float l[MK]; };             // softmax and log-softmax of one pixel
// softmax / log-softmax of one pixel from its K logits (the one expression every loss kernel uses: the scalar and the
// four-pixels-per-thread forms of a kernel give the same bits)
template <int MK>
__device__ __forceinline__ void softmax_vals(const float (&v)[MK], int K, SM<MK>& o) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) m = fmaxf(m, v[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) { o.p[k] = expf(v[k] - m); s += o.p[k]; }
  const float ls = logf(s), inv = 1.f / s;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) { o.l[k] = v[k] - m - ls; o.p[k] *= inv; }
}
template <int MK>
__device__ __forceinline__ void pixel_softmax(const float* __restrict__ z, size_t stride, int K, SM<MK>& o) {
  float v[MK];
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) v[k] = z[(size_t)k * stride];
  softmax_vals(v, K, o);
}

// consistency variants (train_chaos.py:138): 0 none, 1 ce_loss, 2 l1_loss, 3 l2_loss, 4 kl_loss
template <int MK>
__device__ __forceinline__ float cr_value(const SM<MK>& w, const SM<MK>& s, int K, int variant) {
  float L = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      if (variant == 1) L -= w.p[k] * s.l[k];
      else if (variant == 2) L += fabsf(s.p[k] - w.p[k]);
      else if (variant == 3) { const float d = s.p[k] - w.p[k]; L += d * d; }
      else L += w.p[k] * (w.l[k] - s.l[k]);
    }
  return L;
}

// ... 5 bikl_loss, 6 js_loss, 7 hard_ce_loss (this implementation's additions to the CLI; bidirectional_kl_loss is
// losses/losses.py:118-145).  They read the weak / strong log-probability gap t_k = lq_k - ls_k, and where the two views nearly
// agree (late training) every term is a difference of nearly equal numbers: the rounding of lq_k and ls_k (~1e-7 each) would be
// 1e-4 of a gap of 1e-3.  Where every logit difference d_k = zw_k - zs_k of the pixel is at most 1/2, cr_gaps therefore takes
// t_k = d_k - C: d_k is exact to 3e-8 there, and the shift C = log-partition difference is read off the weak arg-max channel c*,
// where the log-probabilities are smallest.  An error of C is the same for every k and cancels to first order in the terms below
// (all but one: cr_gaps_recentre).  Elsewhere t_k = lq_k - ls_k as it stands: a d_k of two logits of magnitude 200 (spread 60) is
// rounded at 1e-5, a log-probability of a class that matters is not.  The two forms approximate the same number; which one a
// pixel takes changes nothing beyond rounding.
// c* = first maximum of the weak logits (the tie rule of argmax_channels_kernel); all t_k are finite for finite logits.
template <int MK>
__device__ __forceinline__ int cr_gaps(const float (&vw)[MK], const float (&vs)[MK], const SM<MK>& w, const SM<MK>& s, int K,
                                       float (&t)[MK]) {
  float mx = vw[0], dmax = 0.f;
  int cs = 0;
#pragma unroll
  for (int k = 1; k < MK; ++k)
    if (k < K && vw[k] > mx) { mx = vw[k]; cs = k; }
  float C = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    if (k == cs) C = (vw[k] - vs[k]) - (w.l[k] - s.l[k]);
    if (k < K) dmax = fmaxf(dmax, fabsf(vw[k] - vs[k]));
  }
  const bool close = dmax <= 0.5f;
#pragma unroll
  for (int k = 0; k < MK; ++k) t[k] = k < K ? (close ? (vw[k] - vs[k]) - C : w.l[k] - s.l[k]) : 0.f;
  return cs;
}
// q_k - s_k from the gap: s expm1(t) for t <= 0, -q expm1(-t) for t > 0.  expm1 of a non-positive number lies in (-1, 0], so
// a probability that underflowed to 0 gives 0 * finite = 0.
__device__ __forceinline__ float cr_pdiff(float q, float s, float t) {
  const float e = expm1f(-fabsf(t));
  return t <= 0.f ? s * e : -q * e;
}
// bikl_loss: (q_k - s_k) itself is first order in an error of C -- the one term here that is -- and sum_k (q_k - s_k) = 0 measures that
// error: with every t_k off by e the sum comes out as e (times sum_k min(q_k, s_k)-like weights, 1 where the views agree), so it is
// subtracted once.  Where the views disagree the sum is rounding noise of ~1e-7 against gaps of order 1.
template <int MK>
__device__ __forceinline__ void cr_gaps_recentre(const SM<MK>& w, const SM<MK>& s, int K, float (&t)[MK]) {
  float e = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) e += cr_pdiff(w.p[k], s.p[k], t[k]);
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) t[k] -= e;
}
// js_loss: lq - lm and ls - lm with lm = log((q + s) / 2) = max(lq, ls) + log((1 + exp(-|t|)) / 2), a log-add-exp of the two
// log-probabilities: h = log1p(expm1(-|t|) / 2) lies in [-ln 2, 0]; the larger of the two is -h, the smaller -|t| - h.
__device__ __forceinline__ void cr_js_gaps(float t, float& qm, float& sm) {
  const float at = fabsf(t), h = log1pf(0.5f * expm1f(-at));
  qm = t <= 0.f ? -at - h : -h;
  sm = t <= 0.f ? -h : -at - h;
}
template <int MK>
__device__ __forceinline__ float cr_value_gap(const float (&vw)[MK], const float (&vs)[MK], const SM<MK>& w, const SM<MK>& s,
                                              int K, int variant) {
  float t[MK];
  const int cs = cr_gaps(vw, vs, w, s, K, t);
  float L = 0.f;
  if (variant == 7) {                                           // -log s_{c*}
#pragma unroll
    for (int k = 0; k < MK; ++k) if (k == cs) L = -s.l[k];
    return L;
  }
  if (variant == 5) cr_gaps_recentre(w, s, K, t);
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      if (variant == 5) L += cr_pdiff(w.p[k], s.p[k], t[k]) * t[k];           // (q - s)(lq - ls)
      else {
        float qm, sm;
        cr_js_gaps(t[k], qm, sm);
        L += w.p[k] * qm + s.p[k] * sm;                                       // q (lq - lm) + s (ls - lm)
      }
    }
  return 0.5f * L;
}
// their gradients, f = g_cr * m / denominator, in closed form (no quotient of probabilities):
//   bikl  dz_s[k] = f/2 [(s_k - q_k) - s_k (t_k - sum_c s_c t_c)]     dz_w[k] = f/2 [(q_k - s_k) + q_k (t_k - sum_c q_c t_c)]
//   js    dz_s[k] = f/2 s_k ((ls - lm)_k - sum_c s_c (ls - lm)_c)      dz_w[k] likewise with q, lq
//   hard  dz_s[k] = f (s_k - [k == c*]), nothing to the weak logits
template <int MK>
__device__ __forceinline__ void cr_grad_gap(const float (&vw)[MK], const float (&vs)[MK], const SM<MK>& w, const SM<MK>& s,
                                            int K, int variant, bool weak_grad, float f, float (&dw)[MK], float (&ds)[MK]) {
  float t[MK];
  const int cs = cr_gaps(vw, vs, w, s, K, t);
  if (variant == 7) {
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) ds[k] = f * (s.p[k] - (k == cs ? 1.f : 0.f));
    return;
  }
  // s_k (x_k - sum_c s_c x_c) does not change when a constant is added to x, but its rounding does: in a confident pixel s_a -> 1,
  // x_a and the sum are the same number, and their difference -- of the size of the runner-up's probability -- is lost below
  // 1e-7 |x_a|.  So x is taken relative to its value at the arg-max a of the distribution it is weighted with (x_a = 0 exactly).
  int as = 0;
  {
    float mx = vs[0];
#pragma unroll
    for (int k = 1; k < MK; ++k)
      if (k < K && vs[k] > mx) { mx = vs[k]; as = k; }
  }
  const float hf = 0.5f * f;
  if (variant == 5) {
    cr_gaps_recentre(w, s, K, t);
    float tw = 0.f, ts = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k) { if (k == cs) tw = t[k]; if (k == as) ts = t[k]; }
    float qt = 0.f, st = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) { qt += w.p[k] * (t[k] - tw); st += s.p[k] * (t[k] - ts); }
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float d = cr_pdiff(w.p[k], s.p[k], t[k]);
        if (weak_grad) dw[k] += hf * (d + w.p[k] * ((t[k] - tw) - qt));
        ds[k] = -hf * (d + s.p[k] * ((t[k] - ts) - st));
      }
    return;
  }
  float qm0 = 0.f, sm0 = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    float qm, sm;
    if (k == cs) { cr_js_gaps(t[k], qm, sm); qm0 = qm; }
    if (k == as) { cr_js_gaps(t[k], qm, sm); sm0 = sm; }
  }
  float qa = 0.f, sa = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      float qm, sm;
      cr_js_gaps(t[k], qm, sm);
      qa += w.p[k] * (qm - qm0);
      sa += s.p[k] * (sm - sm0);
    }
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      float qm, sm;
      cr_js_gaps(t[k], qm, sm);
      if (weak_grad) dw[k] += hf * w.p[k] * ((qm - qm0) - qa);
      ds[k] = hf * s.p[k] * ((sm - sm0) - sa);
    }
}

// sums[0]=pce_sum [1]=n_labelled [2]=ent_sum [3]=ent_den [4]=cr_sum [5]=cr_den   (double)
struct SegAcc { float pce, n, ent, cr, m; };
// GAP: the instantiation for the variants >= 5 (host-side choice).  They are kept out of the kernels of the variants 0 - 4, whose
// code -- and register count: the t[] of cr_gaps costs 20 - 90 VGPRs and one to two waves of occupancy -- stays what it was.
template <int MK, bool GAP>
__device__ __forceinline__ void seg_fwd_pixel(const float (&vw)[MK], const float (&vs)[MK], long long t, float m, int K,
                                              int ignore_index, int do_ent, int variant, SegAcc& a) {
  SM<MK> w;
  softmax_vals(vw, K, w);
  if (t != ignore_index && t >= 0 && t < K) {
    float lt = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k) if (k == (int)t) lt = w.l[k];
    a.pce -= lt;
    a.n += 1.f;
  }
  a.m += m;
  if (do_ent) {
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k) if (k < K) h -= w.p[k] * w.l[k];
    a.ent += h * m;
  }
  if (variant) {
    SM<MK> s;
    softmax_vals(vs, K, s);
    if constexpr (GAP) a.cr += cr_value_gap(vw, vs, w, s, K, variant) * m;
    else a.cr += cr_value(w, s, K, variant) * m;
  }
}

__device__ __forceinline__ void seg_acc_store(const SegAcc& a, float* sh, double* __restrict__ partial) {
  const float r0 = pp_block_sum(a.pce, sh), r1 = pp_block_sum(a.n, sh), r2 = pp_block_sum(a.ent, sh);
  const float r3 = pp_block_sum(a.cr, sh), r4 = pp_block_sum(a.m, sh);
  if (threadIdx.x == 0) {
    double* o = partial + (size_t)blockIdx.x * 5;
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
  }
}

template <int MK, bool GAP>
__global__ __launch_bounds__(LS_THREADS) void seg_losses_partial_kernel(
    const float* __restrict__ zw, const float* __restrict__ zs, const long long* __restrict__ target,
    const float* __restrict__ mask, int N, int K, int HW, int ignore_index, int do_ent, int variant,
    double* __restrict__ partial /*[blocks][5]*/) {
  __shared__ float sh[16];
  const long long P = (long long)N * HW;
  SegAcc a{0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    // (32-bit division where the pixel index fits: the 64-bit form is ~150 VALU instructions of these kernels' ~870 per pixel)
    const int n = p < 0x7fffffffLL ? (int)((unsigned)p / (unsigned)HW) : (int)(p / HW), hw = (int)(p - (long long)n * HW);
    const size_t off = (size_t)n * K * HW + hw;
    float vw[MK], vs[MK];
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      vw[k] = k < K ? zw[off + (size_t)k * HW] : 0.f;
      vs[k] = (k < K && variant) ? zs[off + (size_t)k * HW] : 0.f;
    }
    seg_fwd_pixel<MK, GAP>(vw, vs, target[p], mask ? mask[p] : 1.f, K, ignore_index, do_ent, variant, a);
  }
  seg_acc_store(a, sh, partial);
}

// Four consecutive pixels per thread, K a compile-time constant (round 6): 16-byte loads of every logit plane, the class map
// and the mask, all issued before the first use -- the one-pixel form above ran at 1.2 - 1.7 TB/s of its bytes (r05 profile:
// two dependent rounds of ten 4-byte loads per thread).  The per-pixel arithmetic is the same function in the same order; the
// per-thread and per-block partial sums group the pixels differently, so the SUMS agree to rounding, not bit for bit.
// Host side: HW % 4 == 0, pointers 16-byte aligned, K in {2, 4, 5} (the three data sets), P < 2^31.
template <int KC, bool GAP>
__global__ __launch_bounds__(LS_THREADS) void seg_losses_partial_v4_kernel(
    const float* __restrict__ zw, const float* __restrict__ zs, const long long* __restrict__ target,
    const float* __restrict__ mask, int N, int HW, int ignore_index, int do_ent, int variant,
    double* __restrict__ partial /*[blocks][5]*/) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  __shared__ float sh[16];
  constexpr int K = KC;
  const int Q = (int)(((long long)N * HW) >> 2), HW4 = HW >> 2;
  SegAcc a{0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += gridDim.x * blockDim.x) {
    const int n = (int)((unsigned)q / (unsigned)HW4), hw = (q - n * HW4) << 2;
    const size_t off = (size_t)n * K * HW + hw;
    f32x4 w4[K], s4[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w4[k] = *reinterpret_cast<const f32x4*>(zw + off + (size_t)k * HW);
    if (variant) {
#pragma unroll
      for (int k = 0; k < K; ++k) s4[k] = *reinterpret_cast<const f32x4*>(zs + off + (size_t)k * HW);
    }
    const i64x2 t01 = *reinterpret_cast<const i64x2*>(target + (size_t)q * 4), t23 = *reinterpret_cast<const i64x2*>(target + (size_t)q * 4 + 2);
    const f32x4 m4 = mask ? *reinterpret_cast<const f32x4*>(mask + (size_t)q * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float vw[LS_MAXK], vs[LS_MAXK];
#pragma unroll
      for (int k = 0; k < LS_MAXK; ++k) { vw[k] = k < K ? w4[k < K ? k : 0][j] : 0.f; vs[k] = (k < K && variant) ? s4[k < K ? k : 0][j] : 0.f; }
      seg_fwd_pixel<LS_MAXK, GAP>(vw, vs, j < 2 ? t01[j] : t23[j - 2], m4[j], K, ignore_index, do_ent, variant, a);
    }
  }
  seg_acc_store(a, sh, partial);
}

__global__ __launch_bounds__(64) void seg_losses_reduce_kernel(const double* __restrict__ partial, int nblocks,
                                                               int has_mask, int variant, double unmasked_ent_den,
                                                               double unmasked_cr_den, double* __restrict__ sums) {
  double a[5] = {0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblocks; b += 64)
    for (int j = 0; j < 5; ++j) a[j] += partial[(size_t)b * 5 + j];
  for (int j = 0; j < 5; ++j) a[j] = pp_wave_sum_d(a[j]);
  if (threadIdx.x != 0) return;
  sums[0] = a[0];
  sums[1] = a[1];
  sums[2] = a[2];
  sums[3] = has_mask ? a[4] : unmasked_ent_den;
  sums[4] = a[3];
  sums[5] = has_mask ? a[4] : unmasked_cr_den;
  (void)variant;
}

// loss = sum / den;   masked denominators are clamped as max(mask.sum(), 1e-8)  (losses/losses.py:21,59)
__global__ void losses_finalize_kernel(const double* __restrict__ sums, int has_mask, float* loss_pce, float* loss_ent,
                                       float* loss_cr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (loss_pce) *loss_pce = (float)(sums[0] / sums[1]);              // 0/0 -> NaN like F.cross_entropy
  const double de = has_mask ? fmax(sums[3], 1e-8) : sums[3];
  const double dc = has_mask ? fmax(sums[5], 1e-8) : sums[5];
  if (loss_ent) *loss_ent = (float)(sums[2] / de);
  if (loss_cr) *loss_cr = (float)(sums[4] / dc);
}

// the four-pixels-per-thread forms: 16-byte accesses of every tensor, 32-bit pixel-quad indices
static inline bool seg_v4_ok(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, int N, int K,
                             int HW) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f;
  return HW % 4 == 0 && (bits & 15) == 0 && (long long)N * HW * K < 0x7fffffffLL && (K == 2 || K == 4 || K == 5);
}

extern "C" size_t pp_seg_losses_workspace(int N, int HW) {
  return (size_t)ls_blocks((long long)N * HW, 1024) * 5 * sizeof(double);
}

extern "C" int pp_seg_losses_fwd(const float* logits_w, const float* logits_s, const int64_t* target,
                                 const float* valid_mask, int N, int K, int HW, int ignore_index, int do_ent,
                                 int cr_variant, double* sums, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits_w && target && sums && workspace, "seg_losses_fwd: null pointer");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && cr_variant >= 0 && cr_variant <= 7, "seg_losses_fwd: K=%d (1..%d) variant=%d", K, PP_MAXK, cr_variant);
  PP_CHECK_ARG(cr_variant == 0 || logits_s, "seg_losses_fwd: consistency loss needs the strong logits");
  if (workspace_bytes < pp_seg_losses_workspace(N, HW)) {
    pp_set_error("seg_losses_fwd: workspace too small");
    return PP_ERR_WORKSPACE;
  }
  const int blocks = ls_blocks((long long)N * HW, 1024);
  const double P = (double)N * HW;
  const double den_ent = P * K;                                       // loss.mean() over (N,K,H,W)
  // l1 / l2 / js / hard_ce reduce channels first
  const double den_cr = (cr_variant == 2 || cr_variant == 3 || cr_variant == 6 || cr_variant == 7) ? P : P * K;
  pp_prof_begin(PP_K_LOSS, 0.0, P * (8.0 * K + 12.0), s);
  const bool v4 = seg_v4_ok(logits_w, logits_s, target, valid_mask, nullptr, nullptr, N, K, HW);
  const bool gap = cr_variant >= 5;
#define SEG_FWD_V4_(KC, GAP) hipLaunchKernelGGL((seg_losses_partial_v4_kernel<KC, GAP>), dim3(blocks), dim3(LS_THREADS), 0, s, logits_w, logits_s, \
                     (const long long*)target, valid_mask, N, HW, ignore_index, do_ent, cr_variant, (double*)workspace)
#define SEG_FWD_V4(KC) do { if (gap) SEG_FWD_V4_(KC, true); else SEG_FWD_V4_(KC, false); } while (0)
  if (v4 && K == 5) SEG_FWD_V4(5);
  else if (v4 && K == 4) SEG_FWD_V4(4);
  else if (v4 && K == 2) SEG_FWD_V4(2);
  else
    pp_by_class_bound(K, [&](auto mk) {
      constexpr int MK = decltype(mk)::value;
      auto kern = gap ? seg_losses_partial_kernel<MK, true> : seg_losses_partial_kernel<MK, false>;
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(LS_THREADS), 0, s, logits_w, logits_s,
                         (const long long*)target, valid_mask, N, K, HW, ignore_index, do_ent, cr_variant, (double*)workspace);
    });
#undef SEG_FWD_V4
#undef SEG_FWD_V4_
  hipLaunchKernelGGL(seg_losses_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks,
                     valid_mask ? 1 : 0, cr_variant, den_ent, den_cr, sums);
  pp_prof_end(s);
  return pp_launch_status("seg_losses_fwd");
}

extern "C" int pp_losses_finalize(const double* sums, int has_mask, float* loss_pce, float* loss_ent, float* loss_cr,
                                  void* stream) {
  PP_CHECK_ARG(sums != nullptr, "losses_finalize: null pointer");
  hipLaunchKernelGGL(losses_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, has_mask, loss_pce,
                     loss_ent, loss_cr);
  return pp_launch_status("losses_finalize");
}

// d(sum_i g_i * loss_i)/d logits.  For a per-pixel loss L(q, s) of the weak / strong probabilities with
// partials u = dL/dq, v = dL/ds:  dL/dz_w[k] = q_k (u_k - sum_c q_c u_c),  dL/dz_s[k] = s_k (v_k - sum_c s_c v_c).
struct SegG { float gp, ge, gc; };
__device__ __forceinline__ SegG seg_bwd_scales(const double* __restrict__ sums, int has_mask, int do_ent, int variant,
                                               const float* g_pce, const float* g_ent, const float* g_cr, float grad_scale) {
  SegG g;
  g.gp = (g_pce ? *g_pce : 0.f) * grad_scale / (float)sums[1];
  const double de = has_mask ? fmax(sums[3], 1e-8) : sums[3];
  const double dc = has_mask ? fmax(sums[5], 1e-8) : sums[5];
  g.ge = (do_ent && g_ent) ? (float)((double)(*g_ent * grad_scale) / de) : 0.f;
  g.gc = (variant && g_cr) ? (float)((double)(*g_cr * grad_scale) / dc) : 0.f;
  return g;
}
template <int MK, bool GAP>
__device__ __forceinline__ void seg_bwd_pixel(const float (&vw)[MK], const float (&vs)[MK], long long t, float m, int K,
                                              int ignore_index, int do_ent, int variant, int detach_weak, const SegG& g,
                                              float (&dw)[MK], float (&ds)[MK]) {
  SM<MK> w;
  softmax_vals(vw, K, w);
#pragma unroll
  for (int k = 0; k < MK; ++k) { dw[k] = 0.f; ds[k] = 0.f; }
  if (t != ignore_index && t >= 0 && t < K) {
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) dw[k] = g.gp * (w.p[k] - (k == (int)t ? 1.f : 0.f));
  }
  if (do_ent) {
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k) if (k < K) h -= w.p[k] * w.l[k];
    const float f = g.ge * m;
#pragma unroll
    for (int k = 0; k < MK; ++k) if (k < K) dw[k] -= f * w.p[k] * (w.l[k] + h);
  }
  if (variant) {
    SM<MK> s;
    softmax_vals(vs, K, s);
    if constexpr (GAP) {     // bikl_loss / js_loss honour detach_weak; hard_ce_loss has no weak-view gradient at all
      cr_grad_gap(vw, vs, w, s, K, variant, !detach_weak, g.gc * m, dw, ds);
      return;
    }
    float u[MK], v[MK];
    float qu = 0.f, sv = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        if (variant == 1) { u[k] = -s.l[k]; v[k] = 0.f; }
        else if (variant == 2) {
          const float d = s.p[k] - w.p[k];
          const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
          u[k] = -sg; v[k] = sg;
        } else if (variant == 3) { const float d = s.p[k] - w.p[k]; u[k] = -2.f * d; v[k] = 2.f * d; }
        else { u[k] = w.l[k] - s.l[k] + 1.f; v[k] = 0.f; }
        qu += w.p[k] * u[k];
        sv += s.p[k] * v[k];
      }
    const float f = g.gc * m;
    const bool weak_grad = !(detach_weak && variant != 4);    // kl_loss reads the logits, never detached
    // ce_loss / kl_loss: v = -q/s, so s_k (v_k - sum_c s_c v_c) = s_k - q_k.  The closed form is used because the
    // quotient form is 0 * inf = NaN once a strong-view probability underflows (logit gap > 87): found by the r02
    // multi-seed Dice runs, which died with NaN gradients after ~550 steps; torch's log_softmax backward
    // (the reference, losses/losses.py:54-59) is the closed form too.
    const bool closed = variant == 1 || variant == 4;
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        if (weak_grad) dw[k] += f * w.p[k] * (u[k] - qu);
        ds[k] = closed ? f * (s.p[k] - w.p[k]) : f * s.p[k] * (v[k] - sv);
      }
  }
}

template <int MK, bool GAP>
__global__ __launch_bounds__(LS_THREADS) void seg_losses_bwd_kernel(
    const float* __restrict__ zw, const float* __restrict__ zs, const long long* __restrict__ target,
    const float* __restrict__ mask, int N, int K, int HW, int ignore_index, int do_ent, int variant, int detach_weak,
    const double* __restrict__ sums, int has_mask, const float* __restrict__ g_pce, const float* __restrict__ g_ent,
    const float* __restrict__ g_cr, float grad_scale, float* __restrict__ dzw, float* __restrict__ dzs) {
  const long long P = (long long)N * HW;
  const SegG g = seg_bwd_scales(sums, has_mask, do_ent, variant, g_pce, g_ent, g_cr, grad_scale);
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    // (32-bit division where the pixel index fits: the 64-bit form is ~150 VALU instructions of these kernels' ~870 per pixel)
    const int n = p < 0x7fffffffLL ? (int)((unsigned)p / (unsigned)HW) : (int)(p / HW), hw = (int)(p - (long long)n * HW);
    const size_t off = (size_t)n * K * HW + hw;
    float vw[MK], vs[MK], dw[MK], ds[MK];
#pragma unroll
    for (int k = 0; k < MK; ++k) {
      vw[k] = k < K ? zw[off + (size_t)k * HW] : 0.f;
      vs[k] = (k < K && variant) ? zs[off + (size_t)k * HW] : 0.f;
    }
    seg_bwd_pixel<MK, GAP>(vw, vs, target[p], mask ? mask[p] : 1.f, K, ignore_index, do_ent, variant, detach_weak, g, dw, ds);
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        if (variant) dzs[off + (size_t)k * HW] = ds[k];
        dzw[off + (size_t)k * HW] = dw[k];
      }
  }
}

// four consecutive pixels per thread, compile-time K (see seg_losses_partial_v4_kernel): bit-identical gradients
template <int KC, bool GAP>
__global__ __launch_bounds__(LS_THREADS) void seg_losses_bwd_v4_kernel(
    const float* __restrict__ zw, const float* __restrict__ zs, const long long* __restrict__ target,
    const float* __restrict__ mask, int N, int HW, int ignore_index, int do_ent, int variant, int detach_weak,
    const double* __restrict__ sums, int has_mask, const float* __restrict__ g_pce, const float* __restrict__ g_ent,
    const float* __restrict__ g_cr, float grad_scale, float* __restrict__ dzw, float* __restrict__ dzs) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  constexpr int K = KC;
  const int Q = (int)(((long long)N * HW) >> 2), HW4 = HW >> 2;
  const SegG g = seg_bwd_scales(sums, has_mask, do_ent, variant, g_pce, g_ent, g_cr, grad_scale);
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += gridDim.x * blockDim.x) {
    const int n = (int)((unsigned)q / (unsigned)HW4), hw = (q - n * HW4) << 2;
    const size_t off = (size_t)n * K * HW + hw;
    f32x4 w4[K], s4[K], dw4[K], ds4[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w4[k] = *reinterpret_cast<const f32x4*>(zw + off + (size_t)k * HW);
    if (variant) {
#pragma unroll
      for (int k = 0; k < K; ++k) s4[k] = *reinterpret_cast<const f32x4*>(zs + off + (size_t)k * HW);
    }
    const i64x2 t01 = *reinterpret_cast<const i64x2*>(target + (size_t)q * 4), t23 = *reinterpret_cast<const i64x2*>(target + (size_t)q * 4 + 2);
    const f32x4 m4 = mask ? *reinterpret_cast<const f32x4*>(mask + (size_t)q * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float vw[LS_MAXK], vs[LS_MAXK], dw[LS_MAXK], ds[LS_MAXK];
#pragma unroll
      for (int k = 0; k < LS_MAXK; ++k) { vw[k] = k < K ? w4[k < K ? k : 0][j] : 0.f; vs[k] = (k < K && variant) ? s4[k < K ? k : 0][j] : 0.f; }
      seg_bwd_pixel<LS_MAXK, GAP>(vw, vs, j < 2 ? t01[j] : t23[j - 2], m4[j], K, ignore_index, do_ent, variant, detach_weak, g, dw, ds);
#pragma unroll
      for (int k = 0; k < K; ++k) { dw4[k][j] = dw[k]; ds4[k][j] = ds[k]; }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (variant) *reinterpret_cast<f32x4*>(dzs + off + (size_t)k * HW) = ds4[k];
      *reinterpret_cast<f32x4*>(dzw + off + (size_t)k * HW) = dw4[k];
    }
  }
}

extern "C" int pp_seg_losses_bwd(const float* logits_w, const float* logits_s, const int64_t* target,
                                 const float* valid_mask, int N, int K, int HW, int ignore_index, int do_ent,
                                 int cr_variant, int detach_weak, const double* sums, const float* g_pce,
                                 const float* g_ent, const float* g_cr, float grad_scale, float* dlogits_w,
                                 float* dlogits_s, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits_w && target && sums && dlogits_w, "seg_losses_bwd: null pointer");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && cr_variant >= 0 && cr_variant <= 7, "seg_losses_bwd: K=%d (1..%d) variant=%d", K, PP_MAXK, cr_variant);
  PP_CHECK_ARG(cr_variant == 0 || (logits_s && dlogits_s), "seg_losses_bwd: consistency loss needs the strong logits");
  const double P = (double)N * HW;
  pp_prof_begin(PP_K_LOSS, 0.0, P * (16.0 * K + 12.0), s);
  const bool v4 = seg_v4_ok(logits_w, logits_s, target, valid_mask, dlogits_w, dlogits_s, N, K, HW);
  const bool gap = cr_variant >= 5;
#define SEG_BWD_V4_(KC, GAP) hipLaunchKernelGGL((seg_losses_bwd_v4_kernel<KC, GAP>), dim3(ls_blocks((long long)N * HW / 4, 8192)), dim3(LS_THREADS), 0, s, \
                     logits_w, logits_s, (const long long*)target, valid_mask, N, HW, ignore_index, do_ent, cr_variant,        \
                     detach_weak, sums, valid_mask ? 1 : 0, g_pce, g_ent, g_cr, grad_scale, dlogits_w, dlogits_s)
#define SEG_BWD_V4(KC) do { if (gap) SEG_BWD_V4_(KC, true); else SEG_BWD_V4_(KC, false); } while (0)
  if (v4 && K == 5) SEG_BWD_V4(5);
  else if (v4 && K == 4) SEG_BWD_V4(4);
  else if (v4 && K == 2) SEG_BWD_V4(2);
  else
    pp_by_class_bound(K, [&](auto mk) {
      constexpr int MK = decltype(mk)::value;
      auto kern = gap ? seg_losses_bwd_kernel<MK, true> : seg_losses_bwd_kernel<MK, false>;
      hipLaunchKernelGGL(kern, dim3(ls_blocks((long long)N * HW)), dim3(LS_THREADS), 0, s, logits_w,
                         logits_s, (const long long*)target, valid_mask, N, K, HW, ignore_index, do_ent, cr_variant,
                         detach_weak, sums, valid_mask ? 1 : 0, g_pce, g_ent, g_cr, grad_scale, dlogits_w, dlogits_s);
    });
#undef SEG_BWD_V4
#undef SEG_BWD_V4_
  pp_prof_end(s);
  return pp_launch_status("seg_losses_bwd");
}

// ---------------------------------------------------------------- auxiliary head: up-sample + partial CE
__device__ __forceinline__ void lin_coeff_l(int o, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
  const float src = scale * (float)o;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}
static inline float lin_scale_l(int in_size, int out_size) {
  return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
}

template <int MK>
__global__ __launch_bounds__(LS_THREADS) void aux_pce_fwd_kernel(const float* __restrict__ lo, int N, int K, int h,
                                                                 int w, int H, int W, float sy, float sx,
                                                                 const long long* __restrict__ target,
                                                                 int ignore_index, float* __restrict__ up,
                                                                 double* __restrict__ partial /*[blocks][2]*/) {
  __shared__ float sh[16];
  const long long P = (long long)N * H * W;
  const int HW = H * W, hw_lo = h * w;
  float a_pce = 0.f, a_n = 0.f;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(p / HW), pix = (int)(p % HW);
    const int y = pix / W, x = pix % W;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    lin_coeff_l(y, sy, h, y0, y1, wy0, wy1);
    lin_coeff_l(x, sx, w, x0, x1, wx0, wx1);
    float v[MK];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float* b = lo + ((size_t)n * K + k) * hw_lo;
        v[k] = wy0 * (wx0 * b[y0 * w + x0] + wx1 * b[y0 * w + x1]) + wy1 * (wx0 * b[y1 * w + x0] + wx1 * b[y1 * w + x1]);
        up[((size_t)n * K + k) * HW + pix] = v[k];
        m = fmaxf(m, v[k]);
      }
    const long long t = target[p];
    if (t != ignore_index && t >= 0 && t < K) {
      float s = 0.f, vt = 0.f;
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) { s += expf(v[k] - m); if (k == (int)t) vt = v[k]; }
      a_pce -= vt - m - logf(s);
      a_n += 1.f;
    }
  }
  const float r0 = pp_block_sum(a_pce, sh), r1 = pp_block_sum(a_n, sh);
  if (threadIdx.x == 0) { partial[(size_t)blockIdx.x * 2] = r0; partial[(size_t)blockIdx.x * 2 + 1] = r1; }
}

__global__ __launch_bounds__(64) void pair_reduce_kernel(const double* __restrict__ partial, int nblocks,
                                                         double* __restrict__ sums) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) { a += partial[(size_t)i * 2]; b += partial[(size_t)i * 2 + 1]; }
  a = pp_wave_sum_d(a);
  b = pp_wave_sum_d(b);
  if (threadIdx.x == 0) { sums[0] = a; sums[1] = b; }
}

extern "C" int pp_aux_pce_fwd(const float* lo, int N, int K, int h, int w, int H, int W, const int64_t* target,
                              int ignore_index, float* logits_up, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(lo && target && logits_up && sums && workspace, "aux_pce_fwd: null pointer");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "aux_pce_fwd: K=%d (1..%d)", K, PP_MAXK);
  const int blocks = ls_blocks((long long)N * H * W, 1024);
  if (workspace_bytes < (size_t)blocks * 2 * sizeof(double)) {
    pp_set_error("aux_pce_fwd: workspace too small");
    return PP_ERR_WORKSPACE;
  }
  pp_prof_begin(PP_K_LOSS, 0.0, (double)N * H * W * (4.0 * K + 8.0), s);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(aux_pce_fwd_kernel<decltype(mk)::value>, dim3(blocks), dim3(LS_THREADS), 0, s, lo, N, K, h, w, H, W, lin_scale_l(h, H),
                       lin_scale_l(w, W), (const long long*)target, ignore_index, logits_up, (double*)workspace);
  });
  hipLaunchKernelGGL(pair_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, sums);
  pp_prof_end(s);
  return pp_launch_status("aux_pce_fwd");
}

__device__ __forceinline__ void touch_range_l(int i, float scale, int out_size, int& lo, int& hi) {
  if (scale <= 0.f) { lo = 0; hi = out_size - 1; return; }
  lo = (int)floorf((float)(i - 1) / scale) - 1;
  hi = (int)ceilf((float)(i + 1) / scale) + 1;
  if (lo < 0) lo = 0;
  if (hi > out_size - 1) hi = out_size - 1;
}

// One WAVE per low-res pixel gathers the gradient of every labelled high-res pixel that taps it (round 6; round 2 used 16 lanes
// per pixel, each walking its rows of the ~20 x 20 support window one class-map load at a time: 149 us for 99 MB, 0.67 TB/s).
// Phase 1: the lanes take the window positions lane, lane + 64, ... (AUXB_SLOTS per lane and round) and load their class-map
// entries together -- independent loads, one latency.  The labelled ones (a few per cent of a scribble map) are COMPACTED into
// a per-wave list in LDS, ranked by ballot + population count (position order: deterministic).  Phase 2: lane r evaluates the
// softmax of the up-sampled logits and the bilinear weight of list entry r -- ONE pass for up to 64 labelled positions, where
// a direct walk over the slots executed the softmax body once per slot with most lanes idle.  The 64 per-lane sums are folded by
// the xor butterfly: a fixed order.
#define AUXB_SLOTS 8
#define AUXB_LIST (64 * AUXB_SLOTS)        // labelled positions of one phase-1 round: at most every slot of every lane
template <int MK>
__global__ __launch_bounds__(256) void aux_pce_bwd_kernel(const float* __restrict__ up, const long long* __restrict__ target,
                                                          int ignore_index, const float* __restrict__ g_aux,
                                                          float grad_scale, const double* __restrict__ sums,
                                                          float* __restrict__ dlo, int N, int K, int h, int w, int H,
                                                          int W, float sy, float sx) {
  __shared__ int l_pos[4][AUXB_LIST];
  __shared__ unsigned char l_t[4][AUXB_LIST];
  const int total = N * h * w;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);        // wave-uniform
  if (i >= total) return;                                                    // (no block-wide barrier below: whole waves may leave)
  const int xl = i % w, yl = (i / w) % h, n = i / (w * h);
  const int HW = H * W;
  const float gs = (g_aux ? *g_aux : 0.f) * grad_scale / (float)sums[1];
  int ylo, yhi, xlo, xhi;
  touch_range_l(yl, sy, H, ylo, yhi);
  touch_range_l(xl, sx, W, xlo, xhi);
  const int wx = xhi - xlo + 1, cnt = (yhi - ylo + 1) * wx;
  const long long* tgt = target + (size_t)n * HW;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  float acc[MK];
#pragma unroll
  for (int k = 0; k < MK; ++k) acc[k] = 0.f;
  for (int base = 0; base < cnt; base += 64 * AUXB_SLOTS) {
    long long t[AUXB_SLOTS];
    int pos[AUXB_SLOTS];
#pragma unroll
    for (int j = 0; j < AUXB_SLOTS; ++j) {
      const int idx = base + j * 64 + lane;
      const int dy = (int)((unsigned)idx / (unsigned)wx), dx = idx - dy * wx;
      pos[j] = idx < cnt ? (ylo + dy) * W + xlo + dx : -1;
      t[j] = pos[j] >= 0 ? tgt[pos[j]] : (long long)ignore_index;
    }
    int n_list = 0;                                                         // wave-uniform
#pragma unroll
    for (int j = 0; j < AUXB_SLOTS; ++j) {
      const bool lab = pos[j] >= 0 && t[j] != ignore_index && t[j] >= 0 && t[j] < K;
      const unsigned long long m = __ballot(lab);
      if (lab) {
        const int r = n_list + __popcll(m & lt_mask);
        l_pos[wv][r] = pos[j];
        l_t[wv][r] = (unsigned char)t[j];
      }
      n_list += __popcll(m);
    }
    // the list is written and read by the same wave: its LDS operations complete in issue order, the fence keeps the compiler from
    // moving the reads of other lanes' entries above the writes
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int r = lane; r < n_list; r += 64) {
      const int p = l_pos[wv][r], tt = (int)l_t[wv][r];
      const int y = p / W, x = p - y * W;
      int y0, y1, x0, x1; float wy0, wy1, wx0, wx1;
      lin_coeff_l(y, sy, h, y0, y1, wy0, wy1);
      lin_coeff_l(x, sx, w, x0, x1, wx0, wx1);
      const float wgt = ((y0 == yl ? wy0 : 0.f) + (y1 == yl ? wy1 : 0.f)) * ((x0 == xl ? wx0 : 0.f) + (x1 == xl ? wx1 : 0.f));
      if (wgt == 0.f) continue;
      SM<MK> sm;
      pixel_softmax(up + (size_t)n * K * HW + p, HW, K, sm);
#pragma unroll
      for (int k = 0; k < MK; ++k)
        if (k < K) acc[k] += wgt * (sm.p[k] - (k == tt ? 1.f : 0.f));
    }
  }
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      const float v = pp_wave_sum(acc[k]);
      if (lane == 0) dlo[((size_t)n * K + k) * h * w + yl * w + xl] = v * gs;
    }
}

extern "C" int pp_aux_pce_bwd(const float* logits_up, const int64_t* target, int ignore_index, const float* g_aux,
                              float grad_scale, const double* sums, float* dlo, int N, int K, int h, int w, int H,
                              int W, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits_up && target && sums && dlo, "aux_pce_bwd: null pointer");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "aux_pce_bwd: K=%d (1..%d)", K, PP_MAXK);
  pp_prof_begin(PP_K_LOSS, 0.0, (double)N * H * W * 8.0, s);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(aux_pce_bwd_kernel<decltype(mk)::value>, dim3(pp_cdiv((long long)N * h * w * 64, 256)), dim3(256), 0, s, logits_up,
                       (const long long*)target, ignore_index, g_aux, grad_scale, sums, dlo, N, K, h, w, H, W,
                       lin_scale_l(h, H), lin_scale_l(w, W));
  });
  pp_prof_end(s);
  return pp_launch_status("aux_pce_bwd");
}

// ---------------------------------------------------------------- memory bank (aux_path_memory.py:68-116)
// Round 6: two launches.  memory_partial_kernel, grid (classes, MEMU_SLICES): a block of four waves scans one slice of sample 0's
// scribble plane -- every wave requests its MEM_SCAN 64-pixel strips together, then visits the selected pixels MEM_VB at a time
// with the 64 lanes spread over the hid channels of the bilinearly up-sampled feature -- and leaves per-wave partial sums
// (sum of [weighted] embeddings, sum of weights, count).  memory_finalize_kernel, one block per class, adds them in (slice, wave)
// order and applies the first-visit / EMA rule.  (Round 1 ran ONE block of 16 waves per class, a dependent load per 64 pixels:
// 92 us for 2 MB on five of 256 CUs.)
#define MEMU_SLICES 64
#define MEMU_WAVES 4
#define MEM_CPL 4                 // channels per lane: hid <= 256
#define MEM_SCAN 4                // plane loads in flight per wave and round
#define MEM_VB 4                  // selected pixels whose corner rows are requested together

extern "C" size_t pp_memory_update_workspace(int K, int hid) {
  return (size_t)(K > 0 ? K : 0) * MEMU_SLICES * MEMU_WAVES * ((hid > 0 ? hid : 0) + 2) * sizeof(float);
}

// bank row: all-zero test and L2-normalised copy (wave 0 of the block; the caller synchronises)
__device__ __forceinline__ void memory_row_state(const float* __restrict__ row, int hid, int lane, float* row_hat, int* first_visit) {
  float nz = 0.f, sq = 0.f;
  for (int c = lane; c < hid; c += 64) { const float v = row[c]; nz += (v != 0.f) ? 1.f : 0.f; sq += v * v; }
  nz = pp_wave_sum(nz);
  sq = pp_wave_sum(sq);
  const float inv = 1.f / (sqrtf(sq) + 1e-8f);
  for (int c = lane; c < hid; c += 64) row_hat[c] = row[c] * inv;
  if (lane == 0) *first_visit = (nz == 0.f);
}

template <class FT>               // element type of the feature map: float, or _Float16 / __bf16 in the 16-bit storage modes
__global__ __launch_bounds__(MEMU_WAVES * 64) void memory_partial_kernel(
    const FT* __restrict__ feat, int ld, int hid, int h, int w, const float* __restrict__ scb0, int H, int W,
    float sy, float sx, const float* __restrict__ bank, int cosine_mode, float* __restrict__ partial) {
  __shared__ float row_hat[MEM_CPL * 64];
  __shared__ int first_visit;
  const int cls = blockIdx.x, slice = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* plane = scb0 + (size_t)cls * H * W;
  if (wv == 0) memory_row_state(bank + (size_t)cls * hid, hid, lane, row_hat, &first_visit);
  __syncthreads();
  const bool plain_mean = first_visit || !cosine_mode;
  float U[MEM_CPL] = {0.f, 0.f, 0.f, 0.f};
  float S = 0.f, cnt = 0.f;
  float rh[MEM_CPL];
#pragma unroll
  for (int j = 0; j < MEM_CPL; ++j) rh[j] = (lane + 64 * j < hid) ? row_hat[lane + 64 * j] : 0.f;
  const int HW = H * W;
  const int per = (HW + MEMU_SLICES - 1) / MEMU_SLICES;
  const int p_lo = slice * per, p_hi = (p_lo + per < HW) ? p_lo + per : HW;
  for (int base = p_lo + wv * 64; base < p_hi; base += MEMU_WAVES * 64 * MEM_SCAN) {
    unsigned long long bits_u[MEM_SCAN];
#pragma unroll
    for (int u = 0; u < MEM_SCAN; ++u) {
      const int pix = base + u * MEMU_WAVES * 64 + lane;
      bits_u[u] = __ballot(pix < p_hi && plane[pix] == 1.f);
    }
#pragma unroll
    for (int u = 0; u < MEM_SCAN; ++u) {
      unsigned long long bits = bits_u[u];
      const int base_u = base + u * MEMU_WAVES * 64;
      while (bits) {
        int q[MEM_VB];
#pragma unroll
        for (int b = 0; b < MEM_VB; ++b) {
          q[b] = -1;
          if (bits) { q[b] = base_u + __ffsll((long long)bits) - 1; bits &= bits - 1; }
        }
        float fa[MEM_VB][MEM_CPL], fb[MEM_VB][MEM_CPL], fc[MEM_VB][MEM_CPL], fd[MEM_VB][MEM_CPL];
        float wy0[MEM_VB], wy1[MEM_VB], wx0[MEM_VB], wx1[MEM_VB];
#pragma unroll
        for (int b = 0; b < MEM_VB; ++b) {
          if (q[b] < 0) continue;
          const int y = q[b] / W, x = q[b] % W;
          int y0, y1, x0, x1;
          lin_coeff_l(y, sy, h, y0, y1, wy0[b], wy1[b]);
          lin_coeff_l(x, sx, w, x0, x1, wx0[b], wx1[b]);
#pragma unroll
          for (int j = 0; j < MEM_CPL; ++j) {
            const int c = lane + 64 * j;
            if (c < hid) {
              fa[b][j] = feat[(size_t)(y0 * w + x0) * ld + c]; fb[b][j] = feat[(size_t)(y0 * w + x1) * ld + c];
              fc[b][j] = feat[(size_t)(y1 * w + x0) * ld + c]; fd[b][j] = feat[(size_t)(y1 * w + x1) * ld + c];
            }
          }
        }
#pragma unroll
        for (int b = 0; b < MEM_VB; ++b) {
          if (q[b] < 0) continue;
          float e[MEM_CPL];
          float sq = 0.f;
#pragma unroll
          for (int j = 0; j < MEM_CPL; ++j) {
            const int c = lane + 64 * j;
            e[j] = 0.f;
            if (c < hid) {
              const float a = fa[b][j], bb = fb[b][j], cc = fc[b][j], d = fd[b][j];
              e[j] = wy0[b] * (wx0[b] * a + wx1[b] * bb) + wy1[b] * (wx0[b] * cc + wx1[b] * d);
              sq += e[j] * e[j];
            }
          }
          cnt += 1.f;
          if (plain_mean) {
#pragma unroll
            for (int j = 0; j < MEM_CPL; ++j) U[j] += e[j];
          } else {
            sq = pp_wave_sum(sq);
            const float inv = 1.f / (sqrtf(sq) + 1e-8f);
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < MEM_CPL; ++j) { e[j] *= inv; dot += e[j] * rh[j]; }
            dot = pp_wave_sum(dot);
            const float om = 1.f - dot;
            S += om;
#pragma unroll
            for (int j = 0; j < MEM_CPL; ++j) U[j] += e[j] * om;
          }
        }
      }
    }
  }
  float* o = partial + ((size_t)(cls * MEMU_SLICES + slice) * MEMU_WAVES + wv) * (hid + 2);
#pragma unroll
  for (int j = 0; j < MEM_CPL; ++j)
    if (lane + 64 * j < hid) o[lane + 64 * j] = U[j];
  if (lane == 0) { o[hid] = S; o[hid + 1] = cnt; }
}

#define MEMU_FIN_WAVES 4
__global__ __launch_bounds__(MEMU_FIN_WAVES * 64) void memory_finalize_kernel(const float* __restrict__ partial, int hid,
                                                                              float* __restrict__ bank, float mom, int cosine_mode) {
  __shared__ float row_hat[MEM_CPL * 64];
  __shared__ int first_visit;
  __shared__ float part[MEMU_FIN_WAVES][MEM_CPL * 64 + 2];
  const int cls = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* row = bank + (size_t)cls * hid;
  if (wv == 0) memory_row_state(row, hid, lane, row_hat, &first_visit);
  // wave wv adds its quarter of the (slice, wave) partial rows in order, eight loads in flight; the four quarter sums are then
  // added in wave order: a fixed order over all MEMU_SLICES * MEMU_WAVES rows
  constexpr int ROWS = MEMU_SLICES * MEMU_WAVES, PER = ROWS / MEMU_FIN_WAVES;
  const float* p0 = partial + ((size_t)cls * ROWS + (size_t)wv * PER) * (hid + 2);
  for (int c = lane; c < hid + 2; c += 64) {
    float u = 0.f;
#pragma unroll 8
    for (int k = 0; k < PER; ++k) u += p0[(size_t)k * (hid + 2) + c];
    part[wv][c] = u;
  }
  __syncthreads();
  if (wv != 0) return;
  float St = 0.f, ct = 0.f;
#pragma unroll
  for (int q = 0; q < MEMU_FIN_WAVES; ++q) { St += part[q][hid]; ct += part[q][hid + 1]; }
  if (ct == 0.f) return;                                       // no scribble of this class in sample 0 (uniform over the block)
  for (int c = lane; c < hid; c += 64) {
    float u = 0.f;
#pragma unroll
    for (int q = 0; q < MEMU_FIN_WAVES; ++q) u += part[q][c];
    float nv;
    if (first_visit) {
      nv = u / ct;                                             // first visit: plain mean, no EMA
    } else {
      const float upd = cosine_mode ? u / (St + 1e-8f) : u / ct;
      const float old = cosine_mode ? row_hat[c] : row[c];     // cosine mode normalises the stored row in place
      nv = (1.f - mom) * old + mom * upd;
    }
    row[c] = nv;
  }
}

template <class FT>
static int memory_update_impl(const FT* feat0, int ld, int hid, int h, int w, const float* scribble0, int K,
                              int H, int W, float* bank, float momentum_now, int cosine_mode, void* workspace,
                              size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(feat0 && scribble0 && bank && workspace, "memory_update: null pointer");
  PP_CHECK_ARG(hid >= 1 && hid <= MEM_CPL * 64 && K >= 1 && ld >= hid, "memory_update: hid=%d (<=256) K=%d", hid, K);
  if (workspace_bytes < pp_memory_update_workspace(K, hid)) {
    pp_set_error("memory_update: workspace too small (%zu < %zu)", workspace_bytes, pp_memory_update_workspace(K, hid));
    return PP_ERR_WORKSPACE;
  }
  pp_prof_begin(PP_K_LOSS, 0.0, 4.0 * K * H * W, s);
  hipLaunchKernelGGL(memory_partial_kernel<FT>, dim3(K, MEMU_SLICES), dim3(MEMU_WAVES * 64), 0, s, feat0, ld, hid, h, w, scribble0, H,
                     W, lin_scale_l(h, H), lin_scale_l(w, W), (const float*)bank, cosine_mode, (float*)workspace);
  hipLaunchKernelGGL(memory_finalize_kernel, dim3(K), dim3(MEMU_FIN_WAVES * 64), 0, s, (const float*)workspace, hid, bank, momentum_now, cosine_mode);
  pp_prof_end(s);
  return pp_launch_status("memory_update");
}

extern "C" int pp_memory_update(const float* feat0, int ld, int hid, int h, int w, const float* scribble0, int K,
                                int H, int W, float* bank, float momentum_now, int cosine_mode, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return memory_update_impl(feat0, ld, hid, h, w, scribble0, K, H, W, bank, momentum_now, cosine_mode, workspace, workspace_bytes, stream);
}
// the same with the features stored as IEEE fp16 (16-bit storage mode, include/pacingpseudo_hip_h16.h)
extern "C" int pp_memory_update_h16(const void* feat0, int ld, int hid, int h, int w, const float* scribble0, int K,
                                    int H, int W, float* bank, float momentum_now, int cosine_mode, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return memory_update_impl(reinterpret_cast<const _Float16*>(feat0), ld, hid, h, w, scribble0, K, H, W, bank, momentum_now,
                            cosine_mode, workspace, workspace_bytes, stream);
}
// ... and as bfloat16 (include/pacingpseudo_hip_bf16.h)
extern "C" int pp_memory_update_bf16(const void* feat0, int ld, int hid, int h, int w, const float* scribble0, int K,
                                     int H, int W, float* bank, float momentum_now, int cosine_mode, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return memory_update_impl(reinterpret_cast<const __bf16*>(feat0), ld, hid, h, w, scribble0, K, H, W, bank, momentum_now,
                            cosine_mode, workspace, workspace_bytes, stream);
}

// bank classification: logits[r][k] = <bank[r], wfc[k]>, loss = mean_r CE(logits[r], r)   (aux_path_memory.py:61,
// consistency_reglur_memory.py:94-97).  mode 0: write loss;  mode 1: dwfc (+)= g * dloss/dwfc.
template <int MK>
__global__ __launch_bounds__(64) void memory_ce_kernel(const float* __restrict__ bank, const float* __restrict__ wfc,
                                                       int K, int hid, float* loss, const float* g, float grad_scale,
                                                       float* dwfc, int accumulate, int mode) {
  __shared__ float lg[MK][MK];
  __shared__ float dl[MK][MK];
  const int lane = threadIdx.x;
  for (int r = 0; r < K; ++r)
    for (int k = 0; k < K; ++k) {
      float a = 0.f;
      for (int c = lane; c < hid; c += 64) a += bank[r * hid + c] * wfc[k * hid + c];
      a = pp_wave_sum(a);
      if (lane == 0) lg[r][k] = a;
    }
  __syncthreads();
  if (lane == 0) {
    float tot = 0.f;
    for (int r = 0; r < K; ++r) {
      float m = -INFINITY, s = 0.f;
      for (int k = 0; k < K; ++k) m = fmaxf(m, lg[r][k]);
      for (int k = 0; k < K; ++k) s += expf(lg[r][k] - m);
      const float ls = logf(s);
      tot -= lg[r][r] - m - ls;
      for (int k = 0; k < K; ++k) dl[r][k] = (expf(lg[r][k] - m - ls) - (k == r ? 1.f : 0.f)) / (float)K;
    }
    if (mode == 0 && loss) *loss = tot / (float)K;
  }
  __syncthreads();
  if (mode == 1) {
    const float gs = (g ? *g : 0.f) * grad_scale;
    for (int k = 0; k < K; ++k)
      for (int c = lane; c < hid; c += 64) {
        float a = 0.f;
        for (int r = 0; r < K; ++r) a += dl[r][k] * bank[r * hid + c];
        dwfc[k * hid + c] = (accumulate ? dwfc[k * hid + c] : 0.f) + gs * a;
      }
  }
}

extern "C" int pp_memory_ce_fwd(const float* bank, const float* wfc, int K, int hid, float* loss, void* stream) {
  PP_CHECK_ARG(bank && wfc && loss, "memory_ce_fwd: bad arguments");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "memory_ce_fwd: K=%d (1..%d)", K, PP_MAXK);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(memory_ce_kernel<decltype(mk)::value>, dim3(1), dim3(64), 0, (hipStream_t)stream, bank, wfc, K, hid, loss, nullptr,
                       0.f, nullptr, 0, 0);
  });
  return pp_launch_status("memory_ce_fwd");
}

extern "C" int pp_memory_ce_bwd(const float* bank, const float* wfc, int K, int hid, const float* g, float grad_scale,
                                float* dwfc, int accumulate, void* stream) {
  PP_CHECK_ARG(bank && wfc && dwfc, "memory_ce_bwd: bad arguments");
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK, "memory_ce_bwd: K=%d (1..%d)", K, PP_MAXK);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(memory_ce_kernel<decltype(mk)::value>, dim3(1), dim3(64), 0, (hipStream_t)stream, bank, wfc, K, hid, nullptr, g,
                       grad_scale, dwfc, accumulate, 1);
  });
  return pp_launch_status("memory_ce_bwd");
}

// ---------------------------------------------------------------- validation Dice counts (utils/metrics.py:7-34)
// counts[n][k] = { sum pred_k * target_k, sum pred_k, sum target_k } with pred = one-hot(argmax_k logits)
template <int MK>
__global__ __launch_bounds__(LS_THREADS) void dice_counts_kernel(const float* __restrict__ logits,
                                                                 const float* __restrict__ label, int K, int HW,
                                                                 float* __restrict__ counts) {
  __shared__ float sh[16];
  const int n = blockIdx.x;
  float inter[MK], ps[MK], ts[MK];
#pragma unroll
  for (int k = 0; k < MK; ++k) inter[k] = ps[k] = ts[k] = 0.f;
  const float* lz = logits + (size_t)n * K * HW;
  const float* lb = label + (size_t)n * K * HW;
  for (int p = threadIdx.x; p < HW; p += blockDim.x) {
    float m = lz[p];
    int a = 0;
    for (int k = 1; k < K; ++k) { const float v = lz[(size_t)k * HW + p]; if (v > m) { m = v; a = k; } }
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float t = lb[(size_t)k * HW + p];
        const float pr = (k == a) ? 1.f : 0.f;
        inter[k] += pr * t; ps[k] += pr; ts[k] += t;
      }
  }
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      const float a = pp_block_sum(inter[k], sh), b = pp_block_sum(ps[k], sh), c = pp_block_sum(ts[k], sh);
      if (threadIdx.x == 0) {
        float* o = counts + ((size_t)n * K + k) * 3;
        o[0] = a; o[1] = b; o[2] = c;
      }
    }
}

extern "C" int pp_dice_counts(const float* logits, const float* label_onehot, int N, int K, int HW, float* counts,
                              void* stream) {
  PP_CHECK_ARG(logits && label_onehot && counts && K >= 1, "dice_counts: bad arguments");
  PP_CHECK_ARG(K <= PP_MAXK, "dice_counts: K=%d (1..%d)", K, PP_MAXK);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(dice_counts_kernel<decltype(mk)::value>, dim3(N), dim3(LS_THREADS), 0, (hipStream_t)stream, logits, label_onehot,
                       K, HW, counts);
  });
  return pp_launch_status("dice_counts");
}

// ---------------------------------------------------------------- soft Dice loss (losses/losses.py:147-162, upper_bound_chaos.py)
// dice[n][k] = 2 sum_i p_k t_k / (sum_i p_k + sum_i t_k + 1e-5) on the soft-max probabilities; loss = -mean_{n,k} dice.
// Forward: blocks (x, n) reduce their pixel range of image n into partial[n][blk][K][3] (double); a finalize folds
// the partials into sums[n][K][3] = {sum p t, sum p, sum t} and writes the loss.
// Backward: dL/dp_k = -g/(N K) * (2 t_k down - up) / down^2 per pixel, then through the soft-max.
#define DICE_BLOCKS 64
template <int MK>
__global__ __launch_bounds__(LS_THREADS) void dice_loss_partial_kernel(const float* __restrict__ logits,
                                                                       const float* __restrict__ label, int K, int HW,
                                                                       double* __restrict__ partial) {
  __shared__ float sh[16];
  const int n = blockIdx.y;
  float inter[MK], ps[MK], ts[MK];
#pragma unroll
  for (int k = 0; k < MK; ++k) inter[k] = ps[k] = ts[k] = 0.f;
  const float* lz = logits + (size_t)n * K * HW;
  const float* lb = label + (size_t)n * K * HW;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    SM<MK> w;
    pixel_softmax(lz + p, HW, K, w);
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float t = lb[(size_t)k * HW + p];
        inter[k] += w.p[k] * t; ps[k] += w.p[k]; ts[k] += t;
      }
  }
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < K) {
      const float a = pp_block_sum(inter[k], sh), b = pp_block_sum(ps[k], sh), c = pp_block_sum(ts[k], sh);
      if (threadIdx.x == 0) {
        double* o = partial + (((size_t)n * gridDim.x + blockIdx.x) * K + k) * 3;
        o[0] = a; o[1] = b; o[2] = c;
      }
    }
}

__global__ __launch_bounds__(64) void dice_loss_finalize_kernel(const double* __restrict__ partial, int nblk, int N, int K,
                                                                double* __restrict__ sums, float* __restrict__ loss) {
  __shared__ double dice[64];
  const int i = threadIdx.x;                     // (n, k) pairs handled in strides of 64
  double tot = 0.0;
  for (int e = i; e < N * K; e += 64) {
    const int n = e / K, k = e % K;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
      const double* o = partial + (((size_t)n * nblk + blk) * K + k) * 3;
      a += o[0]; b += o[1]; c += o[2];
    }
    double* s = sums + (size_t)e * 3;
    s[0] = a; s[1] = b; s[2] = c;
    tot += 2.0 * a / (b + c + 1e-5);
  }
  dice[i] = tot;
  __syncthreads();
  if (i == 0) {
    double t = 0.0;
    for (int j = 0; j < 64; ++j) t += dice[j];
    *loss = (float)(-t / (double)(N * K));
  }
}

template <int MK>
__global__ __launch_bounds__(LS_THREADS) void dice_loss_bwd_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ label, int N, int K, int HW,
                                                                   const double* __restrict__ sums, const float* __restrict__ g,
                                                                   float grad_scale, float* __restrict__ dlogits,
                                                                   int accumulate) {
  const int n = blockIdx.y;
  const float gs = (g ? *g : 1.f) * grad_scale / (float)(N * K);
  // dL/dp_k = A_k t_k + B_k.  The wide forms (MK > LS_MAXK) keep A and B in LDS: in registers they took the MK = 32 form to
  // 228 VGPRs + 32 AGPRs, one wave per SIMD.  Same values either way.
  constexpr bool ab_lds = MK > LS_MAXK;
  __shared__ float ab_sh[ab_lds ? 2 * MK : 1];
  float A[ab_lds ? 1 : MK], B[ab_lds ? 1 : MK];
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    float a = 0.f, b = 0.f;
    if (k < K) {
      const double* s = sums + ((size_t)n * K + k) * 3;
      const double up = 2.0 * s[0], down = s[1] + s[2] + 1e-5;
      a = (float)(-2.0 * gs / down);
      b = (float)(gs * up / (down * down));
    }
    if constexpr (ab_lds) {
      if (threadIdx.x == 0) { ab_sh[k] = a; ab_sh[MK + k] = b; }
    } else {
      A[k] = a; B[k] = b;
    }
  }
  if constexpr (ab_lds) __syncthreads();
  const float* lz = logits + (size_t)n * K * HW;
  const float* lb = label + (size_t)n * K * HW;
  float* dz = dlogits + (size_t)n * K * HW;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    SM<MK> w;
    pixel_softmax(lz + p, HW, K, w);
    float u[MK], pu = 0.f;
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float ak = ab_lds ? ab_sh[k] : A[ab_lds ? 0 : k], bk = ab_lds ? ab_sh[MK + k] : B[ab_lds ? 0 : k];
        u[k] = ak * lb[(size_t)k * HW + p] + bk;
        pu += w.p[k] * u[k];
      }
#pragma unroll
    for (int k = 0; k < MK; ++k)
      if (k < K) {
        const float v = w.p[k] * (u[k] - pu);
        float* o = dz + (size_t)k * HW + p;
        *o = accumulate ? *o + v : v;
      }
  }
}

extern "C" size_t pp_dice_loss_workspace(int N, int K) { return (size_t)N * DICE_BLOCKS * K * 3 * sizeof(double) + 64; }

extern "C" int pp_dice_loss_fwd(const float* logits, const float* label_onehot, int N, int K, int HW, double* sums,
                                float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && label_onehot && sums && loss && workspace && N >= 1 && K >= 1 && HW >= 1,
               "dice_loss_fwd: bad arguments");
  PP_CHECK_ARG(K <= PP_MAXK, "dice_loss_fwd: K=%d (1..%d)", K, PP_MAXK);
  if (workspace_bytes < pp_dice_loss_workspace(N, K)) {
    pp_set_error("dice_loss_fwd: workspace too small");
    return PP_ERR_WORKSPACE;
  }
  double* partial = reinterpret_cast<double*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  int bx = pp_cdiv(HW, LS_THREADS);
  if (bx > DICE_BLOCKS) bx = DICE_BLOCKS;
  pp_prof_begin(PP_K_LOSS, 0.0, 8.0 * (double)N * K * HW, s);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(dice_loss_partial_kernel<decltype(mk)::value>, dim3(bx, N), dim3(LS_THREADS), 0, s, logits, label_onehot, K, HW,
                       partial);
  });
  hipLaunchKernelGGL(dice_loss_finalize_kernel, dim3(1), dim3(64), 0, s, partial, bx, N, K, sums, loss);
  pp_prof_end(s);
  return pp_launch_status("dice_loss_fwd");
}

extern "C" int pp_dice_loss_bwd(const float* logits, const float* label_onehot, int N, int K, int HW, const double* sums,
                                const float* g, float grad_scale, float* dlogits, int accumulate, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && label_onehot && sums && dlogits && N >= 1 && K >= 1, "dice_loss_bwd: bad arguments");
  PP_CHECK_ARG(K <= PP_MAXK, "dice_loss_bwd: K=%d (1..%d)", K, PP_MAXK);
  int bx = pp_cdiv(HW, LS_THREADS);
  if (bx > 256) bx = 256;
  pp_prof_begin(PP_K_LOSS, 0.0, 12.0 * (double)N * K * HW, s);
  pp_by_class_bound(K, [&](auto mk) {
    hipLaunchKernelGGL(dice_loss_bwd_kernel<decltype(mk)::value>, dim3(bx, N), dim3(LS_THREADS), 0, s, logits, label_onehot, N, K, HW,
                       sums, g, grad_scale, dlogits, accumulate);
  });
  pp_prof_end(s);
  return pp_launch_status("dice_loss_bwd");
}

// ---------------------------------------------------------------- gated CRF / Potts regulariser on the weak-view logits
//   k_ij = exp(-(dy^2 + dx^2) / (2 sxy^2)) * exp(-|x_i - x_j|^2 / (2 srgb^2)),  j = i + (dy, dx) * d,  dy, dx in [-r, r] \ (0, 0)
//   L = (1/D) sum_i sum_j m_i m_j k_ij (1 - <p_i, p_j>),  D = N H W, or max(sum m, 1e-8) with a mask
// k and m_i m_j are symmetric, so the derivative is a gather: with G_ic = sum_j m_j k_ij p_jc and S_i = sum_j m_j k_ij pixel i
// adds m_i (S_i - <p_i, G_i>) to the numerator and dL/dz_ic = -(2/D) m_i p_ic (G_ic - <p_i, G_i>).
// Forward: a block of four waves owns a 64 x 4 tile (one wave per row, one pixel per lane) and stages tile + halo r*d into LDS,
// pixel-major with an odd row length (consecutive lanes -> distinct banks of ds_read_b32; compile-time offsets for the planes):
// soft-max probabilities of a chunk of KC classes (full-K normaliser, evaluated while staging), the image channels, the mask
// (0 outside the image: such a j contributes nothing).  Every lane then walks the (2r+1)^2 - 1 offsets.  Both factors of k go
// through ONE exp2: the spatial term (dy^2 + dx^2) * a_xy is uniform over the wave and seeds the exponent the channel differences
// are accumulated into, so no table is read in the loop.  K > KC runs in class chunks (restage, walk again, k recomputed); the
// LDS bound picks the chunk count, so every accepted (K, C, r, d) fits.  With `unit` the pass leaves u_ic = m_i p_ic (G_ic -
// <p_i, G_i>) for the streaming backward, which never repeats the walk.  Per block one double partial of the numerator and of
// sum m; crf_reduce_kernel adds them in a fixed order: the same bits run after run, no atomics.
#define CRF_TW 64
#define CRF_TH 4
#define CRF_THREADS (CRF_TW * CRF_TH)
#define CRF_MAXR 8
#define CRF_MAXD 4
#define CRF_MAXHALO 16
#define CRF_MAXC 4
#define CRF_KC 8                       // largest class chunk (= the K <= 8 bound of pp_by_class_bound)
#define CRF_LDS_MAX (160 * 1024 - 256)   // dynamic part; the block also holds 64 B of static partial sums

template <int KC, int CT>              // CT: image channels (1 or 3), 0: any count up to CRF_MAXC at run time
struct CrfLayout {
  static constexpr int NC = CT ? CT : CRF_MAXC;
  static constexpr int P = (KC + NC + 1) | 1;        // floats per staged pixel: [0, KC) p, [KC, KC + NC) x, [KC + NC] m
};
static inline size_t crf_lds_bytes(int P, int halo) {
  return (size_t)(CRF_TW + 2 * halo) * (CRF_TH + 2 * halo) * P * sizeof(float);
}

__device__ __forceinline__ void crf_softmax_norm(const float* __restrict__ zq, int K, int HW, float& mx, float& inv) {
  mx = -INFINITY;
  for (int k = 0; k < K; ++k) mx = fmaxf(mx, zq[(size_t)k * HW]);
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(zq[(size_t)k * HW] - mx);
  inv = 1.f / s;
}
__device__ __forceinline__ float crf_prob(float z, float mx, float inv) { return expf(z - mx) * inv; }

// Stage tile + halo of one class chunk [c0, c0 + KC) into LDS, P floats per pixel (CrfLayout); zeros outside the image: the staging
// loop of crf_fwd_kernel as a function, for the normalised-cut walk further down (crf_fwd_kernel keeps its own copy in line: called
// from there the compiler schedules that kernel differently, and its code is to stay what it was).
template <int KC, int CT>
__device__ __forceinline__ void crf_stage_tile(float* __restrict__ crf_lds, const float* __restrict__ zn, const float* __restrict__ xn,
                                               const float* __restrict__ mn, int K, int C, int H, int W, int R, int LW, int LH, int x0,
                                               int y0, int c0, int nchunks) {
  constexpr int NC = CrfLayout<KC, CT>::NC, P = CrfLayout<KC, CT>::P;
  const int HW = H * W;
  for (int s = threadIdx.x; s < LW * LH; s += CRF_THREADS) {
    const int sy = s / LW, sx = s - sy * LW;
    const int py = y0 - R + sy, px = x0 - R + sx;
    float* o = crf_lds + s * P;
    if (px >= 0 && px < W && py >= 0 && py < H) {
      const int sq = py * W + px;
      if (nchunks == 1) {                                        // K <= KC: one load per logit
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
        crf_softmax_norm(zn + sq, K, HW, mx, inv);
#pragma unroll
        for (int c = 0; c < KC; ++c) o[c] = c0 + c < K ? crf_prob(zn[(size_t)(c0 + c) * HW + sq], mx, inv) : 0.f;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) o[KC + c] = c < C ? xn[(size_t)c * HW + sq] : 0.f;
      o[KC + NC] = mn ? mn[sq] : 1.f;
    } else {
#pragma unroll
      for (int c = 0; c < KC + NC + 1; ++c) o[c] = 0.f;
    }
  }
}

template <int KC, int CT>
__global__ __launch_bounds__(CRF_THREADS) void crf_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ img, const float* __restrict__ mask, int K, int C, int H, int W, int r,
    int d, float a_xy, float a_rgb, int nchunks, float* __restrict__ unit, double* __restrict__ partial /*[blocks][2]*/) {
  extern __shared__ float crf_lds[];
  __shared__ double shd[2][CRF_TH];
  constexpr int NC = CrfLayout<KC, CT>::NC, P = CrfLayout<KC, CT>::P;
  const int R = r * d, LW = CRF_TW + 2 * R, LH = CRF_TH + 2 * R, HW = H * W;
  const int n = blockIdx.z, x0 = blockIdx.x * CRF_TW, y0 = blockIdx.y * CRF_TH;
  const float* zn = z + (size_t)n * K * HW;
  const float* xn = img + (size_t)n * C * HW;
  const float* mn = mask ? mask + (size_t)n * HW : nullptr;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int gx = x0 + lx, gy = y0 + ly, q = gy * W + gx;
  const bool inside = gx < W && gy < H;
  const float* ci = crf_lds + ((ly + R) * LW + lx + R) * P;      // this lane's own pixel
  float dot = 0.f, S = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int c0 = ch * KC;
    if (ch) __syncthreads();                                       // every lane is through with the previous chunk
    // (this staging loop has a twin, crf_stage_tile above: a change of the LDS layout goes into both)
    for (int s = threadIdx.x; s < LW * LH; s += CRF_THREADS) {
      const int sy = s / LW, sx = s - sy * LW;
      const int py = y0 - R + sy, px = x0 - R + sx;
      float* o = crf_lds + s * P;
      if (px >= 0 && px < W && py >= 0 && py < H) {
        const int sq = py * W + px;
        if (nchunks == 1) {                                        // K <= KC: one load per logit
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
          crf_softmax_norm(zn + sq, K, HW, mx, inv);
#pragma unroll
          for (int c = 0; c < KC; ++c) o[c] = c0 + c < K ? crf_prob(zn[(size_t)(c0 + c) * HW + sq], mx, inv) : 0.f;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) o[KC + c] = c < C ? xn[(size_t)c * HW + sq] : 0.f;
        o[KC + NC] = mn ? mn[sq] : 1.f;
      } else {
#pragma unroll
        for (int c = 0; c < KC + NC + 1; ++c) o[c] = 0.f;
      }
    }
    __syncthreads();
    float xi[NC], G[KC];
#pragma unroll
    for (int c = 0; c < NC; ++c) xi[c] = ci[KC + c];
#pragma unroll
    for (int c = 0; c < KC; ++c) G[c] = 0.f;
    float Sc = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const float* row = ci + dy * d * LW * P;
#pragma unroll 2
      for (int dx = -r; dx <= r; ++dx) {
        const float* cj = row + dx * d * P;
        float e = (float)(dy * dy + dx * dx) * a_xy;
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float t = xi[c] - cj[KC + c]; e = __builtin_fmaf(t * t, a_rgb, e); }
        const float k = __builtin_amdgcn_exp2f(e) * (cj[KC + NC] * ((dy | dx) ? 1.f : 0.f));      // (0, 0) is no neighbour: its mask times a uniform 0
        Sc += k;
#pragma unroll
        for (int c = 0; c < KC; ++c) G[c] = __builtin_fmaf(k, cj[c], G[c]);
      }
    }
    if (ch == 0) S = Sc;
#pragma unroll
    for (int c = 0; c < KC; ++c) dot = __builtin_fmaf(ci[c], G[c], dot);
    if (unit && inside) {
      float* un = unit + (size_t)n * K * HW + q;
      if (nchunks == 1) {
        const float mi = ci[KC + NC];
#pragma unroll
        for (int c = 0; c < KC; ++c) if (c < K) un[(size_t)c * HW] = mi * ci[c] * (G[c] - dot);
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) if (c0 + c < K) un[(size_t)(c0 + c) * HW] = G[c];      // finished below, once <p, G> is whole
      }
    }
  }
  const float mi = ci[KC + NC];
  if (unit && inside && nchunks > 1) {
    // same lane, same addresses as the stores above; the probabilities are the staged ones (one expression: crf_prob)
    float* un = unit + (size_t)n * K * HW + q;
    float mx, inv;
    crf_softmax_norm(zn + q, K, HW, mx, inv);
    for (int k = 0; k < K; ++k) un[(size_t)k * HW] = mi * crf_prob(zn[(size_t)k * HW + q], mx, inv) * (un[(size_t)k * HW] - dot);
  }
  double a = inside ? (double)(mi * (S - dot)) : 0.0, b = inside ? (double)mi : 0.0;
  a = pp_wave_sum_d(a);
  b = pp_wave_sum_d(b);
  if (lx == 0) { shd[0][ly] = a; shd[1][ly] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    o[0] = ((shd[0][0] + shd[0][1]) + shd[0][2]) + shd[0][3];
    o[1] = ((shd[1][0] + shd[1][1]) + shd[1][2]) + shd[1][3];
  }
}

// sums[0] = numerator, sums[1] = sum m (mask) or the pixel count: thread t adds blocks t, t + 256, ... in order, then the butterfly
__global__ __launch_bounds__(256) void crf_reduce_kernel(const double* __restrict__ partial, int nblocks, int has_mask,
                                                         double unmasked_den, double* __restrict__ sums) {
  __shared__ double sh[2][4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { a += partial[(size_t)i * 2]; b += partial[(size_t)i * 2 + 1]; }
  a = pp_wave_sum_d(a);
  b = pp_wave_sum_d(b);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  sums[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
  sums[1] = has_mask ? ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3] : unmasked_den;
}

// dlogits += grad_scale * g_up * (-2 / D) * u: 16-byte accesses, D read on the device (behind the cross-rank reduction of sums)
__global__ __launch_bounds__(LS_THREADS) void crf_bwd_kernel(const float* __restrict__ unit, const double* __restrict__ sums,
                                                             int has_mask, const float* __restrict__ g_up, float grad_scale,
                                                             float* __restrict__ dz, long long n, long long n4) {
  const double D = has_mask ? fmax(sums[1], 1e-8) : sums[1];
  const float f = (float)(-2.0 * (double)(*g_up * grad_scale) / D);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  for (long long i = t; i < n4; i += step) {
    const float4 u = reinterpret_cast<const float4*>(unit)[i];
    float4 g = reinterpret_cast<float4*>(dz)[i];
    g.x = __builtin_fmaf(f, u.x, g.x); g.y = __builtin_fmaf(f, u.y, g.y); g.z = __builtin_fmaf(f, u.z, g.z); g.w = __builtin_fmaf(f, u.w, g.w);
    reinterpret_cast<float4*>(dz)[i] = g;
  }
  for (long long i = n4 * 4 + t; i < n; i += step) dz[i] = __builtin_fmaf(f, unit[i], dz[i]);
}

static inline int crf_blocks(int N, int H, int W) { return N * pp_cdiv(H, CRF_TH) * pp_cdiv(W, CRF_TW); }

extern "C" size_t pp_crf_loss_workspace(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (size_t)crf_blocks(N, H, W) * 2 * sizeof(double);
}

extern "C" int pp_crf_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                               int radius, int dilation, float sigma_xy, float sigma_rgb, float* unit_grad, double* sums,
                               void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && image && sums && workspace, "crf_loss_fwd: null pointer");
  // (N and the rows of tiles are grid.z and grid.y: 65535 each)
  PP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 * CRF_TH && W >= 1 && (long long)H * W * K < 0x7fffffffLL,
               "crf_loss_fwd: N=%d (<= 65535) H=%d (<= %d) W=%d", N, H, 65535 * CRF_TH, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && C >= 1 && C <= CRF_MAXC, "crf_loss_fwd: K=%d (1..%d) C=%d (1..%d)", K, PP_MAXK, C, CRF_MAXC);
  PP_CHECK_ARG(radius >= 1 && radius <= CRF_MAXR && dilation >= 1 && dilation <= CRF_MAXD && radius * dilation <= CRF_MAXHALO,
               "crf_loss_fwd: radius=%d (1..%d) dilation=%d (1..%d), radius * dilation <= %d", radius, CRF_MAXR, dilation, CRF_MAXD, CRF_MAXHALO);
  PP_CHECK_ARG(sigma_xy > 0.f && sigma_rgb > 0.f && sigma_xy < INFINITY && sigma_rgb < INFINITY, "crf_loss_fwd: sigma_xy=%g sigma_rgb=%g (> 0)",
               (double)sigma_xy, (double)sigma_rgb);
  if (workspace_bytes < pp_crf_loss_workspace(N, H, W)) {
    pp_set_error("crf_loss_fwd: workspace too small (%zu < %zu)", workspace_bytes, pp_crf_loss_workspace(N, H, W));
    return PP_ERR_WORKSPACE;
  }
  const int halo = radius * dilation, NC = (C == 1 || C == 3) ? C : CRF_MAXC;
  // class chunks: as few as the LDS bound allows, of equal width (K = 9 -> 5 + 4, not 8 + 1)
  int nchunks = pp_cdiv(K, CRF_KC), KC = pp_cdiv(K, nchunks);
  while (crf_lds_bytes((KC + NC + 1) | 1, halo) > CRF_LDS_MAX) { ++nchunks; KC = pp_cdiv(K, nchunks); }
  nchunks = pp_cdiv(K, KC);
  const size_t lds = crf_lds_bytes((KC + NC + 1) | 1, halo);
  const double log2e = 1.4426950408889634;
  const float a_xy = (float)(-log2e / (2.0 * (double)sigma_xy * sigma_xy)), a_rgb = (float)(-log2e / (2.0 * (double)sigma_rgb * sigma_rgb));
  const dim3 grid(pp_cdiv(W, CRF_TW), pp_cdiv(H, CRF_TH), N);
  const int blocks = crf_blocks(N, H, W);
  const double P = (double)N * H * W, nb = (2.0 * radius + 1.0) * (2.0 * radius + 1.0) - 1.0;
  pp_prof_begin(PP_K_LOSS, P * nb * nchunks * (2.0 * KC + 3.0 * C + 4.0), P * (4.0 * K * (unit_grad ? 2 : 1) + 4.0 * C + 4.0), s);
#define CRF_LAUNCH(KC_, CT_)                                                                                                   \
  do {                                                                                                                           \
    auto kern = crf_fwd_kernel<KC_, CT_>;                                                                                        \
    pp_max_lds(reinterpret_cast<const void*>(kern), CRF_LDS_MAX);                                                                \
    hipLaunchKernelGGL(kern, grid, dim3(CRF_THREADS), lds, s, logits, image, valid_mask, K, C, H, W, radius, dilation, a_xy,     \
                       a_rgb, nchunks, unit_grad, (double*)workspace);                                                          \
  } while (0)
#define CRF_BY_C(KC_) do { if (C == 1) CRF_LAUNCH(KC_, 1); else if (C == 3) CRF_LAUNCH(KC_, 3); else CRF_LAUNCH(KC_, 0); } while (0)
  switch (KC) {
    case 1: CRF_BY_C(1); break;
    case 2: CRF_BY_C(2); break;
    case 3: CRF_BY_C(3); break;
    case 4: CRF_BY_C(4); break;
    case 5: CRF_BY_C(5); break;
    case 6: CRF_BY_C(6); break;
    case 7: CRF_BY_C(7); break;
    default: CRF_BY_C(8); break;
  }
#undef CRF_BY_C
#undef CRF_LAUNCH
  hipLaunchKernelGGL(crf_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, blocks, valid_mask ? 1 : 0, P, sums);
  pp_prof_end(s);
  return pp_launch_status("crf_loss_fwd");
}

extern "C" int pp_crf_loss_bwd(const float* unit_grad, const double* sums, int has_mask, const float* g_up, float grad_scale,
                               float* dlogits, long long n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(unit_grad && sums && g_up && dlogits && n >= 1, "crf_loss_bwd: bad arguments");
  const long long n4 = ((((uintptr_t)unit_grad | (uintptr_t)dlogits) & 15) == 0) ? n >> 2 : 0;
  pp_prof_begin(PP_K_LOSS, 2.0 * (double)n, 12.0 * (double)n, s);
  hipLaunchKernelGGL(crf_bwd_kernel, dim3(ls_blocks(n4 ? n4 : n, 8192)), dim3(LS_THREADS), 0, s, unit_grad, sums, has_mask, g_up, grad_scale,
                     dlogits, n, n4);
  pp_prof_end(s);
  return pp_launch_status("crf_loss_bwd");
}

// ---------------------------------------------------------------- normalised cut on the weak-view logits
//   q_ic = sum_j m_j k_ij p_jc,  d_i = sum_j m_j k_ij   (k, offsets and dilation exactly those of the gated-CRF loss above)
//   A_nc = sum_{i in n} m_i p_ic q_ic,  V_nc = sum_{i in n} m_i p_ic d_i,  NC_nc = 1 - A_nc / V_nc if V_nc > 1e-6, else 0
//   L = (1/D) sum_n sum_c NC_nc,  D = N K.  k and m_i m_j are symmetric, so the derivative is a gather once A and V exist:
//   G_ic = m_i (a_nc q_ic + b_nc d_i), a = -2 / V, b = A / V^2 (0 for an inactive class), dL/dz_ic = (1/D) p_ic (G_ic - <p_i, G_i>).
// Pass 1 (nc_fwd_kernel) is the CRF walk -- same tile, LDS layout, one-exp2 kernel and class chunks -- that parks q in `unit` and
// d in the workspace and leaves per-block double partials of m p q and m p d for every class.  nc_reduce_kernel adds the blocks of
// one image in a fixed order per (n, c); nc_final_kernel forms sum NC and the count, and the fp32 pair (a, b) per (n, c), each
// formed in double and rounded once.  Pass 2 (nc_grad_kernel) streams: soft-max again, u = p (G - <p, G>) over q in place.  No
// atomics: the same bits run after run.
#define NC_V_MIN 1e-6

template <int KC, int CT>
__global__ __launch_bounds__(CRF_THREADS) void nc_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ img, const float* __restrict__ mask, int K, int C, int H, int W, int r,
    int d, float a_xy, float a_rgb, int nchunks, float* __restrict__ qout /*(N,K,H,W) or null*/, float* __restrict__ dout /*(N,H,W)*/,
    double* __restrict__ partial /*[blocks][K][2]*/) {
  extern __shared__ float crf_lds[];
  constexpr int NC = CrfLayout<KC, CT>::NC, P = CrfLayout<KC, CT>::P;
  const int R = r * d, LW = CRF_TW + 2 * R, LH = CRF_TH + 2 * R, HW = H * W;
  const int n = blockIdx.z, x0 = blockIdx.x * CRF_TW, y0 = blockIdx.y * CRF_TH;
  const float* zn = z + (size_t)n * K * HW;
  const float* xn = img + (size_t)n * C * HW;
  const float* mn = mask ? mask + (size_t)n * HW : nullptr;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int gx = x0 + lx, gy = y0 + ly, q = gy * W + gx;
  const bool inside = gx < W && gy < H;
  const float* ci = crf_lds + ((ly + R) * LW + lx + R) * P;      // this lane's own pixel
  double* pb = partial + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * K * 2;
  double* shd = reinterpret_cast<double*>(crf_lds);               // [2 * KC][CRF_TH] wave sums, over the tile once the walk is through
  float S = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int c0 = ch * KC;
    if (ch) __syncthreads();                                       // the block sums of the previous chunk have been read
    crf_stage_tile<KC, CT>(crf_lds, zn, xn, mn, K, C, H, W, R, LW, LH, x0, y0, c0, nchunks);
    __syncthreads();
    float xi[NC], G[KC];
#pragma unroll
    for (int c = 0; c < NC; ++c) xi[c] = ci[KC + c];
#pragma unroll
    for (int c = 0; c < KC; ++c) G[c] = 0.f;
    float Sc = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const float* row = ci + dy * d * LW * P;
#pragma unroll 2
      for (int dx = -r; dx <= r; ++dx) {
        const float* cj = row + dx * d * P;
        float e = (float)(dy * dy + dx * dx) * a_xy;
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float t = xi[c] - cj[KC + c]; e = __builtin_fmaf(t * t, a_rgb, e); }
        const float k = __builtin_amdgcn_exp2f(e) * (cj[KC + NC] * ((dy | dx) ? 1.f : 0.f));      // (0, 0) is no neighbour: its mask times a uniform 0
        Sc += k;
#pragma unroll
        for (int c = 0; c < KC; ++c) G[c] = __builtin_fmaf(k, cj[c], G[c]);
      }
    }
    if (ch == 0) {
      S = Sc;                                                      // d_i: the same walk in every chunk, the first one's is kept
      if (qout && inside) dout[(size_t)n * HW + q] = S;
    }
    if (qout && inside) {
      float* qn = qout + (size_t)n * K * HW + q;
#pragma unroll
      for (int c = 0; c < KC; ++c) if (c0 + c < K) qn[(size_t)(c0 + c) * HW] = G[c];
    }
    const float mi = inside ? ci[KC + NC] : 0.f;
    double a[KC], v[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const float mp = mi * ci[c];
      a[c] = pp_wave_sum_d((double)(mp * G[c]));
      v[c] = pp_wave_sum_d((double)(mp * S));
    }
    __syncthreads();                                               // every lane is through with the tile: its head holds the wave sums now
    if (lx == 0) {
#pragma unroll
      for (int c = 0; c < KC; ++c) { shd[(2 * c) * CRF_TH + ly] = a[c]; shd[(2 * c + 1) * CRF_TH + ly] = v[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * KC && c0 + (threadIdx.x >> 1) < K) {
      const double* w = shd + threadIdx.x * CRF_TH;
      pb[(size_t)c0 * 2 + threadIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
  }
}

// assoc_vol[n][c] = {A, V}: block (n, c) adds that image's blocks, thread t blocks t, t + 256, ... in order, then the butterfly
__global__ __launch_bounds__(256) void nc_reduce_kernel(const double* __restrict__ partial, int bpi, int K, double* __restrict__ assoc_vol) {
  __shared__ double sh[2][4];
  const int n = blockIdx.x / K, c = blockIdx.x - n * K;
  const double* p = partial + ((size_t)n * bpi * K + c) * 2;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < bpi; i += 256) { a += p[(size_t)i * K * 2]; b += p[(size_t)i * K * 2 + 1]; }
  a = pp_wave_sum_d(a);
  b = pp_wave_sum_d(b);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  assoc_vol[(size_t)blockIdx.x * 2] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
  assoc_vol[(size_t)blockIdx.x * 2 + 1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
}

// sums[0] = sum NC_nc, sums[1] = N K (a count: exact); coef[n][c] = {a, b} = {-2 / V, A / V^2}, 0 for an inactive class
__global__ __launch_bounds__(256) void nc_final_kernel(const double* __restrict__ assoc_vol, int NK, float* __restrict__ coef,
                                                       double* __restrict__ sums) {
  __shared__ double sh[4];
  double t = 0.0;
  for (int i = threadIdx.x; i < NK; i += 256) {
    const double A = assoc_vol[(size_t)i * 2], V = assoc_vol[(size_t)i * 2 + 1];
    const bool active = V > NC_V_MIN;
    if (active) t += 1.0 - A / V;
    coef[(size_t)i * 2] = active ? (float)(-2.0 / V) : 0.f;
    coef[(size_t)i * 2 + 1] = active ? (float)(A / (V * V)) : 0.f;
  }
  t = pp_wave_sum_d(t);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x != 0) return;
  sums[0] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  sums[1] = (double)NK;
}

// u_ic = p_ic (G_ic - <p_i, G_i>), G_ic = m_i (a_nc q_ic + b_nc d_i), over q in place; V pixels per thread (4: 16-byte accesses)
template <int V>
__global__ __launch_bounds__(LS_THREADS) void nc_grad_kernel(const float* __restrict__ z, const float* __restrict__ mask,
                                                             const float* __restrict__ dws, const float* __restrict__ coef, int K, int HW,
                                                             float* __restrict__ unit) {
  struct alignas(4 * V) Vec { float f[V]; };
  const int n = blockIdx.y, i = blockIdx.x * LS_THREADS + threadIdx.x;
  if (i >= HW / V) return;
  const Vec* zn = reinterpret_cast<const Vec*>(z + (size_t)n * K * HW) + i;
  Vec* un = reinterpret_cast<Vec*>(unit + (size_t)n * K * HW) + i;
  const float* cf = coef + (size_t)n * K * 2;
  const int ld = HW / V;
  const Vec dv = reinterpret_cast<const Vec*>(dws + (size_t)n * HW)[i];
  Vec mv;
#pragma unroll
  for (int j = 0; j < V; ++j) mv.f[j] = 1.f;
  if (mask) mv = reinterpret_cast<const Vec*>(mask + (size_t)n * HW)[i];
  float mx[V], sum[V], dot[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { mx[j] = -INFINITY; sum[j] = 0.f; dot[j] = 0.f; }
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld];
#pragma unroll
    for (int j = 0; j < V; ++j) mx[j] = fmaxf(mx[j], v.f[j]);
  }
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld];
#pragma unroll
    for (int j = 0; j < V; ++j) sum[j] += expf(v.f[j] - mx[j]);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) sum[j] = 1.f / sum[j];
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld], qv = un[(size_t)k * ld];
    const float a = cf[2 * k], b = cf[2 * k + 1];
#pragma unroll
    for (int j = 0; j < V; ++j)
      dot[j] = __builtin_fmaf(crf_prob(v.f[j], mx[j], sum[j]), mv.f[j] * __builtin_fmaf(a, qv.f[j], b * dv.f[j]), dot[j]);
  }
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld], qv = un[(size_t)k * ld];
    const float a = cf[2 * k], b = cf[2 * k + 1];
    Vec o;
#pragma unroll
    for (int j = 0; j < V; ++j)
      o.f[j] = crf_prob(v.f[j], mx[j], sum[j]) * (mv.f[j] * __builtin_fmaf(a, qv.f[j], b * dv.f[j]) - dot[j]);
    un[(size_t)k * ld] = o;
  }
}

// dlogits += grad_scale * g_up / max(D, 1) * u: 16-byte accesses, D read on the device (behind the cross-rank reduction of sums)
__global__ __launch_bounds__(LS_THREADS) void nc_bwd_kernel(const float* __restrict__ unit, const double* __restrict__ sums,
                                                            const float* __restrict__ g_up, float grad_scale, float* __restrict__ dz,
                                                            long long n, long long n4) {
  const float f = (float)((double)(*g_up * grad_scale) / fmax(sums[1], 1.0));
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  for (long long i = t; i < n4; i += step) {
    const float4 u = reinterpret_cast<const float4*>(unit)[i];
    float4 g = reinterpret_cast<float4*>(dz)[i];
    g.x = __builtin_fmaf(f, u.x, g.x); g.y = __builtin_fmaf(f, u.y, g.y); g.z = __builtin_fmaf(f, u.z, g.z); g.w = __builtin_fmaf(f, u.w, g.w);
    reinterpret_cast<float4*>(dz)[i] = g;
  }
  for (long long i = n4 * 4 + t; i < n; i += step) dz[i] = __builtin_fmaf(f, unit[i], dz[i]);
}

// workspace: [blocks][K][2] double partials | [N][K][2] float (a, b), padded to 16 bytes | [N][H][W] float d
static inline size_t nc_partial_bytes(int N, int K, int H, int W) { return (size_t)crf_blocks(N, H, W) * K * 2 * sizeof(double); }
static inline size_t nc_coef_bytes(int N, int K) { return ((size_t)N * K * 2 * sizeof(float) + 15) & ~(size_t)15; }

extern "C" size_t pp_nc_loss_workspace(int N, int K, int H, int W) {
  if (N < 1 || K < 1 || H < 1 || W < 1) return 0;
  return nc_partial_bytes(N, K, H, W) + nc_coef_bytes(N, K) + (size_t)N * H * W * sizeof(float);
}

extern "C" int pp_nc_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                              int radius, int dilation, float sigma_xy, float sigma_rgb, float* unit_grad, double* assoc_vol,
                              double* sums, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && image && assoc_vol && sums && workspace, "nc_loss_fwd: null pointer");
  // (N and the rows of tiles are grid.z and grid.y: 65535 each)
  PP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 * CRF_TH && W >= 1 && (long long)H * W * K < 0x7fffffffLL,
               "nc_loss_fwd: N=%d (<= 65535) H=%d (<= %d) W=%d", N, H, 65535 * CRF_TH, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && C >= 1 && C <= CRF_MAXC, "nc_loss_fwd: K=%d (1..%d) C=%d (1..%d)", K, PP_MAXK, C, CRF_MAXC);
  PP_CHECK_ARG(radius >= 1 && radius <= CRF_MAXR && dilation >= 1 && dilation <= CRF_MAXD && radius * dilation <= CRF_MAXHALO,
               "nc_loss_fwd: radius=%d (1..%d) dilation=%d (1..%d), radius * dilation <= %d", radius, CRF_MAXR, dilation, CRF_MAXD, CRF_MAXHALO);
  PP_CHECK_ARG(sigma_xy > 0.f && sigma_rgb > 0.f && sigma_xy < INFINITY && sigma_rgb < INFINITY, "nc_loss_fwd: sigma_xy=%g sigma_rgb=%g (> 0)",
               (double)sigma_xy, (double)sigma_rgb);
  PP_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "nc_loss_fwd: the workspace must be 16-byte aligned");
  if (workspace_bytes < pp_nc_loss_workspace(N, K, H, W)) {
    pp_set_error("nc_loss_fwd: workspace too small (%zu < %zu)", workspace_bytes, pp_nc_loss_workspace(N, K, H, W));
    return PP_ERR_WORKSPACE;
  }
  const int halo = radius * dilation, NC = (C == 1 || C == 3) ? C : CRF_MAXC;
  // class chunks: as few as the LDS bound allows, of equal width (as pp_crf_loss_fwd)
  int nchunks = pp_cdiv(K, CRF_KC), KC = pp_cdiv(K, nchunks);
  while (crf_lds_bytes((KC + NC + 1) | 1, halo) > CRF_LDS_MAX) { ++nchunks; KC = pp_cdiv(K, nchunks); }
  nchunks = pp_cdiv(K, KC);
  const size_t lds = crf_lds_bytes((KC + NC + 1) | 1, halo);
  const double log2e = 1.4426950408889634;
  const float a_xy = (float)(-log2e / (2.0 * (double)sigma_xy * sigma_xy)), a_rgb = (float)(-log2e / (2.0 * (double)sigma_rgb * sigma_rgb));
  const dim3 grid(pp_cdiv(W, CRF_TW), pp_cdiv(H, CRF_TH), N);
  const int bpi = pp_cdiv(W, CRF_TW) * pp_cdiv(H, CRF_TH), HW = H * W;
  double* partial = (double*)workspace;
  float* coef = (float*)((char*)workspace + nc_partial_bytes(N, K, H, W));
  float* dws = (float*)((char*)coef + nc_coef_bytes(N, K));
  const double P = (double)N * H * W, nb = (2.0 * radius + 1.0) * (2.0 * radius + 1.0) - 1.0;
  pp_prof_begin(PP_K_LOSS, P * nb * nchunks * (2.0 * KC + 3.0 * C + 4.0), P * (4.0 * K * (unit_grad ? 4 : 1) + 4.0 * C + 4.0), s);
#define NC_LAUNCH(KC_, CT_)                                                                                                    \
  do {                                                                                                                           \
    auto kern = nc_fwd_kernel<KC_, CT_>;                                                                                         \
    pp_max_lds(reinterpret_cast<const void*>(kern), CRF_LDS_MAX);                                                                \
    hipLaunchKernelGGL(kern, grid, dim3(CRF_THREADS), lds, s, logits, image, valid_mask, K, C, H, W, radius, dilation, a_xy,     \
                       a_rgb, nchunks, unit_grad, dws, partial);                                                                \
  } while (0)
#define NC_BY_C(KC_) do { if (C == 1) NC_LAUNCH(KC_, 1); else if (C == 3) NC_LAUNCH(KC_, 3); else NC_LAUNCH(KC_, 0); } while (0)
  switch (KC) {
    case 1: NC_BY_C(1); break;
    case 2: NC_BY_C(2); break;
    case 3: NC_BY_C(3); break;
    case 4: NC_BY_C(4); break;
    case 5: NC_BY_C(5); break;
    case 6: NC_BY_C(6); break;
    case 7: NC_BY_C(7); break;
    default: NC_BY_C(8); break;
  }
#undef NC_BY_C
#undef NC_LAUNCH
  hipLaunchKernelGGL(nc_reduce_kernel, dim3(N * K), dim3(256), 0, s, (const double*)partial, bpi, K, assoc_vol);
  hipLaunchKernelGGL(nc_final_kernel, dim3(1), dim3(256), 0, s, (const double*)assoc_vol, N * K, coef, sums);
  if (unit_grad) {
    const bool v4 = (HW & 3) == 0 && ((((uintptr_t)logits | (uintptr_t)unit_grad | (uintptr_t)valid_mask) & 15) == 0);
    if (v4)
      hipLaunchKernelGGL(nc_grad_kernel<4>, dim3(pp_cdiv(HW / 4, LS_THREADS), N), dim3(LS_THREADS), 0, s, logits, valid_mask,
                         (const float*)dws, (const float*)coef, K, HW, unit_grad);
    else
      hipLaunchKernelGGL(nc_grad_kernel<1>, dim3(pp_cdiv(HW, LS_THREADS), N), dim3(LS_THREADS), 0, s, logits, valid_mask,
                         (const float*)dws, (const float*)coef, K, HW, unit_grad);
  }
  pp_prof_end(s);
  return pp_launch_status("nc_loss_fwd");
}

extern "C" int pp_nc_loss_bwd(const float* unit_grad, const double* sums, const float* g_up, float grad_scale, float* dlogits,
                              long long n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(unit_grad && sums && g_up && dlogits && n >= 1, "nc_loss_bwd: bad arguments");
  const long long n4 = ((((uintptr_t)unit_grad | (uintptr_t)dlogits) & 15) == 0) ? n >> 2 : 0;
  pp_prof_begin(PP_K_LOSS, 2.0 * (double)n, 12.0 * (double)n, s);
  hipLaunchKernelGGL(nc_bwd_kernel, dim3(ls_blocks(n4 ? n4 : n, 8192)), dim3(LS_THREADS), 0, s, unit_grad, sums, g_up, grad_scale, dlogits,
                     n, n4);
  pp_prof_end(s);
  return pp_launch_status("nc_loss_bwd");
}

// ---------------------------------------------------------------- Mumford-Shah level-set loss on the weak-view logits
//   S_nc = sum_i m_i p_ic,  mu_ncr = sum_i m_i p_ic x_ir / S_nc if S_nc > 1e-6 (else the class is inactive in that image),
//   e_ic = sum_r (x_ir - mu_ncr)^2,  E_ls = sum_nci m_i p_ic e_ic [active],  E_tv = sum_nc sum_(i,j) m_i m_j |p_ic - p_jc| over the
//   vertical and horizontal neighbour pairs inside the image (each once),  L = (E_ls + lambda E_tv) / D,  D = N H W, or
//   max(sum m, 1e-8) with a mask.  mu is the m p-weighted mean, so the derivative through mu vanishes:
//   g_ic = m_i e_ic [active] + lambda sum_{j in 4-neighbours} m_i m_j sign(p_ic - p_jc),  dL/dz_ic = (1/D) p_ic (g_ic - <p_i, g_i>).
// ms_sums_kernel streams logits, image and mask once (V pixels per thread) and leaves one double partial of S and of every X_r per
// (block, class); blocks never straddle an image.  ms_stats_kernel adds the blocks of one image in a fixed order per (n, c) into
// stats[n][c] = {S, mu_0 .. mu_{C-1}} (double) and the fp32 copy {active, mu_r} the next pass reads (formed in double, rounded once).
// ms_energy_kernel owns a 32 x 8 tile: it stages the probabilities of ALL K classes and the mask of tile + a one-pixel halo in LDS,
// class-major (m = 0 outside the image: such a neighbour adds nothing), every staged pixel through the one expression crf_prob
// behind crf_softmax_norm -- a pixel's probabilities are the same bits in a tile's interior, in a halo and in the next tile, so
// sign() and |.| see a difference only where there is one.  Each lane then walks the classes of its pixel twice over LDS with
// nothing but scalars live (energy and <p, g>; then u = p (g - <p, g>)): no class array in registers at any K.  Per block one double
// partial of the energy and of sum m; crf_reduce_kernel adds them in a fixed order.  No atomics: the same bits run after run.
#define MS_S_MIN 1e-6
#define MS_TW 32
#define MS_TH 8
#define MS_THREADS (MS_TW * MS_TH)
#define MS_LW (MS_TW + 2)
#define MS_LH (MS_TH + 2)
#define MS_NSTAT (1 + CRF_MAXC)                       // floats per (n, c) of the fp32 copy: active flag, mu_0 .. mu_3

template <int V>
__global__ __launch_bounds__(LS_THREADS) void ms_sums_kernel(const float* __restrict__ z, const float* __restrict__ img,
                                                             const float* __restrict__ mask, int K, int C, int HW,
                                                             double* __restrict__ partial /*[N][gridDim.x][K][1 + C]*/) {
  struct alignas(4 * V) Vec { float f[V]; };
  __shared__ double sh[PP_MAXK * MS_NSTAT][LS_THREADS / 64];
  const int n = blockIdx.y, ld = HW / V, i0 = blockIdx.x * LS_THREADS + threadIdx.x;
  const bool on = i0 < ld;
  const int i = on ? i0 : ld - 1;                    // lanes past the image read its last group and weigh it 0
  const Vec* zn = reinterpret_cast<const Vec*>(z + (size_t)n * K * HW) + i;
  const Vec* xn = reinterpret_cast<const Vec*>(img + (size_t)n * C * HW) + i;
  Vec mv, xv[CRF_MAXC];
#pragma unroll
  for (int j = 0; j < V; ++j) mv.f[j] = 1.f;
  if (mask) mv = reinterpret_cast<const Vec*>(mask + (size_t)n * HW)[i];
  if (!on) {
#pragma unroll
    for (int j = 0; j < V; ++j) mv.f[j] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < CRF_MAXC; ++r) {
    if (r < C) xv[r] = xn[(size_t)r * ld];
    else {
#pragma unroll
      for (int j = 0; j < V; ++j) xv[r].f[j] = 0.f;
    }
  }
  float mx[V], inv[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { mx[j] = -INFINITY; inv[j] = 0.f; }
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld];
#pragma unroll
    for (int j = 0; j < V; ++j) mx[j] = fmaxf(mx[j], v.f[j]);
  }
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld];
#pragma unroll
    for (int j = 0; j < V; ++j) inv[j] += expf(v.f[j] - mx[j]);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) inv[j] = 1.f / inv[j];
  const int wave = threadIdx.x >> 6, nq = 1 + C;
  for (int k = 0; k < K; ++k) {
    const Vec v = zn[(size_t)k * ld];
    double a[MS_NSTAT];
#pragma unroll
    for (int r = 0; r < MS_NSTAT; ++r) a[r] = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double w = (double)(mv.f[j] * crf_prob(v.f[j], mx[j], inv[j]));
      a[0] += w;
#pragma unroll
      for (int r = 0; r < CRF_MAXC; ++r) a[1 + r] += w * (double)xv[r].f[j];
    }
#pragma unroll
    for (int r = 0; r < MS_NSTAT; ++r) {
      if (r < nq) {                                  // (uniform)
        const double t = pp_wave_sum_d(a[r]);
        if ((threadIdx.x & 63) == 0) sh[k * nq + r][wave] = t;
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K * nq) {
    const double* w = sh[threadIdx.x];
    partial[((size_t)n * gridDim.x + blockIdx.x) * K * nq + threadIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

// stats[n][c] = {S, mu_0 .. mu_{C-1}} and statf[n][c] = {active, mu_0 .. mu_3}: block (n, c) adds that image's blocks, thread t
// blocks t, t + 256, ... in order, then the butterfly -- one quantity after the other
__global__ __launch_bounds__(256) void ms_stats_kernel(const double* __restrict__ partial, int bpi, int K, int C,
                                                       double* __restrict__ stats, float* __restrict__ statf) {
  __shared__ double sh[MS_NSTAT][4];
  const int n = blockIdx.x / K, c = blockIdx.x - n * K, nq = 1 + C;
  const double* p = partial + ((size_t)n * bpi * K + c) * nq;
  for (int r = 0; r < nq; ++r) {
    double a = 0.0;
    for (int i = threadIdx.x; i < bpi; i += 256) a += p[(size_t)i * K * nq + r];
    a = pp_wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) sh[r][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double S = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
  const bool active = S > MS_S_MIN;
  double* o = stats + (size_t)blockIdx.x * nq;
  float* of = statf + (size_t)blockIdx.x * MS_NSTAT;
  o[0] = S;
  of[0] = active ? 1.f : 0.f;
  for (int r = 0; r < CRF_MAXC; ++r) {
    double mu = 0.0;
    if (r < C && active) mu = (((sh[1 + r][0] + sh[1 + r][1]) + sh[1 + r][2]) + sh[1 + r][3]) / S;
    if (r < C) o[1 + r] = mu;
    of[1 + r] = (float)mu;
  }
}

__device__ __forceinline__ float ms_sign(float a, float b) { return (a > b ? 1.f : 0.f) - (a < b ? 1.f : 0.f); }

__global__ __launch_bounds__(MS_THREADS) void ms_energy_kernel(const float* __restrict__ z, const float* __restrict__ img,
                                                               const float* __restrict__ mask, const float* __restrict__ statf,
                                                               int K, int C, int H, int W, float lambda,
                                                               float* __restrict__ unit /*(N,K,H,W) or null*/,
                                                               double* __restrict__ partial /*[blocks][2]*/) {
  extern __shared__ float ms_lds[];                  // [K + 1][MS_LH][MS_LW]: the classes' probabilities, then the mask
  __shared__ double shd[2][MS_THREADS / 64];
  constexpr int PL = MS_LH * MS_LW;
  const int HW = H * W, n = blockIdx.z, x0 = blockIdx.x * MS_TW, y0 = blockIdx.y * MS_TH;
  const float* zn = z + (size_t)n * K * HW;
  const float* mn = mask ? mask + (size_t)n * HW : nullptr;
  for (int s = threadIdx.x; s < PL; s += MS_THREADS) {
    const int sy = s / MS_LW, sx = s - sy * MS_LW;
    const int py = y0 - 1 + sy, px = x0 - 1 + sx;
    if (px >= 0 && px < W && py >= 0 && py < H) {
      const int sq = py * W + px;
      float mx, inv;
      crf_softmax_norm(zn + sq, K, HW, mx, inv);
      for (int c = 0; c < K; ++c) ms_lds[c * PL + s] = crf_prob(zn[(size_t)c * HW + sq], mx, inv);
      ms_lds[K * PL + s] = mn ? mn[sq] : 1.f;
    } else {
      for (int c = 0; c <= K; ++c) ms_lds[c * PL + s] = 0.f;
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & (MS_TW - 1), ly = threadIdx.x / MS_TW;
  const int gx = x0 + lx, gy = y0 + ly;
  const bool inside = gx < W && gy < H;
  const int q = inside ? gy * W + gx : 0;
  const int ls = (ly + 1) * MS_LW + lx + 1;
  const float* ml = ms_lds + K * PL;
  // (0 outside the image, so a lane outside the image adds nothing and a neighbour outside it neither)
  const float mi = ml[ls];
  const float wl = mi * ml[ls - 1], wr = mi * ml[ls + 1], wu = mi * ml[ls - MS_LW], wd = mi * ml[ls + MS_LW];
  float xi[CRF_MAXC];
#pragma unroll
  for (int r = 0; r < CRF_MAXC; ++r) xi[r] = (r < C && inside) ? img[((size_t)n * C + r) * HW + q] : 0.f;
  const float* sf = statf + (size_t)n * K * MS_NSTAT;
  float en = 0.f, dot = 0.f;
  for (int c = 0; c < K; ++c) {
    const float* pl = ms_lds + c * PL + ls;
    const float p = pl[0], pL = pl[-1], pR = pl[1], pU = pl[-MS_LW], pD = pl[MS_LW];
    float e = 0.f;
#pragma unroll
    for (int r = 0; r < CRF_MAXC; ++r) { const float t = xi[r] - sf[c * MS_NSTAT + 1 + r]; e = __builtin_fmaf(t, t, e); }
    e *= mi * sf[c * MS_NSTAT];
    const float t = (wl * ms_sign(p, pL) + wr * ms_sign(p, pR)) + (wu * ms_sign(p, pU) + wd * ms_sign(p, pD));
    const float g = __builtin_fmaf(lambda, t, e);
    dot = __builtin_fmaf(p, g, dot);
    en += p * e + lambda * (wr * fabsf(p - pR) + wd * fabsf(p - pD));
  }
  if (unit && inside) {
    float* un = unit + (size_t)n * K * HW + q;
    for (int c = 0; c < K; ++c) {
      const float* pl = ms_lds + c * PL + ls;
      const float p = pl[0], pL = pl[-1], pR = pl[1], pU = pl[-MS_LW], pD = pl[MS_LW];
      float e = 0.f;
#pragma unroll
      for (int r = 0; r < CRF_MAXC; ++r) { const float t = xi[r] - sf[c * MS_NSTAT + 1 + r]; e = __builtin_fmaf(t, t, e); }
      e *= mi * sf[c * MS_NSTAT];
      const float t = (wl * ms_sign(p, pL) + wr * ms_sign(p, pR)) + (wu * ms_sign(p, pU) + wd * ms_sign(p, pD));
      un[(size_t)c * HW] = p * (__builtin_fmaf(lambda, t, e) - dot);
    }
  }
  double a = pp_wave_sum_d((double)en), b = pp_wave_sum_d((double)mi);
  if ((threadIdx.x & 63) == 0) { shd[0][threadIdx.x >> 6] = a; shd[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    o[0] = ((shd[0][0] + shd[0][1]) + shd[0][2]) + shd[0][3];
    o[1] = ((shd[1][0] + shd[1][1]) + shd[1][2]) + shd[1][3];
  }
}

// dlogits += grad_scale * g_up / D * u: 16-byte accesses, D read on the device (behind the cross-rank reduction of sums)
__global__ __launch_bounds__(LS_THREADS) void ms_bwd_kernel(const float* __restrict__ unit, const double* __restrict__ sums,
                                                            int has_mask, const float* __restrict__ g_up, float grad_scale,
                                                            float* __restrict__ dz, long long n, long long n4) {
  const double D = has_mask ? fmax(sums[1], 1e-8) : sums[1];
  const float f = (float)((double)(*g_up * grad_scale) / D);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  for (long long i = t; i < n4; i += step) {
    const float4 u = reinterpret_cast<const float4*>(unit)[i];
    float4 g = reinterpret_cast<float4*>(dz)[i];
    g.x = __builtin_fmaf(f, u.x, g.x); g.y = __builtin_fmaf(f, u.y, g.y); g.z = __builtin_fmaf(f, u.z, g.z); g.w = __builtin_fmaf(f, u.w, g.w);
    reinterpret_cast<float4*>(dz)[i] = g;
  }
  for (long long i = n4 * 4 + t; i < n; i += step) dz[i] = __builtin_fmaf(f, unit[i], dz[i]);
}

// workspace: [N][bpi][K][1 + C] double partials of the sums pass | [tiles][2] double partials of the energy pass |
// [N][K][MS_NSTAT] float {active, mu}; bpi: blocks per image of the sums pass at ONE pixel per thread (the four-pixel form needs fewer)
static inline int ms_bpi(int H, int W) { return pp_cdiv((long long)H * W, LS_THREADS); }
static inline int ms_tiles(int N, int H, int W) { return N * pp_cdiv(H, MS_TH) * pp_cdiv(W, MS_TW); }
static inline size_t ms_sums_bytes(int N, int K, int C, int H, int W) { return (size_t)N * ms_bpi(H, W) * K * (1 + C) * sizeof(double); }

extern "C" size_t pp_ms_loss_workspace(int N, int K, int C, int H, int W) {
  if (N < 1 || K < 1 || C < 1 || H < 1 || W < 1) return 0;
  return ms_sums_bytes(N, K, C, H, W) + (size_t)ms_tiles(N, H, W) * 2 * sizeof(double) + (size_t)N * K * MS_NSTAT * sizeof(float);
}

extern "C" int pp_ms_loss_fwd(const float* logits, const float* image, const float* valid_mask, int N, int K, int C, int H, int W,
                              float tv_weight, float* unit_grad, double* stats, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(logits && image && stats && sums && workspace, "ms_loss_fwd: null pointer");
  // (N is grid.y of the sums pass and grid.z of the energy pass, the rows of tiles are its grid.y: 65535 each)
  PP_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 * MS_TH && W >= 1 && (long long)H * W * K < 0x7fffffffLL,
               "ms_loss_fwd: N=%d (<= 65535) H=%d (<= %d) W=%d", N, H, 65535 * MS_TH, W);
  PP_CHECK_ARG(K >= 1 && K <= PP_MAXK && C >= 1 && C <= CRF_MAXC, "ms_loss_fwd: K=%d (1..%d) C=%d (1..%d)", K, PP_MAXK, C, CRF_MAXC);
  PP_CHECK_ARG(tv_weight >= 0.f && tv_weight < INFINITY, "ms_loss_fwd: tv_weight=%g (>= 0, finite)", (double)tv_weight);
  PP_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ms_loss_fwd: the workspace must be 16-byte aligned");
  if (workspace_bytes < pp_ms_loss_workspace(N, K, C, H, W)) {
    pp_set_error("ms_loss_fwd: workspace too small (%zu < %zu)", workspace_bytes, pp_ms_loss_workspace(N, K, C, H, W));
    return PP_ERR_WORKSPACE;
  }
  const int HW = H * W, tiles = ms_tiles(N, H, W);
  double* part_s = (double*)workspace;
  double* part_e = (double*)((char*)workspace + ms_sums_bytes(N, K, C, H, W));
  float* statf = (float*)(part_e + (size_t)tiles * 2);
  const double P = (double)N * HW;
  pp_prof_begin(PP_K_LOSS, P * K * (60.0 + 4.0 * C), P * (4.0 * K * (unit_grad ? 3 : 2) + 8.0 * C + 8.0), s);
  const bool v4 = (HW & 3) == 0 && ((((uintptr_t)logits | (uintptr_t)image | (uintptr_t)valid_mask) & 15) == 0);
  const int bpi = v4 ? pp_cdiv(HW / 4, LS_THREADS) : ms_bpi(H, W);
  if (v4)
    hipLaunchKernelGGL(ms_sums_kernel<4>, dim3(bpi, N), dim3(LS_THREADS), 0, s, logits, image, valid_mask, K, C, HW, part_s);
  else
    hipLaunchKernelGGL(ms_sums_kernel<1>, dim3(bpi, N), dim3(LS_THREADS), 0, s, logits, image, valid_mask, K, C, HW, part_s);
  hipLaunchKernelGGL(ms_stats_kernel, dim3(N * K), dim3(256), 0, s, (const double*)part_s, bpi, K, C, stats, statf);
  hipLaunchKernelGGL(ms_energy_kernel, dim3(pp_cdiv(W, MS_TW), pp_cdiv(H, MS_TH), N), dim3(MS_THREADS),
                     (size_t)(K + 1) * MS_LH * MS_LW * sizeof(float), s, logits, image, valid_mask, (const float*)statf, K, C, H, W,
                     tv_weight, unit_grad, part_e);
  hipLaunchKernelGGL(crf_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)part_e, tiles, valid_mask ? 1 : 0, P, sums);
  pp_prof_end(s);
  return pp_launch_status("ms_loss_fwd");
}

extern "C" int pp_ms_loss_bwd(const float* unit_grad, const double* sums, int has_mask, const float* g_up, float grad_scale,
                              float* dlogits, long long n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(unit_grad && sums && g_up && dlogits && n >= 1, "ms_loss_bwd: bad arguments");
  const long long n4 = ((((uintptr_t)unit_grad | (uintptr_t)dlogits) & 15) == 0) ? n >> 2 : 0;
  pp_prof_begin(PP_K_LOSS, 2.0 * (double)n, 12.0 * (double)n, s);
  hipLaunchKernelGGL(ms_bwd_kernel, dim3(ls_blocks(n4 ? n4 : n, 8192)), dim3(LS_THREADS), 0, s, unit_grad, sums, has_mask, g_up, grad_scale,
                     dlogits, n, n4);
  pp_prof_end(s);
  return pp_launch_status("ms_loss_bwd");
}

// ---------------------------------------------------------------- 95 % Hausdorff distance (inference.py:217-237)
// The reference calls medpy.metric.binary.hd95(pred == k, label == k, spacing, connectivity 1): the surface of a mask is
// mask XOR erode(mask, 4-neighbourhood cross, outside = background); each directed set is the Euclidean distance (in
// units of the pixel spacing) from every surface pixel of one mask to the nearest surface pixel of the other, and the
// metric is the 95th percentile of both sets together.  Per (image, class): one block compacts the two surfaces into
// coordinate lists (row-major order: the distance sets come out in the same order in every run), then every surface pixel scans
// the other list staged through LDS.  dist: [N][K][2][cap] floats, counts: [N][K][4] = {surface a, surface b, |a|, |b|}.
#define HD_THREADS 256
__global__ __launch_bounds__(HD_THREADS) void hd_surface_kernel(const long long* __restrict__ pred, const long long* __restrict__ label,
                                                                int K, int H, int W, int cap, int* __restrict__ coords,
                                                                int* __restrict__ counts) {
  const int n = blockIdx.x / K, k = blockIdx.x % K;
  const long long* A = pred + (size_t)n * H * W;
  const long long* B = label + (size_t)n * H * W;
  int* ca = coords + ((size_t)blockIdx.x * 2 + 0) * cap;
  int* cb = coords + ((size_t)blockIdx.x * 2 + 1) * cap;
  int* cnt = counts + (size_t)blockIdx.x * 4;
  // Ordered compaction: the lists hold the surface pixels in row-major order whatever the waves' schedule (ballot + population
  // count inside a wave, the waves' totals through LDS).  An append through an LDS counter gave the same SET in an order that
  // changed from run to run; pp_surface_reduce adds the distances in storage order, so its sums inherit the order.
  __shared__ int wa[HD_THREADS / 64], wb[HD_THREADS / 64];
  __shared__ int ta, tb;
  if (threadIdx.x == 0) { ta = 0; tb = 0; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  int na = 0, nb = 0;                                           // list lengths so far: the same in every thread
  int my_ta = 0, my_tb = 0;
  for (int p0 = 0; p0 < H * W; p0 += HD_THREADS) {              // uniform trip count: the barriers below are reached by all
    const int p = p0 + threadIdx.x;
    bool sa = false, sb = false;
    if (p < H * W) {
      const int y = p / W, x = p % W;
      const bool a = A[p] == k, b = B[p] == k;
      const bool border = !(y > 0 && y < H - 1 && x > 0 && x < W - 1);
      my_ta += a; my_tb += b;
      sa = a && (border || !(A[p - W] == k && A[p + W] == k && A[p - 1] == k && A[p + 1] == k));
      sb = b && (border || !(B[p - W] == k && B[p + W] == k && B[p - 1] == k && B[p + 1] == k));
    }
    const unsigned long long ma = __ballot(sa), mb = __ballot(sb);
    if (lane == 0) { wa[wave] = __popcll(ma); wb[wave] = __popcll(mb); }
    __syncthreads();
    int oa = na, ob = nb;
#pragma unroll
    for (int q = 0; q < HD_THREADS / 64; ++q) {
      if (q < wave) { oa += wa[q]; ob += wb[q]; }
      na += wa[q]; nb += wb[q];
    }
    if (sa) { const int i = oa + __popcll(ma & lt_mask); if (i < cap) ca[i] = p; }
    if (sb) { const int i = ob + __popcll(mb & lt_mask); if (i < cap) cb[i] = p; }
    __syncthreads();                                            // wa / wb are rewritten by the next trip
  }
  atomicAdd(&ta, my_ta);                                        // integer: order independent
  atomicAdd(&tb, my_tb);
  __syncthreads();
  if (threadIdx.x == 0) { cnt[0] = na; cnt[1] = nb; cnt[2] = ta; cnt[3] = tb; }
}

__global__ __launch_bounds__(HD_THREADS) void hd_distance_kernel(const int* __restrict__ coords, const int* __restrict__ counts,
                                                                 int W, int cap, float sy, float sx, float* __restrict__ dist) {
  __shared__ int tile[HD_THREADS];
  const int item = blockIdx.x, dir = blockIdx.y;             // dir 0: a -> b, 1: b -> a
  const int* cnt = counts + (size_t)item * 4;
  const int n_from = min(cnt[dir], cap), n_to = min(cnt[1 - dir], cap);
  const int* from = coords + ((size_t)item * 2 + dir) * cap;
  const int* to = coords + ((size_t)item * 2 + (1 - dir)) * cap;
  float* out = dist + ((size_t)item * 2 + dir) * cap;
  for (int base = 0; base < n_from; base += HD_THREADS) {
    const int i = base + threadIdx.x;
    const int p = i < n_from ? from[i] : 0;
    const int py = p / W, px = p % W;            // integer offsets first: coincident pixels give exactly 0
    float best = 3.0e38f;
    for (int t0 = 0; t0 < n_to; t0 += HD_THREADS) {
      __syncthreads();
      if (t0 + threadIdx.x < n_to) tile[threadIdx.x] = to[t0 + threadIdx.x];
      __syncthreads();
      const int m = min(HD_THREADS, n_to - t0);
      for (int j = 0; j < m; ++j) {
        const int q = tile[j];
        const float dy = (float)(q / W - py) * sy, dx = (float)(q % W - px) * sx;
        best = fminf(best, dy * dy + dx * dx);
      }
    }
    if (i < n_from) out[i] = sqrtf(best);
  }
}

// ---- loss assembly (train_chaos.py:273-310): total = t0 * w0 + t1 * w1 + ... of 0-dim device losses, one launch ----
// The Python form is eight element-wise launches forward and five backward on 0-dim tensors, ~6 us each behind one another on
// the stream between the forward and the backward pass.  Same arithmetic as that chain: every product and every sum rounded to
// fp32, left to right (no fused multiply-add).
struct WSumArgs { const float* t[8]; float w[8]; int n; };
__global__ void weighted_sum_fwd_kernel(WSumArgs a, float* out) {
#pragma clang fp contract(off)                      // (hipcc contracts a * b + c by default: __fmul_rn / __fadd_rn are plain operators)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float acc = a.t[0][0] * a.w[0];
  for (int i = 1; i < a.n; ++i) {
    const float prod = a.t[i][0] * a.w[i];
    acc = acc + prod;
  }
  out[0] = acc;
}
__global__ void weighted_sum_bwd_kernel(const float* g, WSumArgs a, float* gout) {
  const int i = threadIdx.x;
  if (i < a.n) gout[i] = __fmul_rn(g[0], a.w[i]);
}
extern "C" int pp_weighted_sum_fwd(const float* const* terms, const float* weights, int n, float* out, void* stream) {
  PP_CHECK_ARG(terms && weights && out && n >= 1 && n <= 8, "weighted_sum_fwd: 1..8 terms");
  WSumArgs a;
  for (int i = 0; i < 8; ++i) { a.t[i] = i < n ? terms[i] : nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
  for (int i = 0; i < n; ++i) PP_CHECK_ARG(terms[i], "weighted_sum_fwd: null term");
  a.n = n;
  hipLaunchKernelGGL(weighted_sum_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, out);
  return pp_launch_status("weighted_sum_fwd");
}
extern "C" int pp_weighted_sum_bwd(const float* g, const float* weights, int n, float* gout, void* stream) {
  PP_CHECK_ARG(g && weights && gout && n >= 1 && n <= 8, "weighted_sum_bwd: 1..8 terms");
  WSumArgs a;
  for (int i = 0; i < 8; ++i) { a.t[i] = nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
  a.n = n;
  hipLaunchKernelGGL(weighted_sum_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, g, a, gout);
  return pp_launch_status("weighted_sum_bwd");
}

extern "C" size_t pp_hd95_workspace(int N, int K, int H, int W) {
  return (size_t)N * K * 2 * H * W * sizeof(int) + 64;
}

// pred / label: int64 class maps [N][H][W] (device).  dist: [N*K][2][H*W] floats, counts: [N*K][4] ints (device); the
// caller takes the 95th percentile of dist[item][0][:counts[0]] ++ dist[item][1][:counts[1]] (numpy.percentile, linear).
extern "C" int pp_hd95_surface_distances(const int64_t* pred, const int64_t* label, int N, int K, int H, int W,
                                         float spacing_y, float spacing_x, float* dist, int* counts, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  PP_CHECK_ARG(pred && label && dist && counts && workspace && N >= 1 && K >= 1 && H >= 1 && W >= 1, "hd95: bad arguments");
  if (workspace_bytes < pp_hd95_workspace(N, K, H, W)) {
    pp_set_error("hd95: workspace too small");
    return PP_ERR_WORKSPACE;
  }
  int* coords = reinterpret_cast<int*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  const int cap = H * W;
  pp_prof_begin(PP_K_LOSS, 0.0, 16.0 * N * K * H * W, s);
  hipLaunchKernelGGL(hd_surface_kernel, dim3(N * K), dim3(HD_THREADS), 0, s, (const long long*)pred, (const long long*)label, K, H,
                     W, cap, coords, counts);
  hipLaunchKernelGGL(hd_distance_kernel, dim3(N * K, 2), dim3(HD_THREADS), 0, s, coords, counts, W, cap, spacing_y, spacing_x, dist);
  pp_prof_end(s);
  return pp_launch_status("hd95_surface_distances");
}
