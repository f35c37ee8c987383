// Random walker with priors (include/pacingpseudo_rwp.h; DESIGN.md section 7, "Random-walker refresh"): the whole of
// libpacingpseudo_rwp.so.  The training driver re-runs the walker every few epochs with the network's own soft-max as a unary
// prior beside the scribble seeds (Grady 2005) and replaces the pseudo-labels; nothing here runs inside the training step.
//
// Per slice and class k: (L_UU + gamma I) x_k = b_k + gamma q_k|U with q = softmax_k(logits), for EVERY class when gamma > 0
// (a class without a seed, and a slice without any seed, are ordinary systems: the shift alone makes them definite); gamma = 0 is
// the plain walker, a class without a seed is exactly 0 and runs no solve.  Two kernels:
//   rw_weights_kernel  (pp_rw_common.h, shared with pp_random_walker.hip) with shift = gamma: the diagonal of an unknown pixel is
//                      sum_j w_ij + gamma, of a seed 0 -- how the solver tells U from S
//   rwp_solve_kernel   pp_random_walker.hip's rw_solve_kernel with the shifted diagonal and the prior in the right-hand side:
//                      one block of 1024 threads per (slice, class) system from start to finish, x in the prob plane, r, p and
//                      A p in the caller's workspace, a thread owns the pixels tid, tid + 1024, ...; only p is read across
//                      threads, always on the far side of a __syncthreads() from its stores.  q_k of a pixel is computed where
//                      it is needed (fp32, max-subtracted, classes summed in index order): once for the right-hand side, once
//                      for the true residual after the loop -- no plane of its own.
// Dot products as in the plain walker (per-thread serial in index order, a fixed shuffle tree per wave, the 16 wave sums in wave
// order, all in double): the same bits in every run, in any batch, on any stream.
#include "pacingpseudo_rwp.h"
#include "pp_rw_common.h"

#define PRWP_VERSION 100

// softmax_k(z)[k] of one pixel: z points at class 0 of the pixel, classes are `stride` floats apart
__device__ __forceinline__ float rwp_prior(const float* __restrict__ z, size_t stride, int K, int k) {
  float m = z[0];
  for (int c = 1; c < K; ++c) m = fmaxf(m, z[(size_t)c * stride]);
  float sum = 0.f;
  for (int c = 0; c < K; ++c) sum += expf(z[(size_t)c * stride] - m);
  return expf(z[(size_t)k * stride] - m) / sum;
}

// grid (K, slices of the chunk).  x and p carry no __restrict__: other threads of the block read what this one stores.
__global__ __launch_bounds__(RW_THREADS) void rwp_solve_kernel(const int* __restrict__ scb, const float* __restrict__ logits, RwSizes sz,
                                                                int n0, int K, int H, int W, float gamma, float tol, int max_iters,
                                                                const float* __restrict__ w_right, const float* __restrict__ w_down,
                                                                const float* __restrict__ diag, const unsigned* __restrict__ mask,
                                                                float* rbuf, float* pbuf, float* qbuf, float* prob,
                                                                float* __restrict__ stats) {
  __shared__ double s_a[RW_WAVES], s_b[RW_WAVES], s_c[RW_WAVES], s_d[RW_WAVES];
  const int k = blockIdx.x, n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y], np = h * w, HW = H * W;
  const size_t sl = (size_t)n * HW, sy = ((size_t)n * K + k) * HW;
  scb += sl, w_right += sl, w_down += sl, diag += sl;
  logits += (size_t)n * K * HW;
  float* r = rbuf + sy;
  float* p = pbuf + sy;
  float* q = qbuf + sy;
  float* x = prob + sy;
  float* st = stats + ((size_t)n * K + k) * 3;
  const bool prior = gamma > 0.f;
  const bool active = prior || ((mask[n] >> k) & 1u);            // gamma = 0: a class without a seed is exactly 0
  for (int i = threadIdx.x; i < HW; i += RW_THREADS) {
    const int y = i / W, xx = i - y * W;
    if (!active || y >= h || xx >= w) x[i] = 0.f;
  }
  if (!active) {                                                 // uniform: the whole block leaves before any barrier
    if (threadIdx.x == 0) st[0] = 0.f, st[1] = 0.f, st[2] = 1.f;
    return;
  }
  // x0 = one-hot at seeds, 0 on U; r0 = b = sum_j w_ij x0_j + gamma q; p0 = z0 = r0 / diag
  double bb_ = 0.0, rz_ = 0.0;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, xx = i - y * w, o = y * W + xx;
    const float d = diag[o];
    if (!(d > 0.f)) {                                            // a seed (gamma = 0: or a 1 x 1 slice's lone pixel): fixed
      const int s = scb[o];
      x[o] = (s == k) ? 1.f : 0.f;
      p[o] = 0.f;
      continue;
    }
    float b = 0.f;
    if (xx > 0 && scb[o - 1] == k) b += w_right[o - 1];
    if (xx + 1 < w && scb[o + 1] == k) b += w_right[o];
    if (y > 0 && scb[o - W] == k) b += w_down[o - W];
    if (y + 1 < h && scb[o + W] == k) b += w_down[o];
    if (prior) b = fmaf(gamma, rwp_prior(logits + o, (size_t)HW, K, k), b);
    const float z = b / d;
    x[o] = 0.f;
    r[o] = b;
    p[o] = z;
    bb_ += (double)b * b;
    rz_ += (double)b * z;
  }
  double bb, rz;
  rw_block_sum2(bb_, rz_, s_b, s_c, &bb, &rz);                   // the barrier inside also publishes p0
  const double thr = (double)tol * (double)tol * bb;
  double rr = bb;
  int it = 0;
  bool conv = rr <= thr;
  while (!conv && it < max_iters) {
    double pq_ = 0.0;
    for (int i = threadIdx.x; i < np; i += RW_THREADS) {
      const int y = i / w, xx = i - y * w, o = y * W + xx;
      const float d = diag[o];
      if (!(d > 0.f)) continue;
      const float pc = p[o];
      float a = d * pc;
      if (xx > 0) a = fmaf(-w_right[o - 1], p[o - 1], a);
      if (xx + 1 < w) a = fmaf(-w_right[o], p[o + 1], a);
      if (y > 0) a = fmaf(-w_down[o - W], p[o - W], a);
      if (y + 1 < h) a = fmaf(-w_down[o], p[o + W], a);
      q[o] = a;
      pq_ += (double)pc * a;
    }
    const double pq = rw_block_sum(pq_, s_a);
    if (!(pq > 0.0)) break;                                      // uniform; cannot happen for an SPD system short of overflow
    const float alpha = (float)(rz / pq);
    double rr_ = 0.0;
    rz_ = 0.0;
    for (int i = threadIdx.x; i < np; i += RW_THREADS) {
      const int y = i / w, xx = i - y * w, o = y * W + xx;
      const float d = diag[o];
      if (!(d > 0.f)) continue;
      x[o] = fmaf(alpha, p[o], x[o]);
      const float rn = fmaf(-alpha, q[o], r[o]);
      r[o] = rn;
      rr_ += (double)rn * rn;
      rz_ += (double)rn * (rn / d);
    }
    double rz_new;
    rw_block_sum2(rr_, rz_, s_b, s_c, &rr, &rz_new);
    ++it;
    conv = rr <= thr;
    if (!conv && it < max_iters) {
      const float bt = (float)(rz_new / rz);
      for (int i = threadIdx.x; i < np; i += RW_THREADS) {
        const int y = i / w, xx = i - y * w, o = y * W + xx;
        const float d = diag[o];
        if (!(d > 0.f)) continue;
        p[o] = fmaf(bt, p[o], r[o] / d);
      }
    }
    rz = rz_new;
    __syncthreads();                                             // the new p before the next A p reads it
  }
  // the true residual b - A x = sum_j w_ij (x_j - x_i) + gamma (q_i - x_i) with x = one-hot on the seeds, once, in double.  Every
  // store of x lies behind a barrier here (the one in the last block sum).
  double tr_ = 0.0;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, xx = i - y * w, o = y * W + xx;
    if (!(diag[o] > 0.f)) continue;
    const double xi = (double)x[o];
    double a = 0.0;
    if (xx > 0) a += (double)w_right[o - 1] * ((double)x[o - 1] - xi);
    if (xx + 1 < w) a += (double)w_right[o] * ((double)x[o + 1] - xi);
    if (y > 0) a += (double)w_down[o - W] * ((double)x[o - W] - xi);
    if (y + 1 < h) a += (double)w_down[o] * ((double)x[o + W] - xi);
    if (prior) a += (double)gamma * ((double)rwp_prior(logits + o, (size_t)HW, K, k) - xi);
    tr_ += a * a;
  }
  const double tr = rw_block_sum(tr_, s_d);
  if (threadIdx.x == 0) {
    st[0] = (float)it;
    st[1] = bb > 0.0 ? (float)sqrt(tr / bb) : 0.f;
    st[2] = conv ? 1.f : 0.f;
  }
}

// ---- host side ----
extern "C" int prwp_version(void) { return PRWP_VERSION; }
extern "C" const char* prwp_last_error(void) { return g_prep_err; }

extern "C" size_t prwp_workspace_bytes(int N, int K, int H, int W) {
  if (rw_check_shape("prwp_workspace_bytes", nullptr, N, K, H, W) != 0) return 0;
  const size_t plane = (size_t)H * W * sizeof(float);
  return rw_mask_bytes(N) + (size_t)N * 3 * plane + (size_t)N * K * 3 * plane;
}

extern "C" int prwp_solve(const float* img, const int* scb, const float* logits, const int* sizes, int N, int K, int H, int W, float beta,
                          float eps, float gamma, float tol, int max_iters, float* prob, float* stats, void* workspace, void* stream) {
  const char* who = "prwp_solve";
  PREP_CHECK_ARG(img && scb && logits && prob && stats && workspace,
                 "%s: null pointer (img %p, scb %p, logits %p, prob %p, stats %p, workspace %p)", who, (const void*)img, (const void*)scb,
                 (const void*)logits, (void*)prob, (void*)stats, workspace);
  PREP_CHECK_ARG((((uintptr_t)img | (uintptr_t)scb | (uintptr_t)logits | (uintptr_t)prob | (uintptr_t)stats) & 3) == 0,
                 "%s: pointers must be 4-byte aligned", who);
  PREP_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  PREP_CHECK_ARG(beta >= 0.f && isfinite(beta), "%s: beta = %g, need a finite beta >= 0", who, (double)beta);
  PREP_CHECK_ARG(eps > 0.f && isfinite(eps), "%s: eps = %g, need a finite eps > 0", who, (double)eps);
  PREP_CHECK_ARG(gamma >= 0.f && isfinite(gamma), "%s: gamma = %g, need a finite gamma >= 0", who, (double)gamma);
  PREP_CHECK_ARG(tol > 0.f && isfinite(tol), "%s: tol = %g, need a finite tol > 0", who, (double)tol);
  PREP_CHECK_ARG(max_iters >= 1, "%s: max_iters = %d, need max_iters >= 1", who, max_iters);
  const int rc = rw_check_shape(who, sizes, N, K, H, W);
  if (rc != 0) return rc;
  const size_t HW = (size_t)H * W;
  char* ws = (char*)workspace;
  unsigned* mask = (unsigned*)ws;
  float* w_right = (float*)(ws + rw_mask_bytes(N));
  float* w_down = w_right + (size_t)N * HW;
  float* diag = w_down + (size_t)N * HW;
  float* rbuf = diag + (size_t)N * HW;
  float* pbuf = rbuf + (size_t)N * K * HW;
  float* qbuf = pbuf + (size_t)N * K * HW;
  hipStream_t st = (hipStream_t)stream;
  for (int n0 = 0; n0 < N; n0 += RW_CHUNK) {
    const int cnt = N - n0 < RW_CHUNK ? N - n0 : RW_CHUNK;
    const RwSizes sz = rw_chunk_sizes(sizes, n0, cnt, H, W);
    rw_weights_kernel<<<dim3(cnt), dim3(RW_THREADS), 0, st>>>(img, scb, sz, n0, K, H, W, beta, eps, gamma, w_right, w_down, diag, mask);
    int e = rw_launched("prwp_solve (weights)");
    if (e != 0) return e;
    rwp_solve_kernel<<<dim3(K, cnt), dim3(RW_THREADS), 0, st>>>(scb, logits, sz, n0, K, H, W, gamma, tol, max_iters, w_right, w_down, diag,
                                                                mask, rbuf, pbuf, qbuf, prob, stats);
    e = rw_launched("prwp_solve (solve)");
    if (e != 0) return e;
  }
  return 0;
}
