// Random-walker expansion of scribbles (include/pacingpseudo_prep.h; DESIGN.md section 7, "Random-walker scribbles"): the whole of
// libpacingpseudo_prep.so.  The reference trains on the scribbles as they are on disk; this runs once per training slice before
// the first step and never inside it, which is why it is a library of its own beside the per-step one.
//
// Per slice (h x w in the corner of an H x W plane) and class k with a seed: L_UU x_k = b_k on the 4-neighbour grid, solved by
// Jacobi-preconditioned conjugate gradients, matrix-free, fp32 vectors, every dot product in double.  Three kernels:
//   rw_weights_kernel  one block per slice: mean and population std of the image (double, two passes), then the two weight planes
//                      w_right[y][x] = w((y,x),(y,x+1)), w_down[y][x] = w((y,x),(y+1,x)) (0 at the slice's last column / row), the
//                      diagonal sum_j w_ij -- written as 0 at SEED pixels, which is how the solver tells U from S -- and the bit
//                      mask of the classes that have a seed
//   rw_solve_kernel    one block of 1024 threads per (slice, class) system from start to finish.  x lives in the prob plane itself
//                      (one-hot at seeds, so b = sum_j w_ij x0_j), r, p and A p in the caller's workspace.  A thread owns the
//                      pixels tid, tid + 1024, ... of the slice's row-major h x w order: r, A p and x are touched by their owner
//                      alone; p is read by the owners of the four neighbours, always on the far side of a __syncthreads() from
//                      its stores.  All waves of a block share their CU's L1, so plain stores, the barrier, plain loads are a
//                      complete workgroup-scope hand-off; no block reads another block's vectors, so nothing wider is needed.
//   rw_labels_kernel   thresholded first-maximum arg-max into an int32 map
// Dot products: per-thread serial sum over its pixels in index order, a fixed shuffle tree per wave, the 16 wave sums through
// LDS added in wave order by every thread -- all threads hold the same double, so the loop's exit test (read from those LDS
// values) is uniform and every barrier is reached by the whole block; the loop is bounded by max_iters.  The order depends on
// (h, w) alone: the same bits in every run, in any batch, on any stream.
#include "pacingpseudo_prep.h"
#include "pp_rw_common.h"        // size tables, block sums, rw_weights_kernel, argument checks: shared with pp_rw_prior.hip

#define PPREP_VERSION 100
#define RW_LABEL_THREADS 256

// grid (K, slices of the chunk).  x and p carry no __restrict__: other threads of the block read what this one stores.
__global__ __launch_bounds__(RW_THREADS) void rw_solve_kernel(const int* __restrict__ scb, RwSizes sz, int n0, int K, int H, int W,
                                                               float tol, int max_iters, const float* __restrict__ w_right,
                                                               const float* __restrict__ w_down, const float* __restrict__ diag,
                                                               const unsigned* __restrict__ mask, float* rbuf, float* pbuf, float* qbuf,
                                                               float* prob, float* __restrict__ stats) {
  __shared__ double s_a[RW_WAVES], s_b[RW_WAVES], s_c[RW_WAVES], s_d[RW_WAVES];
  const int k = blockIdx.x, n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y], np = h * w, HW = H * W;
  const size_t sl = (size_t)n * HW, sy = ((size_t)n * K + k) * HW;
  scb += sl, w_right += sl, w_down += sl, diag += sl;
  float* r = rbuf + sy;
  float* p = pbuf + sy;
  float* q = qbuf + sy;
  float* x = prob + sy;
  float* st = stats + ((size_t)n * K + k) * 3;
  const bool seeded = (mask[n] >> k) & 1u;
  for (int i = threadIdx.x; i < HW; i += RW_THREADS) {
    const int y = i / W, xx = i - y * W;
    if (!seeded || y >= h || xx >= w) x[i] = 0.f;
  }
  if (!seeded) {                                                 // uniform: the whole block leaves before any barrier
    if (threadIdx.x == 0) st[0] = 0.f, st[1] = 0.f, st[2] = 1.f;
    return;
  }
  // x0 = one-hot at seeds, 0 on U; r0 = b = sum_j w_ij x0_j; p0 = z0 = r0 / diag
  double bb_ = 0.0, rz_ = 0.0;
  for (int i = threadIdx.x; i < np; i += RW_THREADS) {
    const int y = i / w, xx = i - y * w, o = y * W + xx;
    const float d = diag[o];
    if (!(d > 0.f)) {                                            // a seed (or a 1 x 1 slice's lone pixel): fixed, never a direction
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
  // the true residual b - A x = sum_j w_ij (x_j - x_i) with x = one-hot on the seeds, once, in double.  Every store of x lies
  // behind a barrier here (the one in the last block sum).
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
    tr_ += a * a;
  }
  const double tr = rw_block_sum(tr_, s_d);
  if (threadIdx.x == 0) {
    st[0] = (float)it;
    st[1] = bb > 0.0 ? (float)sqrt(tr / bb) : 0.f;
    st[2] = conv ? 1.f : 0.f;
  }
}

// grid (blocks over H * W, slices of the chunk)
__global__ __launch_bounds__(RW_LABEL_THREADS) void rw_labels_kernel(const float* __restrict__ prob, const int* __restrict__ scb, RwSizes sz,
                                                                      int n0, int K, int H, int W, float threshold,
                                                                      int* __restrict__ out) {
  const int n = n0 + blockIdx.y, h = sz.h[blockIdx.y], w = sz.w[blockIdx.y], HW = H * W;
  const int i = blockIdx.x * RW_LABEL_THREADS + threadIdx.x;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  const size_t o = (size_t)n * HW + i;
  int lab = K;
  if (y < h && x < w) {
    const int s = scb[o];
    if (s >= 0 && s < K) {
      lab = s;
    } else {
      const float* pr = prob + (size_t)n * K * HW + i;
      float best = pr[0];
      int arg = 0;
      for (int k = 1; k < K; ++k) {
        const float v = pr[(size_t)k * HW];
        if (v > best) best = v, arg = k;
      }
      if (best >= threshold) lab = arg;
    }
  }
  out[o] = lab;
}

extern "C" int pprep_version(void) { return PPREP_VERSION; }
extern "C" const char* pprep_last_error(void) { return g_prep_err; }

extern "C" size_t pprep_rw_workspace_bytes(int N, int K, int H, int W) {
  if (rw_check_shape("pprep_rw_workspace_bytes", nullptr, N, K, H, W) != 0) return 0;
  const size_t plane = (size_t)H * W * sizeof(float);
  return rw_mask_bytes(N) + (size_t)N * 3 * plane + (size_t)N * K * 3 * plane;
}

extern "C" int pprep_rw_solve(const float* img, const int* scb, const int* sizes, int N, int K, int H, int W, float beta, float eps,
                              float tol, int max_iters, float* prob, float* stats, void* workspace, void* stream) {
  const char* who = "pprep_rw_solve";
  PREP_CHECK_ARG(img && scb && prob && stats && workspace, "%s: null pointer (img %p, scb %p, prob %p, stats %p, workspace %p)", who,
                 (const void*)img, (const void*)scb, (void*)prob, (void*)stats, workspace);
  PREP_CHECK_ARG((((uintptr_t)img | (uintptr_t)scb | (uintptr_t)prob | (uintptr_t)stats) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  PREP_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
  PREP_CHECK_ARG(beta >= 0.f && isfinite(beta), "%s: beta = %g, need a finite beta >= 0", who, (double)beta);
  PREP_CHECK_ARG(eps > 0.f && isfinite(eps), "%s: eps = %g, need a finite eps > 0", who, (double)eps);
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
    rw_weights_kernel<<<dim3(cnt), dim3(RW_THREADS), 0, st>>>(img, scb, sz, n0, K, H, W, beta, eps, 0.f, w_right, w_down, diag, mask);
    int e = rw_launched("pprep_rw_solve (weights)");
    if (e != 0) return e;
    rw_solve_kernel<<<dim3(K, cnt), dim3(RW_THREADS), 0, st>>>(scb, sz, n0, K, H, W, tol, max_iters, w_right, w_down, diag, mask, rbuf,
                                                               pbuf, qbuf, prob, stats);
    e = rw_launched("pprep_rw_solve (solve)");
    if (e != 0) return e;
  }
  return 0;
}

extern "C" int pprep_rw_labels(const float* prob, const int* scb, const int* sizes, int N, int K, int H, int W, float threshold, int* out,
                               void* stream) {
  const char* who = "pprep_rw_labels";
  PREP_CHECK_ARG(prob && scb && out, "%s: null pointer (prob %p, scb %p, out %p)", who, (const void*)prob, (const void*)scb, (void*)out);
  PREP_CHECK_ARG((((uintptr_t)prob | (uintptr_t)scb | (uintptr_t)out) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  PREP_CHECK_ARG(threshold > 0.f && threshold <= 1.f, "%s: threshold = %g, need 0 < threshold <= 1", who, (double)threshold);
  const int rc = rw_check_shape(who, sizes, N, K, H, W);
  if (rc != 0) return rc;
  const int HW = H * W;
  hipStream_t st = (hipStream_t)stream;
  for (int n0 = 0; n0 < N; n0 += RW_CHUNK) {
    const int cnt = N - n0 < RW_CHUNK ? N - n0 : RW_CHUNK;
    const RwSizes sz = rw_chunk_sizes(sizes, n0, cnt, H, W);
    rw_labels_kernel<<<dim3((HW + RW_LABEL_THREADS - 1) / RW_LABEL_THREADS, cnt), dim3(RW_LABEL_THREADS), 0, st>>>(prob, scb, sz, n0, K, H,
                                                                                                                   W, threshold, out);
    const int e = rw_launched("pprep_rw_labels");
    if (e != 0) return e;
  }
  return 0;
}
