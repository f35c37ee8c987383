/* pacingpseudo_prep.h -- C ABI of libpacingpseudo_prep.so (MI355X / gfx950): work done ONCE on the training data before the
 * first step, beside the per-step library of pacingpseudo_hip.h.  The reference (zefanyang/pacingpseudo) trains on the scribbles
 * as they are on disk and has no such stage.
 *
 * Random-walker expansion of scribbles (Grady 2006; DESIGN.md section 7, "Random-walker scribbles").  A slice of true size
 * h x w lies in the top-left corner of a padded H x W plane; img is its image, scb its scribble map with values 0 .. K where K
 * means "unlabelled".  With g = (img - mean) / (std + 1e-8) (mean and population std over the h x w pixels, sums in double),
 * edge weights w_ij = exp(-beta (g_i - g_j)^2) + eps on the 4-neighbour grid inside h x w, U = {scb == K}, S = {scb < K}:
 * for every class k with a seed in the slice
 *     L_UU x_k = b_k,   (L_UU)_ii = sum_{j~i} w_ij,   (L_UU)_ij = -w_ij (i, j in U),   (b_k)_i = sum_{j~i, j in S, scb_j = k} w_ij
 * is solved by Jacobi-preconditioned conjugate gradients in fp32 with every dot product in double.  prob[k] = x_k on U and the
 * one-hot of scb on S; a class without a seed has prob[k] = 0 and runs no solve; prob = 0 outside h x w.
 *
 * Conventions (those of pacingpseudo_hip.h)
 *   - plain C types; img, scb, prob, stats, out, workspace are raw DEVICE pointers (4-byte aligned; workspace 256-byte aligned);
 *     `sizes` is a HOST array of N (h, w) pairs, read before the call returns, or NULL for h = H, w = W everywhere;
 *     `void* stream` = hipStream_t, last; all work is enqueued there, no implicit synchronisation, nothing allocated.
 *   - return value: 0 = OK, negative = library error (bad argument -1, unsupported size -2), positive = hipError_t;
 *     pprep_last_error() returns a thread-local message for the last failure.  The size query returns bytes, 0 for arguments
 *     the solve would refuse.  Every argument is checked on the host before anything is launched.
 *   - limits: 1 <= K <= 32, 1 <= h <= H <= 1024, 1 <= w <= W <= 1024, N >= 1 (beyond: -2); beta >= 0, eps > 0, tol > 0,
 *     max_iters >= 1, 0 < threshold <= 1, all finite (else -1).  Scribble values outside 0 .. K count as K.
 *   - results do not depend on what else is in the batch, on the stream, or on stale workspace content: same bits every run.
 */
#ifndef PACINGPSEUDO_PREP_H
#define PACINGPSEUDO_PREP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_prep.py: MIN_PREP_VERSION) refuses a library older than the header it was written against. */
int pprep_version(void);
const char* pprep_last_error(void);

/* Bytes of caller-owned device workspace of one pprep_rw_solve call: per slice the weight planes w_right, w_down and the
 * diagonal, per (slice, class) system the vectors r, p and A p; nothing in it has to be cleared. */
size_t pprep_rw_workspace_bytes(int N, int K, int H, int W);

/* prob (N, K, H, W) fp32, every element written.  stats (N, K, 3) fp32 = (iterations, true relative residual
 * ||b - A x|| / ||b|| evaluated once after the loop, converged 1 / 0) per system; a class without a seed reports (0, 0, 1).
 * The loop ends when the recurrence residual satisfies ||r||^2 <= tol^2 ||b||^2, or after max_iters iterations. */
int pprep_rw_solve(const float* img, const int* scb, const int* sizes, int N, int K, int H, int W, float beta, float eps,
                   float tol, int max_iters, float* prob, float* stats, void* workspace, void* stream);

/* out (N, H, W) int32: the seed's class on S; on U the first-maximum arg-max over k of prob where that maximum >= threshold,
 * else K; K outside h x w. */
int pprep_rw_labels(const float* prob, const int* scb, const int* sizes, int N, int K, int H, int W, float threshold, int* out,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
