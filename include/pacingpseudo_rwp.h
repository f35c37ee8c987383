/* pacingpseudo_rwp.h -- C ABI of libpacingpseudo_rwp.so (MI355X / gfx950): the random walker with priors, which the training
 * driver re-runs every few epochs to refresh the scribble pseudo-labels (train_chaos.py --rw_refresh N).  A third library beside
 * pacingpseudo_hip.h (the step) and pacingpseudo_prep.h (the plain walker, once before the first step): the symbol lists and
 * versions of those two are fixed by their tests.  The reference (zefanyang/pacingpseudo) has no such stage.
 *
 * Definition (Grady 2005, "Multilabel random walker image segmentation using prior models"; DESIGN.md section 7, "Random-walker
 * refresh").  Slices, img, scb, g, w_ij, U and S exactly as in pacingpseudo_prep.h; logits (N, K, H, W) fp32 are the network's
 * outputs, q = softmax_k(logits) per pixel (fp32, max-subtracted, computed in the kernel).  For EVERY class k when gamma > 0
 *     (L_UU + gamma I) x_k = b_k + gamma q_k|U
 * is solved by the plain walker's Jacobi-preconditioned conjugate gradients (fp32 vectors, dot products in double, one workgroup
 * per (slice, class), fixed summation order).  prob[k] = x_k on U, the one-hot of scb on S, 0 outside h x w.  With gamma > 0 a
 * class without a seed, and a slice without any seed, are ordinary systems; because sum_k q_k = 1, sum_k prob[k] = 1 on h x w.
 * gamma = 0 is the plain walker: a class without a seed is exactly 0 and runs no solve.  Labels come from pprep_rw_labels.
 *
 * Conventions: those of pacingpseudo_prep.h -- raw DEVICE pointers (4-byte aligned; workspace 256-byte aligned), `sizes` a HOST
 * array of N (h, w) pairs or NULL, `void* stream` = hipStream_t last, nothing allocated, no implicit synchronisation; 0 = OK,
 * -1 = bad argument, -2 = unsupported size, positive = hipError_t; prwp_last_error() returns a thread-local message; every
 * argument is checked on the host before anything is launched.  Limits: 1 <= K <= 32, 1 <= h <= H <= 1024, 1 <= w <= W <= 1024,
 * N >= 1 (64 slices per launch); beta >= 0, eps > 0, gamma >= 0, tol > 0, all finite, max_iters >= 1.  Logits must be finite
 * inside h x w (the caller's duty: device data are not inspected); outside h x w nothing is read.  Same bits in every run,
 * whatever the batch, the stream or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_RWP_H
#define PACINGPSEUDO_RWP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_rwp.py: MIN_RWP_VERSION) refuses a library older than the header it was written against. */
int prwp_version(void);
const char* prwp_last_error(void);

/* Bytes of caller-owned device workspace of one prwp_solve call (per slice two weight planes and the diagonal, per system the
 * vectors r, p and A p; nothing in it has to be cleared); 0 for arguments the solve would refuse. */
size_t prwp_workspace_bytes(int N, int K, int H, int W);

/* prob (N, K, H, W) fp32, every element written.  stats (N, K, 3) fp32 = (iterations, true relative residual
 * ||b + gamma q - (L_UU + gamma I) x|| / ||b + gamma q|| evaluated once after the loop, converged 1 / 0) per system; with
 * gamma = 0 a class without a seed reports (0, 0, 1).  The loop ends when the recurrence residual satisfies
 * ||r||^2 <= tol^2 ||b + gamma q||^2, or after max_iters iterations. */
int prwp_solve(const float* img, const int* scb, const float* logits, const int* sizes, int N, int K, int H, int W, float beta,
               float eps, float gamma, float tol, int max_iters, float* prob, float* stats, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
