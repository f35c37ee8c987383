/* pacingpseudo_unc.h -- C ABI of libpacingpseudo_unc.so (MI355X / gfx950): the uncertainty mask of the mean-teacher consistency
 * term (train_chaos.py --cr_uncertainty T; UA-MT, Yu et al. 2019; USTM, Liu et al. 2022).  A fourth library beside
 * pacingpseudo_hip.h (the step), pacingpseudo_prep.h and pacingpseudo_rwp.h (the two random walkers): the symbol lists and versions
 * of those three are fixed by their tests.  The reference (zefanyang/pacingpseudo) has no such stage.
 *
 * Definition ("Uncertainty mask").  For pass t = 0 .. T-1 the teacher sees x_t = x + clamp(sigma n_t, -c, +c),
 * n_t ~ N(0,1) from Philox-4x32-10 with key = (seed low 32 bits, seed high 32 bits) and counter = (q, t, step low 32, step high 32),
 * q the index of the element quad (elements 4q .. 4q+3 of the flattened array).  The four outputs r0..r3 give the uniforms
 * u_j = ((r_j >> 8) + 0.5) 2^-24, Box-Muller gives (n0, n1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1) and (n2, n3) likewise from
 * (u2, u3); element 4q+j takes n_j.  The value depends on (seed, step, t, element index) alone -- never on the grid, the vector
 * width or how the batch is split.  pbar = (1/T) sum_t softmax_k(logits_t) (fp32, max-subtracted, summed in the order t = 0..T-1),
 * u = -sum_k pbar_k ln pbar_k (a term with pbar_k = 0 is 0), mask = [u < threshold] * valid_mask.
 *
 * Conventions: raw DEVICE pointers (4-byte aligned; `state`, `stats` and the workspace 8-byte aligned), `void* stream` =
 * hipStream_t last, nothing allocated, no implicit synchronisation; 0 = OK, -1 = bad argument, positive = hipError_t;
 * punc_last_error() returns a thread-local message; every argument is checked on the host before anything is launched.
 * Limits: 2 <= K <= 32, N >= 1, HW >= 1, N * HW < 2^31, 1 <= passes <= 16, 0 <= pass < passes, sigma >= 0, clip >= 0, a finite
 * threshold, 1 <= n <= 2^34.  Same bits in every run, whatever the stream or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_UNC_H
#define PACINGPSEUDO_UNC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_unc.py: MIN_UNC_VERSION) refuses a library older than the header it was written against. */
int punc_version(void);
const char* punc_last_error(void);

/* Bytes of caller-owned device workspace of the LAST punc_accumulate call of a round (three doubles per block of 256 pixels;
 * nothing in it has to be cleared); 0 for arguments the call would refuse. */
size_t punc_workspace_bytes(int N, int K, int HW);

/* out[i] = image[i] + clamp(sigma * n_pass[i], -clip, +clip) for i in [0, n).  `state` is a DEVICE pointer to two uint64 values
 * (seed, step) that the KERNEL reads: a replayed graph draws the noise of the step the buffer holds then.  16-byte accesses when
 * both pointers are 16-byte aligned (scalar tail for n % 4), 4-byte accesses otherwise; the same bits per element either way.
 * out may equal image. */
int punc_noise_add(const float* image, long long n, float sigma, float clip, const unsigned long long* state, int pass, float* out,
                   void* stream);

/* One teacher pass into the running mean.  logits (N, K, HW) fp32.  pass 0 writes acc (N, K, HW) = softmax, passes 1 .. passes-2
 * add to it, the last pass (pass == passes - 1; with passes == 1 the only one, acc is not touched) forms pbar and u in registers
 * and writes mask (N, HW) fp32 = [u < threshold] * valid_mask (valid_mask (N, HW) fp32 or NULL = all ones), unc (N, HW) = u when
 * not NULL, and stats = double[3]: (sum of mask, sum of valid_mask * u, sum of valid_mask), from per-block partial sums in the
 * workspace that one block adds in a fixed order.  Earlier passes touch neither mask, unc, stats nor the workspace (they are
 * checked all the same). */
int punc_accumulate(const float* logits, int N, int K, int HW, int pass, int passes, const float* valid_mask, float threshold,
                    float* acc, float* mask, float* unc, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* state[1] += 1 (one thread): the next step's noise. */
int punc_advance(unsigned long long* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
