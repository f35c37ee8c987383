/* pacingpseudo_opt.h -- C ABI of libpacingpseudo_opt.so (MI355X / gfx950): fused AdamW over a flat fp32 parameter slab, with a per-element
 * exemption from the weight decay (pacingpseudo_amd.optim.FusedAdamW; train_chaos.py / upper_bound_chaos.py --optimizer adamw
 * [--wd_exempt_1d]).  A ninth library beside pacingpseudo_hip.h (the step, whose pp_adam_step_* / pp_sgd_momentum_step_* entry points
 * decay through the gradient and are left as they are) and its seven companions: the symbol lists and versions of those eight are
 * fixed by their tests.  The reference (zefanyang/pacingpseudo) trains with torch.optim.Adam only.
 *
 * Definition ("Fused AdamW"): torch.optim.AdamW, non-amsgrad, maximize=False.  For an element of a step that is
 * not skipped, with t0 = step_dev[0], t = t0 + 1 and lr read from lr_dev[0] when lr_dev is given:
 *     gc  = clip_dev ? fl32(g * clip_dev[0]) : g                       rounded on its own
 *     f   = (float)(1.0 - (double)lr * (double)weight_decay)           f = 1 where exempt[i] != 0
 *     pd  = fl32(p * f)                                                rounded on its own: p * 1 is p exactly
 *     m   = b1 m + (1 - b1) gc ;  v = b2 v + (1 - b2) gc gc            the decay never enters the moments
 *     p   = pd - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))        bc1 = 1 - b1^t, bc2 = 1 - b2^t formed in double, rounded once
 *     ema = ema + fl32(w * fl32(p - ema))                              w = fl32(1 - min(D, (1 + t0) / (10 + t0)))
 * A skipped step (skip && skip[0] != 0) touches none of p, m, v, ema and does not advance step_dev[0]; it adds 1 to skip[1] iff
 * count_skip != 0 (give it to the first segment's call of an optimizer step only: one skipped step, one count).  Otherwise
 * step_dev[0] is advanced by 1 behind the update.
 *
 * Conventions: raw DEVICE pointers; p, g, m, v, ema fp32[n] and 16-byte aligned; exempt (nullable: nothing is exempt and no mask is
 * read) one byte per element of the same range, 4-byte aligned; step_dev (required), skip (nullable, int[2]), lr_dev (nullable),
 * clip_dev device scalars, 4-byte aligned; `void* stream` = hipStream_t last; nothing allocated, nothing copied, no implicit
 * synchronisation; 0 = OK, -1 = bad argument, positive = hipError_t; popt_last_error() returns a thread-local message; every
 * argument is checked on the host before anything is launched: n >= 1, lr / eps / weight_decay finite and >= 0, betas in [0, 1),
 * ema_decay in (0, 1).  No atomics: the same bits in every run, eager or replayed from a hipGraph.
 */
#ifndef PACINGPSEUDO_OPT_H
#define PACINGPSEUDO_OPT_H

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_opt.py: MIN_OPT_VERSION) refuses a library older than the header it was written against. */
int popt_version(void);
const char* popt_last_error(void);

/* Elements one trip of the update kernel's largest grid covers (4 per lane x threads per block x the block cap): a range longer than
 * this goes round the kernel's grid-stride loop more than once. */
long long popt_trip_elements(void);

/* The update above without clipping and without a shadow slab. */
int popt_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1, float beta2,
                    float eps, float weight_decay, int* step_dev, int* skip, int count_skip, const unsigned char* exempt, void* stream);

/* ... on gradients scaled by the clip coefficient clip_dev[0] (required; out2 + 1 of pp_grad_clip_finalize).  g is not written. */
int popt_adamw_step_clip(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                         float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                         const unsigned char* exempt, const float* clip_dev, void* stream);

/* ... that also moves the shadow slab ema (required, laid out as p) towards the p it has just computed; clip_dev nullable. */
int popt_adamw_step_ema(float* p, const float* g, float* m, float* v, long long n, float lr, const float* lr_dev, float beta1,
                        float beta2, float eps, float weight_decay, int* step_dev, int* skip, int count_skip,
                        const unsigned char* exempt, float* ema, double ema_decay, const float* clip_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
