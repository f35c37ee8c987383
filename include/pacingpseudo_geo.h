/* pacingpseudo_geo.h -- C ABI of libpacingpseudo_geo.so (MI355X / gfx950): geodesic distance transforms of scribble seeds on a guide
 * image and the dense pseudo-labels taken from them (train_chaos.py --geo_scribbles; GeoS, Criminisi et al. 2008; DeepIGeoS, Wang et
 * al. 2018).  A sixth library beside pacingpseudo_hip.h (the step), pacingpseudo_prep.h, pacingpseudo_rwp.h (the two random
 * walkers), pacingpseudo_unc.h (the uncertainty mask) and pacingpseudo_dist.h (Euclidean distance maps): the symbol lists and
 * versions of those five are fixed by their tests.  The reference (zefanyang/pacingpseudo) has no such stage.
 *
 * Definition ("Geodesic scribbles").  A slice has true size h x w in the top-left corner of an H x W plane, a
 * guide g (fp32) and a scribble map with values 0 .. K (K = unlabelled).  Paths move between 8-neighbours inside h x w only.  A step
 * from p to q costs
 *     c(p, q) = fl(s + fl(lam * |fl(g_p - g_q)|)),   s = 1.0f for the four axis neighbours, 1.41421354f (0x3FB504F3) for the diagonals,
 * every operation rounded to fp32 on its own (no fused multiply-add).  dist[n, k] is the least fixed point of
 *     d(q) = min(d0(q), min over neighbours p of fl(d(p) + c(p, q))),   d0 = 0 where scb == k, +inf elsewhere;
 * a candidate replaces a value only if candidate < value, so a NaN cost never propagates and a NaN pixel is a wall.  dist[n, k] is
 * +inf over the whole plane for a class without a seed in that slice, and +inf outside h x w.  fl(x + c) is monotone in x and never
 * below x, so the fixed point is unique BIT FOR BIT whatever the order of relaxation: it is what a float32 Dijkstra computes.
 * Labels: with best = the first arg-min over k and second = the smallest distance among the other classes (+inf if none), a pixel
 * takes best iff D_best is finite, D_best <= max_dist and D_best <= fl(ratio * D_second), otherwise K; seeds keep their class; K
 * outside h x w.
 *
 * Conventions: raw DEVICE pointers (4-byte aligned, the workspace 8-byte aligned) except `sizes`, a HOST int[N][2] of (h, w) or NULL
 * (every slice fills its plane); `void* stream` = hipStream_t last, nothing allocated, no implicit synchronisation; 0 = OK, -1 = bad
 * argument, positive = hipError_t; pgeo_last_error() returns a thread-local message; every argument is checked on the host before
 * anything is launched.  Limits: 1 <= H, W <= 1024, 1 <= K <= 32, N >= 1, N * K * H * W < 2^31.  No floating-point atomics: same
 * bits in every run, whatever the stream, the batch or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_GEO_H
#define PACINGPSEUDO_GEO_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_geo.py: MIN_GEO_VERSION) refuses a library older than the header it was written against. */
int pgeo_version(void);
const char* pgeo_last_error(void);

/* The guide of the walkers' normalisation: g = (img - mean) / (std + 1e-8), mean and population standard deviation over the slice's
 * own h x w pixels, sums in double in a fixed order, one rounding to fp32.  img, g fp32 (N, H, W); g is 0 outside h x w; a constant
 * slice gives g = 0.  One workgroup per slice. */
int pgeo_normalize(const float* img, const int* sizes, int N, int H, int W, float* g, void* stream);

/* Bytes of caller-owned device workspace of pgeo_distance (one byte per (slice, class, 64 x 64 tile), rounded up to 8; nothing in
 * it has to be cleared); 0 for arguments the call would refuse. */
size_t pgeo_distance_workspace(int N, int K, int H, int W);

/* Geodesic distances.  g fp32 (N, H, W), scb int32 (N, H, W) with values 0 .. K (anything else counts as unlabelled), lam finite
 * and >= 0, dist fp32 (N, K, H, W), stats int32 (N, K, 2) = (passes over the plane, converged).  One workgroup per (slice, class)
 * plane; a pass is one walk over the plane's dirty 64 x 64 tiles, each relaxed to its own fixed point, and a pass that changes no
 * pixel ends the loop with converged = 1.  A plane without a seed reports (0, 1) and never runs; a plane whose every pixel is a
 * seed reports (1, 1).  Reaching max_sweeps (in [1, 2^31)) first gives converged = 0: the field left behind is >= the exact one
 * everywhere and 0 at the seeds. */
int pgeo_distance(const float* g, const int* scb, const int* sizes, int N, int K, int H, int W, float lam, int max_sweeps, float* dist,
                  int* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Labels from the distances by the ratio rule above: max_dist > 0 (+inf allowed), ratio in (0, 1].  out int32 (N, H, W). */
int pgeo_labels(const float* dist, const int* scb, const int* sizes, int N, int K, int H, int W, float max_dist, float ratio, int* out,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif
