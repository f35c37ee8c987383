/* pacingpseudo_dist.h -- C ABI of libpacingpseudo_dist.so (MI355X / gfx950): exact Euclidean distance transforms on the device and
 * the boundary loss built on them (upper_bound_chaos.py --do_loss_boundary; Kervadec et al., MIDL 2019).  A fifth library beside
 * pacingpseudo_hip.h (the step), pacingpseudo_prep.h, pacingpseudo_rwp.h (the two random walkers) and pacingpseudo_unc.h (the
 * uncertainty mask): the symbol lists and versions of those four are fixed by their tests.  The reference (zefanyang/pacingpseudo)
 * has no such stage.
 *
 * Definition ("Boundary loss").  The distance between pixels (y, x) and (y', x') is
 * sqrt(((y - y') sy)^2 + ((x - x') sx)^2).  The transform is the separable exact one: a column pass gives every pixel its distance
 * along y (in pixels, 16 bits) to the nearest pixel of the opposite membership, a row pass takes the minimum over x' of
 * g(y, x')^2 + ((x - x') sx)^2 by an outward scan that stops once ((x - x') sx)^2 >= the best candidate so far.  Every candidate is
 * formed in fp32 as (g sy)^2 + (dx sx)^2; with unit spacing all of them are integers below 2^24 and the squared field is exact.
 *
 * Conventions: raw DEVICE pointers (fp32 and int64 buffers aligned to their element size, workspaces 8-byte aligned), `void* stream`
 * = hipStream_t last, nothing allocated, no implicit synchronisation; 0 = OK, -1 = bad argument, positive = hipError_t;
 * pdist_last_error() returns a thread-local message; every argument is checked on the host before anything is launched.
 * Limits: 1 <= H, W <= 2048, 1 <= K <= 32, N >= 1 (P >= 1), N * K * H * W < 2^31 (P * H * W < 2^31), spacings finite and > 0.
 * No floating-point atomics: same bits in every run, whatever the stream or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_DIST_H
#define PACINGPSEUDO_DIST_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_dist.py: MIN_DIST_VERSION) refuses a library older than the header it was written against. */
int pdist_version(void);
const char* pdist_last_error(void);

/* Bytes of caller-owned device workspace of pdist_edt (the column distances, 2 bytes per pixel, rounded up to 8; nothing in it has
 * to be cleared); 0 for arguments the call would refuse. */
size_t pdist_edt_workspace(int P, int H, int W);

/* Exact Euclidean distance transform of P binary planes.  mask uint8 (P, H, W), out fp32 (P, H, W): at a non-zero pixel the distance
 * to the nearest zero pixel of the same plane (scipy.ndimage.distance_transform_edt(mask, sampling=(sy, sx))), at a zero pixel 0,
 * +inf everywhere in a plane without a zero pixel.  squared != 0 returns the squared field (no root). */
int pdist_edt(const unsigned char* mask, int P, int H, int W, float sy, float sx, int squared, float* out, void* workspace,
              size_t workspace_bytes, void* stream);

/* Bytes of workspace of pdist_signed_maps (2 bytes per pixel and class, rounded up to 8); 0 for refused arguments. */
size_t pdist_signed_maps_workspace(int N, int K, int H, int W);

/* Level-set maps of the boundary loss from the class-index map.  class_map int64 (N, H, W), phi fp32 (N, K, H, W).  With S the
 * pixels of image n whose value is k: phi = +d(x, S) outside S, -(d(x, complement of S) - min(sy, sx)) inside; phi of that (n, k)
 * is 0 everywhere when S is empty or the whole image.  A value outside [0, K) is outside every S.  No one-hot planes are formed:
 * one thread per column reads the class map once per sweep and writes the column distances of all K classes. */
int pdist_signed_maps(const long long* class_map, int N, int K, int H, int W, float sy, float sx, float* phi, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Bytes of workspace of pdist_boundary_loss_fwd (one double per block of 256 pixels); 0 for refused arguments. */
size_t pdist_boundary_loss_workspace(int N, int K, int H, int W);

/* loss = (1 / (N |I| H W)) sum_{n, k in I, x} softmax_k(logits) phi_k, I = {1 .. K-1} (for K = 1: {0}).  logits, phi fp32
 * (N, K, H, W); loss: one fp32 on the device.  Per-block partial sums in double into the workspace, then one block adds them in a
 * fixed order. */
int pdist_boundary_loss_fwd(const float* logits, const float* phi, int N, int K, int H, int W, float* loss, void* workspace,
                            size_t workspace_bytes, void* stream);

/* dlogits_j = g p_j (1[j in I] phi_j - sum_{k in I} p_k phi_k) / (N |I| H W), the soft-max recomputed; `grad` is a DEVICE pointer to
 * the upstream fp32 scalar g.  phi receives no gradient. */
int pdist_boundary_loss_bwd(const float* logits, const float* phi, int N, int K, int H, int W, const float* grad, float* dlogits,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
