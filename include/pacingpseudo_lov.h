/* pacingpseudo_lov.h -- C ABI of libpacingpseudo_lov.so (MI355X / gfx950): a segmented, stable, descending radix sort on the device
 * and the Lovasz-softmax loss built on it (upper_bound_chaos.py --do_loss_lovasz; Berman, Triki, Blaschko, CVPR 2018).  A tenth library
 * beside pacingpseudo_hip.h (the step) and its eight companions: their symbol lists and versions are fixed by their tests.  The
 * reference (zefanyang/pacingpseudo) has no such loss.
 *
 * Definition ("Lovasz-softmax loss").  p = softmax(logits) over K.  A pixel is valid when 0 <= target < K and
 * target != ignore_index (has_ignore != 0); any other target value is ignored and indexes nothing.  A segment is one class over the
 * valid pixels of the batch (per_image = 0) or of one image (per_image = 1).  In a segment fg_i = [target_i == c], e_i = |fg_i - p_ci|;
 * the segment is ordered by e descending, ties in ascending pixel index (n, y, x).  With G = sum fg and c_i the running sum of fg
 * along that order (1-based i): J_i = 1 - (G - c_i) / (G + i - c_i), g_i = J_i - J_{i-1} (J_0 = 0), segment loss = sum_i e_i g_i.
 * classes_all = 0 averages over the segments with G > 0, classes_all = 1 over all K (G = 0: the loss is max e).  per_image: the mean
 * over all N images of the image's average, 0 for an image without an averaged segment.  No averaged segment at all: loss 0.
 * g_i is formed from the integer counts in double (1 / U_i for fg_i = 1, (G - c_i) / ((U_i - 1) U_i) for fg_i = 0, U_i = G + i - c_i),
 * the sums are double and in a fixed order.  A non-finite logit gives a NaN loss; nothing outside the stated extents is touched.
 *
 * The sort: least-significant digit first, 8-bit digits, four passes over (key, payload); per pass a histogram per block of
 * plov_tile() keys, a scan of the segment x digit x block table and a stable scatter.  One launch sequence serves all segments.
 *
 * Conventions: raw DEVICE pointers (fp32 / int32 buffers 4-byte aligned, int64 buffers and workspaces 8-byte aligned), `void* stream`
 * = hipStream_t last, nothing allocated, no implicit synchronisation, no device-to-host read; 0 = OK, -1 = bad argument, positive =
 * hipError_t; plov_last_error() returns a thread-local message; every argument is checked on the host before anything is launched.
 * Limits: 2 <= K <= 32, N, H, W >= 1, N * K * H * W < 2^31; the sort: S, n >= 1, S * n < 2^31.  Nothing in a workspace has to be
 * cleared.  No floating-point atomics: same bits in every run, whatever the stream or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_LOV_H
#define PACINGPSEUDO_LOV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_lov.py: MIN_LOV_VERSION) refuses a library older than the header it was written against. */
int plov_version(void);
const char* plov_last_error(void);

/* The largest number of keys one block handles per pass: a segment of more keys spans several blocks. */
int plov_tile(void);

/* Bytes of caller-owned device workspace of plov_sort_descending (two (key, payload) buffers of 4 + 4 bytes per value and the
 * digit table of 256 words per block); 0 for arguments the call would refuse. */
size_t plov_sort_workspace(int S, int n);

/* Sort each of the S rows of values fp32 (S, n) in descending order, stable: sorted fp32 (S, n) and perm int32 (S, n) equal
 * torch.sort(values, dim=1, descending=True, stable=True) for every float32 input (-0 ties with +0, every NaN is the one value above
 * +inf, equal values keep their order); sorted holds the input's own bit patterns. */
int plov_sort_descending(const float* values, int S, int n, float* sorted, int* perm, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Bytes of workspace of plov_loss_fwd (16 bytes per pixel and class, the digit table and the per-block and per-segment sums); 0 for
 * refused arguments. */
size_t plov_loss_workspace(int N, int K, int H, int W, int per_image);

/* The loss.  logits fp32 (N, K, H, W), target int64 (N, H, W), loss: one fp32 on the device.  Kept for plov_loss_bwd: weights fp32
 * (K, N*H*W), g of every pixel's rank in its segment, in pixel order (0 at ignored pixels), and seg_scale fp32, one per segment (K, or
 * N*K with per_image, image-major): 1 / (averaged segments [of the image] [* N]), 0 for a segment that is not averaged.  Optional
 * (may be null): errors fp32 (K, N*H*W), e in pixel order (0 at ignored pixels); perm int32, n flattened (n, y, x) pixel indices per
 * segment in sorted order, ignored pixels last in ascending index order ((K, N*H*W), or (N*K, H*W) with per_image). */
int plov_loss_fwd(const float* logits, const long long* target, int N, int K, int H, int W, int has_ignore, long long ignore_index,
                  int per_image, int classes_all, float* loss, float* weights, float* seg_scale, float* errors, int* perm,
                  void* workspace, size_t workspace_bytes, void* stream);

/* dp_ci = sign(p_ci - fg_i) * weights_ci * seg_scale * grad at valid pixels, 0 at ignored ones; dlogits_k = p_k (dp_k - sum_j p_j
 * dp_j), the soft-max recomputed.  `grad` is a DEVICE pointer to the upstream fp32 scalar. */
int plov_loss_bwd(const float* logits, const long long* target, int N, int K, int H, int W, int has_ignore, long long ignore_index,
                  int per_image, const float* weights, const float* seg_scale, const float* grad, float* dlogits, void* stream);

#ifdef __cplusplus
}
#endif
#endif
