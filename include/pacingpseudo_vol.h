/* pacingpseudo_vol.h -- C ABI of libpacingpseudo_vol.so (MI355X / gfx950): volume-wise evaluation of hard class maps -- 3-D connected
 * components, the keep-largest-3-D-component filter, the exact 3-D Euclidean distance transform and the two directed surface-distance
 * sets of a (prediction, label) pair of volumes (inference.py --volumes).  A seventh library beside pacingpseudo_hip.h (the step),
 * pacingpseudo_prep.h, pacingpseudo_rwp.h, pacingpseudo_unc.h, pacingpseudo_dist.h and pacingpseudo_geo.h: the symbol lists and
 * versions of those six are fixed by their tests.  The reference (zefanyang/pacingpseudo) scores every slice on its own.
 *
 * Definitions ("Volume-wise evaluation").  A volume is (D, H, W), x fastest; the linear index of a voxel is
 * z * H * W + y * W + x.  `connectivity` 1, 2, 3 = the 6-, 18-, 26-neighbourhood (scipy.ndimage.generate_binary_structure(3, c)).
 * Two voxels are connected when they are neighbours and hold the same value; the label of a voxel is the smallest linear index of
 * its component, so labels are unique.  The surface of a mask is mask XOR its erosion by the 6-neighbour cross with voxels outside
 * the volume counting as 0 (medpy's __surface_distances with connectivity 1).  Distances are Euclidean with voxel pitch
 * (sz, sy, sx); every candidate is formed in fp32 as fl(fl((g sz)^2 + (dy sy)^2) + (dx sx)^2) from singly rounded products, so with
 * unit spacing the squared field is exact (3 * 2048^2 < 2^24 bounds H and W; along z the distance is held as 16 bits).
 *
 * Conventions: raw DEVICE pointers (int64 arrays and every workspace 8-byte aligned, int32 / fp32 arrays 4-byte aligned); `void*
 * stream` = hipStream_t last; nothing allocated, no implicit synchronisation; 0 = OK, -1 = bad argument, positive = hipError_t;
 * pvol_last_error() returns a thread-local message; every argument is checked on the host before anything is launched.  Limits:
 * 1 <= D <= 4096, 1 <= H, W <= 2048, D * H * W < 2^31, 1 <= K <= 32, spacings finite and > 0; one volume per call (volumes differ
 * in depth).  Integer atomics only, no workspace region has to be cleared by the caller: the same bits in every run, whatever the
 * stream or the workspace's previous content.
 */
#ifndef PACINGPSEUDO_VOL_H
#define PACINGPSEUDO_VOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_vol.py: MIN_VOL_VERSION) refuses a library older than the header it was written against. */
int pvol_version(void);
const char* pvol_last_error(void);

/* With n = D * H * W and pad8(b) = b rounded up to a multiple of 8 -- every query returns 0 for arguments its call would refuse:
 *   pvol_label_workspace          pad8(4 n)                                          the parent forest
 *   pvol_keep_largest_workspace   pad8(16 K) + 3 pad8(4 n)                           per class {best, components, voxels}; forest, sizes, labels
 *   pvol_edt_workspace            pad8(2 n)                                          the 16-bit distances along z
 *   pvol_surface_workspace        pad8(4 n) + pad8(2 n) + 2 pad8(n) + pad8(24 B)     ONE class at a time: a distance field, the z distances,
 *                                 with B = ceil(n / 4096)                            two surface byte masks, six counters per block of 4096 voxels */
size_t pvol_label_workspace(int D, int H, int W);
size_t pvol_keep_largest_workspace(int K, int D, int H, int W);
size_t pvol_edt_workspace(int D, int H, int W);
size_t pvol_surface_workspace(int K, int D, int H, int W);

/* labels int32 (D, H, W): for every voxel -- every value is labelled, 0 included -- the smallest linear index of its component.
 * A union-find forest in which a parent is never larger than its child: bricks of 4 x 16 x 32 voxels are joined in LDS, the pairs
 * that straddle a brick face, edge or corner on the global parent array with relaxed agent-scope atomics, then the forest is
 * flattened.  No block waits for another; every retry of a union strictly descends. */
int pvol_label_components(const int64_t* cls, int D, int H, int W, int connectivity, int32_t* labels, void* workspace,
                          size_t workspace_bytes, void* stream);

/* out int64 (D, H, W), may be cls itself: of every foreground class 1 .. K - 1 the component with the most voxels stays (ties: the
 * smallest label), the class's other voxels become 0; values outside [1, K) are copied.  stats int32 (K, 2) = {components of the class
 * before filtering, voxels removed}; {0, 0} for class 0 and for an absent class. */
int pvol_keep_largest_components(const int64_t* cls, int K, int D, int H, int W, int connectivity, int64_t* out, int32_t* stats,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* out fp32 (D, H, W): scipy.ndimage.distance_transform_edt(mask, sampling=(sz, sy, sx)) -- at a non-zero voxel the distance to the
 * nearest zero voxel, 0 at a zero voxel; squared = 1 leaves the squared distances.  A volume without a zero voxel gives +inf
 * everywhere.  Three separable passes: z (16-bit voxel counts per column, threads along x), y and x (outward scans that stop once the
 * offset alone reaches the best candidate: exact). */
int pvol_edt(const unsigned char* mask, int D, int H, int W, float sz, float sy, float sx, int squared, float* out, void* workspace,
             size_t workspace_bytes, void* stream);

/* The 3-D counterpart of pp_hd95_surface_distances.  pred, label int64 (D, H, W); per class k in 0 .. K - 1 the surfaces of pred == k
 * and label == k.  dist fp32 (K, 2, cap) with cap = D * H * W: dist[k][0][:counts[k][0]] = for every surface voxel of the prediction,
 * in linear-index order, the distance to the nearest surface voxel of the label (+inf if it has none); dist[k][1][:counts[k][1]] the
 * other direction.  counts int32 (K, 4) = {|surface pred|, |surface label|, |pred|, |label|}.  The layout is the one
 * pp_surface_reduce(dist, counts, items = K, cap = D * H * W, ...) of libpacingpseudo_hip.so takes; that call needs
 * K * 2 * D * H * W < 2^31, which is checked here.  Classes are processed one after another in the same workspace. */
int pvol_surface_distances(const int64_t* pred, const int64_t* label, int K, int D, int H, int W, float sz, float sy, float sx,
                           float* dist, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* counts int32 (K, 3) = {|pred == k and label == k|, |pred == k|, |label == k|} per class: what the volume Dice is made of.  The
 * output is cleared here (hipMemsetAsync on the stream). */
int pvol_dice_counts(const int64_t* pred, const int64_t* label, int K, int D, int H, int W, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
