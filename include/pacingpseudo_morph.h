/* pacingpseudo_morph.h -- C ABI of libpacingpseudo_morph.so (MI355X / gfx950): what to do with the component labels of a hard class
 * map beyond keeping the largest component -- a size threshold per class and hole filling (inference.py --min_component_size,
 * --fill_holes).  An eighth library beside pacingpseudo_hip.h (the step), pacingpseudo_prep.h, pacingpseudo_rwp.h, pacingpseudo_unc.h,
 * pacingpseudo_dist.h, pacingpseudo_geo.h and pacingpseudo_vol.h: the symbol lists and versions of those seven are fixed by their
 * tests.  The reference (zefanyang/pacingpseudo) scores its raw arg-max; it has no such stage.
 *
 * Definitions ("Size threshold and hole filling").  An item is one slice (dims = 2: (H, W), D = 1) or one volume
 * (dims = 3: (D, H, W)); N items lie one after another.  The linear index of a voxel within its item is z * H * W + y * W + x.
 * `labels` is what pp_label_components (dims = 2, libpacingpseudo_hip.so) or pvol_label_components (dims = 3, one call per item,
 * libpacingpseudo_vol.so) wrote for `cls`: per voxel the smallest linear index of its component within the item, every value labelled,
 * 0 included.  This library does not label.
 *
 * Remove small components: a component of a class k in 1 .. K - 1 with fewer than min_size[k] voxels becomes 0 (exactly min_size[k]
 * voxels stay: skimage.morphology.remove_small_objects); min_size[k] <= 1 leaves class k alone; class 0 and values outside [0, K)
 * are copied.  `labels` at the connectivity the components are meant in.
 *
 * Fill holes: a cavity is a component of value-0 voxels (`labels` at connectivity ch) without a voxel on the item's border (dims = 2:
 * y in {0, H - 1} or x in {0, W - 1}; dims = 3: the two z faces too).  Its contacts are the values of the non-zero voxels that are
 * ch-neighbours of one of its voxels.  A cavity whose contacts are one single class k in 1 .. K - 1 becomes k; one that touches two or
 * more classes of 1 .. K - 1 and nothing else is left and counted as mixed; one that touches a value outside [0, K) is left like
 * the background it cannot be told from.  Nothing non-zero is ever overwritten.  For K = 2 this is scipy.ndimage.binary_fill_holes
 * with generate_binary_structure(dims, ch).
 *
 * Conventions: raw DEVICE pointers (int64 arrays and the workspace 8-byte aligned, int32 arrays 4-byte aligned) except min_size, which
 * is HOST memory read during the call; `void* stream` = hipStream_t last; nothing allocated, no implicit synchronisation; 0 = OK,
 * -1 = bad argument, positive = hipError_t; pmor_last_error() returns a thread-local message; every argument is checked on the host
 * before anything is launched.  Limits: N >= 1, 1 <= K <= 32, 1 <= D <= 4096 (dims = 2: D = 1), 1 <= H, W <= 2048,
 * N * D * H * W < 2^31.  connectivity 1, 2 (dims = 2: 4 / 8 neighbours) or 1, 2, 3 (dims = 3: 6 / 18 / 26).  Integer atomics only, the
 * workspace is cleared here (hipMemsetAsync on the stream), the launch sequence depends on the shape alone: the same bits in every
 * run, whatever the stream or the workspace's previous content.  A label outside [0, own linear index] -- which no labeller writes
 * -- is never used as an index: that voxel is copied.
 */
#ifndef PACINGPSEUDO_MORPH_H
#define PACINGPSEUDO_MORPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100 * major + revision; bumped whenever an entry point is removed or changes its arguments.  The Python binding
 * (pacingpseudo_amd/_morph.py: MIN_MORPH_VERSION) refuses a library older than the header it was written against. */
int pmor_version(void);
const char* pmor_last_error(void);

/* pad8(4 * N * D * H * W): one 32-bit accumulator per voxel, used at the roots (component sizes, or contact masks).  0 for arguments
 * a call would refuse. */
size_t pmor_workspace(int N, int K, int D, int H, int W, int dims);

/* out int64 (N, D, H, W), may be cls itself.  stats int32 (N, K, 2) = {components removed, voxels removed} per item and class,
 * {0, 0} for class 0; cleared here. */
int pmor_remove_small(const int64_t* cls, const int32_t* labels, int N, int K, int D, int H, int W, int dims, const int32_t* min_size,
                      int64_t* out, int32_t* stats, void* workspace, size_t workspace_bytes, void* stream);

/* out int64 (N, D, H, W), may be cls itself.  stats int32 (N, K, 2): row k >= 1 = {cavities filled with k, voxels filled}, row 0 =
 * {cavities left because their contacts are two or more classes, their voxels}; cleared here. */
int pmor_fill_holes(const int64_t* cls, const int32_t* labels, int N, int K, int D, int H, int W, int dims, int connectivity,
                    int64_t* out, int32_t* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
