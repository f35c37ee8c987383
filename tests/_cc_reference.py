"""Oracle of the connected-component tests: scipy.ndimage restated in the canonical form of pp_label_components /
pp_keep_largest_components (include/pacingpseudo_hip.h), plus a brute-force flood fill that pins the restatement itself."""
import numpy as np
from scipy import ndimage


def structure(connectivity):
    return ndimage.generate_binary_structure(2, connectivity)


def canonical_labels(class_map, connectivity=1):
    """(H, W) integer map -> int32 (H, W): the smallest row-major index of every pixel's component.  Every distinct value is
    labelled on its own mask (scipy labels one binary mask at a time), background like any class."""
    cm = np.asarray(class_map)
    H, W = cm.shape
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    out = np.full((H, W), -1, np.int64)
    for v in np.unique(cm):
        lab, n = ndimage.label(cm == v, structure=structure(connectivity))
        if n:
            mins = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1))).astype(np.int64)
            mask = lab > 0
            out[mask] = mins[lab[mask] - 1]
    assert (out >= 0).all()
    return out.astype(np.int32)


def keep_largest(class_map, num_classes, connectivity=1):
    """-> (filtered map (same dtype), stats int32 (K, 2) = components before filtering, pixels kept).  The component kept is
    argmax(bincount(labels)[1:]): of equal sizes the first in scipy's numbering, which is raster order of the first pixel."""
    cm = np.asarray(class_map)
    out = cm.copy()
    stats = np.zeros((num_classes, 2), np.int32)
    for k in range(1, num_classes):
        lab, n = ndimage.label(cm == k, structure=structure(connectivity))
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel())[1:]
        keep = int(np.argmax(sizes)) + 1
        out[(lab > 0) & (lab != keep)] = 0
        stats[k] = (n, sizes[keep - 1])
    return out, stats


def flood_fill_labels(class_map, connectivity=1):
    """The definition, literally: an explicit stack per unvisited pixel in raster order (small maps only)."""
    cm = np.asarray(class_map)
    H, W = cm.shape
    if connectivity == 1:
        offs = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    else:
        offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    out = np.full((H, W), -1, np.int32)
    for y0 in range(H):
        for x0 in range(W):
            if out[y0, x0] >= 0:
                continue
            seed = y0 * W + x0                      # raster order: the first pixel reached is the component's minimum
            out[y0, x0] = seed
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in offs:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and out[yy, xx] < 0 and cm[yy, xx] == cm[y0, x0]:
                        out[yy, xx] = seed
                        stack.append((yy, xx))
    return out


def flood_fill_keep_largest(class_map, num_classes, connectivity=1):
    cm = np.asarray(class_map)
    lab = flood_fill_labels(cm, connectivity)
    out = cm.copy()
    stats = np.zeros((num_classes, 2), np.int32)
    for k in range(1, num_classes):
        ids, sizes = np.unique(lab[cm == k], return_counts=True)        # ascending labels: argmax takes the smallest of a tie
        if len(ids) == 0:
            continue
        keep = ids[int(np.argmax(sizes))]
        out[(cm == k) & (lab != keep)] = 0
        stats[k] = (len(ids), sizes.max())
    return out, stats


def serpentine(H, W):
    """Every second row filled, rows joined alternately at the right and the left end: one 4-connected component."""
    m = np.zeros((H, W), np.int64)
    m[0::2, :] = 1
    for i, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    """Teeth in every second column, joined only along the bottom row."""
    m = np.zeros((H, W), np.int64)
    m[:, 0::2] = 1
    m[H - 1, :] = 1
    return m
