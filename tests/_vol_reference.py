"""Oracle of the volume-wise evaluation tests, on numpy and scipy only: scipy.ndimage restated in the canonical form of
include/pacingpseudo_vol.h.  Every function works on an array of any rank (generate_binary_structure(ndim, .)), so a single slice
handed over as a 2-D array must agree with tests/_cc_reference.py and tests/_surface_reference.py -- tests/test_vol.py checks that."""
import numpy as np
from scipy import ndimage

KEYS = ('hd', 'hdp', 'assd', 'nsd')


def structure(ndim, connectivity):
    return ndimage.generate_binary_structure(ndim, connectivity)


def canonical_labels(class_map, connectivity=1):
    """Integer array -> int32 array: the smallest linear (C-order) index of every element's component.  Every distinct value is
    labelled on its own mask, 0 like any other."""
    cm = np.asarray(class_map)
    index = np.arange(cm.size, dtype=np.int64).reshape(cm.shape)
    out = np.full(cm.shape, -1, np.int64)
    for v in np.unique(cm):
        lab, n = ndimage.label(cm == v, structure=structure(cm.ndim, connectivity))
        if n:
            mins = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1))).astype(np.int64)
            mask = lab > 0
            out[mask] = mins[lab[mask] - 1]
    assert (out >= 0).all()
    return out.astype(np.int32)


def keep_largest(class_map, num_classes, connectivity=1):
    """-> (filtered map (same dtype), stats int32 (K, 2) = components before filtering, voxels removed).  The component kept is
    argmax(bincount(labels)[1:]): of equal sizes the first in scipy's numbering, which is the order of the components' first
    elements -- the smallest canonical label."""
    cm = np.asarray(class_map)
    out = cm.copy()
    stats = np.zeros((num_classes, 2), np.int32)
    for k in range(1, num_classes):
        lab, n = ndimage.label(cm == k, structure=structure(cm.ndim, connectivity))
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel())[1:]
        keep = int(np.argmax(sizes)) + 1
        out[(lab > 0) & (lab != keep)] = 0
        stats[k] = (n, int(sizes.sum() - sizes[keep - 1]))
    return out, stats


def edt(mask, spacing=None):
    """float64 distance_transform_edt; +inf everywhere when the array has no zero element (scipy's values there mean nothing)."""
    m = np.asarray(mask) != 0
    if m.all():
        return np.full(m.shape, np.inf)
    return ndimage.distance_transform_edt(m, sampling=spacing)


def edt_squared_int(mask):
    """Unit spacing: the squared distances as exact integers (-1: no zero element), from scipy's nearest-zero indices."""
    m = np.asarray(mask) != 0
    if m.all():
        return np.full(m.shape, -1, np.int64)
    idx = ndimage.distance_transform_edt(m, return_distances=False, return_indices=True)
    grid = np.indices(m.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(0)


def is_scored(a, b):
    """A class is skipped when the prediction or the label is empty or fills the array (inference.py:232)."""
    return bool(a.any() and b.any() and not a.all() and not b.all())


def surfaces(a, b):
    """medpy 0.4.0 metric/binary.py:__surface_distances with connectivity 1: mask XOR binary_erosion(mask, cross), outside = 0."""
    fp = structure(a.ndim, 1)
    return a ^ ndimage.binary_erosion(a, structure=fp, iterations=1), b ^ ndimage.binary_erosion(b, structure=fp, iterations=1)


def directed_sets(a, b, spacing):
    """Boolean arrays -> (distances from the surface of a to the surface of b, and back), float64, each in C order of its own
    surface elements.  A surface that does not exist gives +inf distances to it."""
    ab, bb = surfaces(a, b)
    return edt(~bb, spacing)[ab], edt(~ab, spacing)[bb]


def metrics_of_sets(d1, d2, tolerance=2.0, percentile=95.0):
    s = np.hstack((d1, d2))
    return dict(hd=float(s.max()), hdp=float(np.percentile(s, percentile)), assd=float((d1.mean() + d2.mean()) / 2.0),
                nsd=float(((d1 <= tolerance).sum() + (d2 <= tolerance).sum()) / s.size))


def assert_tolerance_is_clear(sets, tolerance):
    """No oracle distance d has 0 < |d - tolerance| <= 1e-5 * tolerance (as tests/_surface_reference.py): the device's fp32 distance,
    within 1e-6 of d, then cannot fall on the other side of the threshold."""
    for d in sets:
        gap = np.abs(np.asarray(d, np.float64) - tolerance)
        near = (gap > 0) & (gap <= 1e-5 * tolerance)
        assert not near.any(), (tolerance, np.asarray(d)[near][:4])


def surface_metrics(pred, label, num_classes, spacing, tolerance=2.0, percentile=95.0, check_tolerance=True):
    """Class maps of any rank -> dict of (num_classes,) float64 arrays hd, hdp, assd, nsd; NaN for a skipped class."""
    out = {k: np.full(num_classes, np.nan) for k in KEYS}
    for c in range(num_classes):
        a, b = pred == c, label == c
        if not is_scored(a, b):
            continue
        d1, d2 = directed_sets(a, b, spacing)
        if check_tolerance:
            assert_tolerance_is_clear((d1, d2), tolerance)
        for k, v in metrics_of_sets(d1, d2, tolerance, percentile).items():
            out[k][c] = v
    return out


def dice(pred, label, num_classes):
    """inference.py:205-216 on element counts: 2 |P & T| / max(|P| + |T|, 1e-8), NaN where both are empty."""
    out = np.full(num_classes, np.nan)
    for c in range(num_classes):
        a, b = pred == c, label == c
        if a.any() or b.any():
            out[c] = 2.0 * float((a & b).sum()) / max(float(a.sum() + b.sum()), 1e-8)
    return out


# ---- shapes of the GPU tests ----
def serpentine_3d(D, H, W):
    """One path, one voxel wide, of value 1: in every second slice every second row is filled and the rows are joined alternately at
    the right and the left end (tests/_cc_reference.py:serpentine); the slices are joined through single voxels of the slices between
    them, alternately above the path's end in the last filled row and above its start (0, 0).  One 6-connected component that
    crosses every brick face many times; its minimum index, voxel 0, is one END of the path."""
    m = np.zeros((D, H, W), np.int64)
    joints = [y for y in range(1, H, 2) if y + 1 < H]
    end = (2 * len(joints), W - 1 if len(joints) % 2 == 0 else 0)          # where the walk from (0, 0) through a slice ends
    for i, z in enumerate(range(0, D, 2)):
        m[z, 0::2, :] = 1
        for j, y in enumerate(joints):
            m[z, y, W - 1 if j % 2 == 0 else 0] = 1
        if z + 2 < D:
            y, x = end if i % 2 == 0 else (0, 0)
            m[z + 1, y, x] = 1
    return m


def blobs_3d(D, H, W, K, seed, count=None):
    """Ellipsoids of the classes 1 .. K-1 dropped at random: a class map int64 (D, H, W)."""
    rng = np.random.RandomState(seed)
    cm = np.zeros((D, H, W), np.int64)
    zz, yy, xx = np.indices((D, H, W))
    for i in range(count or 3 * K):
        k = 1 + i % (K - 1) if K > 1 else 0
        cz, cy, cx = rng.randint(D), rng.randint(H), rng.randint(W)
        rz, ry, rx = rng.randint(1, max(D // 2, 2)), rng.randint(2, max(H // 3, 3)), rng.randint(2, max(W // 3, 3))
        cm[((zz - cz) / rz) ** 2 + ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return cm
