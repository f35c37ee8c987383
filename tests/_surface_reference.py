"""The oracle of the surface-metric tests, on numpy and scipy only.  Surfaces and both directed surface-distance sets are taken
exactly as ``oracle/pacing_oracle.py:compute_95hd`` takes them (medpy 0.4.0, metric/binary.py:__surface_distances restated:
border = mask XOR binary_erosion(mask, cross structure), distance_transform_edt(~other border, sampling=spacing) at the border);
from those float64 sets: hd (medpy's ``hd``: the maximum of both), assd (medpy's ``assd``: the mean of the two directed means),
the surface Dice at a tolerance, and ``numpy.percentile``.  Also here: a brute-force O(n^2) form of the sets for tiny masks, the
seeded maps of the GPU tests, and the contract of ``pp_surface_reduce`` restated on numpy."""
import numpy as np

SPACINGS = ((1.0, 1.0), (1.51, 1.51), (0.7, 2.3))
KEYS = ('hd', 'hdp', 'assd', 'nsd')


def is_scored(a, b):
    """inference.py:232 / :253: a class is skipped when the prediction or the label is empty or fills the image."""
    return bool(a.any() and b.any() and not a.all() and not b.all())


def directed_sets(a, b, spacing):
    """Boolean masks -> (distances from the surface of a to the surface of b, and back), float64."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    fp = generate_binary_structure(2, 1)
    ab = a ^ binary_erosion(a, structure=fp, iterations=1)
    bb = b ^ binary_erosion(b, structure=fp, iterations=1)
    d1 = distance_transform_edt(~bb, sampling=spacing)[ab]
    d2 = distance_transform_edt(~ab, sampling=spacing)[bb]
    return d1, d2


def brute_force_sets(a, b, spacing):
    """The same two sets by definition: a pixel of a mask is on its surface when one of its four neighbours is outside the mask or
    outside the image; every surface pixel looks at every surface pixel of the other mask."""
    def surface(m):
        H, W = m.shape
        pts = []
        for y in range(H):
            for x in range(W):
                if m[y, x] and not all(0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx] for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))):
                    pts.append((y, x))
        return np.array(pts, np.float64).reshape(-1, 2)
    sa, sb = surface(a) * np.asarray(spacing, np.float64), surface(b) * np.asarray(spacing, np.float64)
    d = np.sqrt(((sa[:, None, :] - sb[None, :, :]) ** 2).sum(-1))
    return d.min(1), d.min(0)


def metrics_of_sets(d1, d2, tolerance=2.0, percentile=95.0):
    s = np.hstack((d1, d2))
    return dict(hd=float(s.max()), hdp=float(np.percentile(s, percentile)), assd=float((d1.mean() + d2.mean()) / 2.0),
                nsd=float(((d1 <= tolerance).sum() + (d2 <= tolerance).sum()) / s.size))


def assert_tolerance_is_clear(sets, tolerance):
    """No oracle distance d has 0 < |d - tolerance| <= 1e-5 * tolerance: the fp32 distance of the device (within 1e-6 of d) then
    cannot fall on the other side of the threshold.  An exact hit stays one in fp32 (it occurs at spacing 1 only, where the
    value is an integer square root taken exactly)."""
    for d in sets:
        gap = np.abs(np.asarray(d, np.float64) - tolerance)
        near = (gap > 0) & (gap <= 1e-5 * tolerance)
        assert not near.any(), (tolerance, np.asarray(d)[near][:4])


def surface_metrics(pred, label, num_classes, spacing, tolerance=2.0, percentile=95.0, check_tolerance=True):
    """(H, W) class maps -> dict of (num_classes,) float64 arrays hd, hdp, assd, nsd; NaN for a skipped class."""
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


def batch_surface_metrics(pred, label, num_classes, spacing, tolerance=2.0, percentile=95.0):
    """(N, H, W) class maps -> dict of (N, num_classes) arrays."""
    rows = [surface_metrics(p, t, num_classes, spacing, tolerance, percentile) for p, t in zip(pred, label)]
    return {k: np.stack([r[k] for r in rows]) for k in KEYS}


def reduce_row(a, b, tolerance, percentile):
    """pp_surface_reduce's contract for one item on numpy: a, b the two sets (any float dtype; `<=` in that dtype)."""
    n = a.size + b.size
    if n == 0:
        return np.zeros(8)
    s = np.sort(np.hstack((a, b)))
    v = float(n - 1) * (percentile / 100.0)
    j = int(np.floor(v))
    tol = a.dtype.type(tolerance)
    return np.array([s[-1], a.astype(np.float64).sum(), b.astype(np.float64).sum(), (a <= tol).sum(), (b <= tol).sum(), s[j],
                     s[min(j + 1, n - 1)], n], np.float64)


# ---- the seeded maps of the end-to-end GPU test ----
SHAPES = ((2, 2), (1, 70), (70, 1), (37, 53), (64, 48), (96, 80))
KINDS = ('discs, 10 % label noise', 'discs, 50 % label noise', 'noise against noise', 'prediction = label')


def disc_phantom(shape, num_classes=5):
    """Ellipses of the classes 1 .. K-1 along the diagonal, in coordinates normalised to the shape: defined for a single row or
    column as well."""
    H, W = shape
    u = ((np.arange(H) + 0.5) / H)[:, None]
    v = ((np.arange(W) + 0.5) / W)[None, :]
    m = np.zeros(shape, np.int64)
    for c in range(1, num_classes):
        centre = c / num_classes
        m[((u - centre) / 0.16) ** 2 + ((v - centre) / 0.16) ** 2 < 1.0] = c
    return m


def seeded_maps(shape, num_classes=5):
    """-> (pred, label), each (4, H, W): one pair per entry of KINDS."""
    rng = np.random.default_rng(4000 + 100 * shape[0] + shape[1])
    base = disc_phantom(shape, num_classes)

    def noisy(m, share):
        m = m.copy()
        hit = rng.random(shape) < share
        m[hit] = rng.integers(0, num_classes, int(hit.sum()))
        return m
    label = [noisy(base, 0.1), noisy(base, 0.1), rng.integers(0, num_classes, shape), noisy(base, 0.1)]
    pred = [noisy(label[0], 0.1), noisy(label[1], 0.5), rng.integers(0, num_classes, shape), label[3].copy()]
    return np.stack(pred), np.stack(label)
