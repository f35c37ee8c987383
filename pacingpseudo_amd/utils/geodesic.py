"""Geodesic-distance expansion of scribbles on the GPU (GeoS, Criminisi et al. 2008; DeepIGeoS, Wang et al. 2018; PA-Seg, Zhai et al.
2023).  The reference trains on the scribbles as they are on disk; this is an addition, off by default (``train_chaos.py
--geo_scribbles``, ``scripts/expand_scribbles.py --method geo``).  Like the random walker it acts on the LABELS, once per slice,
before the first step: a pixel takes the class of the seed it can reach without crossing an intensity edge.

For a slice of true size h x w inside a padded H x W plane, with scribble values 0 .. K (K = unlabelled)::

    g       = (img - mean) / (std + 1e-8)                 mean, population std over the slice's own h x w pixels (the walker's)
    c(p, q) = fl(s + fl(lam |fl(g_p - g_q)|))             8-neighbours inside h x w; s = 1 along the axes, 1.41421354f diagonally
    dist[k] = the least fixed point of d(q) = min(d0(q), min_p fl(d(p) + c(p, q))),  d0 = 0 on scb == k, +inf elsewhere
    label   = the first arg-min k where D_best is finite, <= max_dist and <= fl(ratio D_second), else K; seeds keep their class

Every operation is rounded to fp32 on its own, a candidate replaces a value only when it is smaller (NaN pixels are walls), and
because fl(x + c) is monotone in x the fixed point is unique BIT FOR BIT: it is what a float32 Dijkstra gives, whatever order the
device relaxes pixels in.  dist[k] is +inf for a class without a seed and outside h x w.  ``lam = 20``, ``ratio = 0.25`` and
``max_dist = inf`` are untuned first values, checked on the 64 x 64 five-class synthetic phantoms of the tests only (DESIGN.md
section 7).  libpacingpseudo_geo.so, include/pacingpseudo_geo.h; no CPU path."""
import math

import numpy as np
import torch

from .._lib import stream_ptr

GEO_MAX_CLASSES = 32
GEO_MAX_SIZE = 1024
GEO_BATCH = 32             # slices per call of expand_dataset_geo


def check_geo_params(lam=20.0, ratio=0.25, max_dist=math.inf, max_sweeps=100000, K=None) -> dict:
    """The accepted ranges of pgeo_distance / pgeo_labels, checked before any launch: ValueError for values that are no edge
    weight / ratio / distance / count at all, NotImplementedError for a count beyond what the kernels run.  Returns the normalised
    parameters."""
    if isinstance(max_sweeps, bool) or isinstance(max_sweeps, float) and not math.isfinite(max_sweeps) or int(max_sweeps) != max_sweeps:
        raise ValueError(f'geodesic scribbles: max_sweeps must be an integer (got {max_sweeps!r})')
    for v, what in ((lam, 'lam'), (ratio, 'ratio'), (max_dist, 'max_dist')):
        if isinstance(v, bool):
            raise ValueError(f'geodesic scribbles: {what} must be a number (got {v!r})')
    lam, ratio, max_dist, max_sweeps = float(lam), float(ratio), float(max_dist), int(max_sweeps)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f'geodesic scribbles: lam must be a finite number >= 0 (got {lam!r})')
    if not (0.0 < ratio <= 1.0):
        raise ValueError(f'geodesic scribbles: ratio must lie in (0, 1] (got {ratio!r})')
    if not max_dist > 0.0:
        raise ValueError(f'geodesic scribbles: max_dist must be > 0, inf allowed (got {max_dist!r})')
    if max_sweeps < 1:
        raise ValueError(f'geodesic scribbles: max_sweeps must be >= 1 (got {max_sweeps})')
    if max_sweeps >= 2 ** 31:
        raise NotImplementedError(f'geodesic scribbles: max_sweeps < 2^31 (got {max_sweeps})')
    if K is not None:
        if isinstance(K, bool) or int(K) != K or int(K) < 1:
            raise ValueError(f'geodesic scribbles: the class count must be an integer >= 1 (got {K!r})')
        if int(K) > GEO_MAX_CLASSES:
            raise NotImplementedError(f'geodesic scribbles: K <= {GEO_MAX_CLASSES} classes (got {K})')
    return dict(lam=lam, ratio=ratio, max_dist=max_dist, max_sweeps=max_sweeps)


def add_geo_flags(parser) -> None:
    """--geo_scribbles and its parameters (train_chaos.py only: the fully-supervised driver trains on full labels)."""
    parser.add_argument('--geo_scribbles', action='store_true',
                        help='expand every training slice\'s scribbles ONCE before the first step by geodesic distance on the '
                             'normalised image (a pixel takes the class of the seed it reaches without crossing an intensity edge, '
                             'the ignore index where no class is clearly nearest); nothing runs per step, validation data are untouched')
    parser.add_argument('--geo_lambda', type=float, default=20.0,
                        help='a step between neighbours costs its length + lambda |g_p - g_q| on the normalised image, lambda >= 0 '
                             '(an untuned first value)')
    parser.add_argument('--geo_ratio', type=float, default=0.25,
                        help='a pixel takes the nearest class where its distance is at most this times the distance of the runner-up, '
                             'in (0, 1] (an untuned first value)')
    parser.add_argument('--geo_max_dist', type=float, default=math.inf,
                        help='... and at most this, > 0 (an untuned first value: inf = no limit)')
    parser.add_argument('--geo_max_sweeps', type=int, default=100000, help='cap of the passes over a plane, >= 1')


def _inputs(image, scribble, num_classes, sizes):
    """(img (N, H, W) fp32, scb (N, H, W) int32, host sizes array or None, K), every check made before the library is touched."""
    for x, what in ((image, 'image'), (scribble, 'scribble')):
        if not torch.is_tensor(x):
            raise TypeError(f'{what} must be a torch tensor, got {type(x).__name__}')
        if not x.is_cuda:
            raise TypeError(f'{what} must be a CUDA tensor: the geodesic transform has no CPU path')
    if image.dtype != torch.float32:
        raise TypeError(f'image must be float32, got {image.dtype}')
    if scribble.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise TypeError(f'scribble must be an integer class map, got {scribble.dtype}')
    if image.dim() == 4 and image.shape[1] == 1:
        image = image[:, 0]
    if image.dim() != 3:
        raise ValueError(f'image must be (N, H, W) or (N, 1, H, W), got {tuple(image.shape)}')
    if tuple(scribble.shape) != tuple(image.shape):
        raise ValueError(f'scribble must be (N, H, W) = {tuple(image.shape)}, got {tuple(scribble.shape)}')
    if scribble.device != image.device:
        raise ValueError(f'scribble is on {scribble.device}, image on {image.device}')
    N, H, W = image.shape
    if min(N, H, W) < 1:
        raise ValueError(f'image has an empty axis: {tuple(image.shape)}')
    check_geo_params(K=num_classes)
    K = int(num_classes)
    if H > GEO_MAX_SIZE or W > GEO_MAX_SIZE:
        raise NotImplementedError(f'geodesic scribbles: planes up to {GEO_MAX_SIZE} x {GEO_MAX_SIZE} (got {H} x {W})')
    if N * K * H * W >= 2 ** 31:
        raise NotImplementedError(f'geodesic scribbles: N * K * H * W < 2^31 (got {N} x {K} x {H} x {W})')
    host_sizes = None
    if sizes is not None:
        sz = [(int(h), int(w)) for h, w in sizes]
        if len(sz) != N:
            raise ValueError(f'sizes must hold one (h, w) per slice: {N}, got {len(sz)}')
        for n, (h, w) in enumerate(sz):
            if not (1 <= h <= H and 1 <= w <= W):
                raise ValueError(f'sizes[{n}] = ({h}, {w}) does not lie inside the {H} x {W} plane')
        host_sizes = np.ascontiguousarray(np.asarray(sz, dtype=np.int32).reshape(N, 2))
    lo, hi = torch.aminmax(scribble)
    if int(lo) < 0 or int(hi) > K:
        raise ValueError(f'scribble values must lie in 0 .. {K} (K = unlabelled), got {int(lo)} .. {int(hi)}')
    return image.contiguous(), scribble.to(torch.int32).contiguous(), host_sizes, K


def _sizes_ptr(host_sizes):
    import ctypes
    return None if host_sizes is None else host_sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _guide(img, host_sizes, normalize):
    if not normalize:
        return img
    from .._geo import geo
    N, H, W = img.shape
    g = torch.empty_like(img)
    with torch.cuda.device(img.device):
        geo.pgeo_normalize(img.data_ptr(), _sizes_ptr(host_sizes), N, H, W, g.data_ptr(), stream_ptr())
    return g


def _distance(g, scb, host_sizes, K, prm):
    from .._geo import geo
    N, H, W = g.shape
    dist = torch.empty((N, K, H, W), device=g.device, dtype=torch.float32)
    stats = torch.empty((N, K, 2), device=g.device, dtype=torch.int32)
    nbytes = geo.pgeo_distance_workspace(N, K, H, W)
    ws = torch.empty(nbytes, device=g.device, dtype=torch.uint8)
    with torch.cuda.device(g.device):
        geo.pgeo_distance(g.data_ptr(), scb.data_ptr(), _sizes_ptr(host_sizes), N, K, H, W, prm['lam'], prm['max_sweeps'],
                          dist.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, stream_ptr())
    return dist, stats


def _labels(dist, scb, host_sizes, K, prm):
    from .._geo import geo
    N, H, W = scb.shape
    out = torch.empty((N, H, W), device=scb.device, dtype=torch.int32)
    with torch.cuda.device(scb.device):
        geo.pgeo_labels(dist.data_ptr(), scb.data_ptr(), _sizes_ptr(host_sizes), N, K, H, W, prm['max_dist'], prm['ratio'],
                        out.data_ptr(), stream_ptr())
    return out


def geodesic_distance(image, scribble, num_classes, sizes=None, *, lam=20.0, max_sweeps=100000, normalize=True, return_stats=False,
                      return_guide=False):
    """Geodesic distances to the seeds of every class (the module docstring has the definition).  `image` is (N, H, W) or
    (N, 1, H, W) fp32 CUDA: raw intensities, normalised per slice on the device; with ``normalize=False`` it is the guide itself.
    `scribble` is an (N, H, W) integer CUDA map with values 0 .. K, `sizes` an optional list of N (h, w): the true size of each
    slice in the top-left corner of its plane.  Returns dist (N, K, H, W) fp32; with ``return_stats`` also stats (N, K, 2) int32 =
    (passes over the plane, converged), with ``return_guide`` also the guide (N, H, W).  Runs on the current stream."""
    prm = check_geo_params(lam=lam, max_sweeps=max_sweeps)
    img, scb, host_sizes, K = _inputs(image, scribble, num_classes, sizes)
    g = _guide(img, host_sizes, normalize)
    dist, stats = _distance(g, scb, host_sizes, K, prm)
    out = (dist,) + ((stats,) if return_stats else ()) + ((g,) if return_guide else ())
    return out if len(out) > 1 else dist


def geodesic_expand_scribbles(image, scribble, num_classes, sizes=None, *, lam=20.0, ratio=0.25, max_dist=math.inf, max_sweeps=100000,
                              normalize=True, return_stats=False, return_dist=False):
    """Dense pseudo-labels from scribbles: ``geodesic_distance`` followed by the ratio rule.  Returns labels (N, H, W) with the
    dtype of `scribble`: the nearest class where its distance is finite, <= `max_dist` and <= `ratio` x the runner-up's, K elsewhere
    and outside h x w; seeds keep their class.  With ``return_stats`` / ``return_dist`` a tuple (labels[, stats][, dist])."""
    prm = check_geo_params(lam, ratio, max_dist, max_sweeps)
    img, scb, host_sizes, K = _inputs(image, scribble, num_classes, sizes)
    dist, stats = _distance(_guide(img, host_sizes, normalize), scb, host_sizes, K, prm)
    labels = _labels(dist, scb, host_sizes, K, prm).to(scribble.dtype)
    out = (labels,) + ((stats,) if return_stats else ()) + ((dist,) if return_dist else ())
    return out if len(out) > 1 else labels


# ---- a whole data set, once (the training driver and scripts/expand_scribbles.py --method geo) -------------------------------------
def expand_dataset_geo(dataset, num_classes, device, prm, keep_mindist=False):
    """Expand every slice of a ``data.NpzSlices`` (or ``SyntheticPhantoms``) data set, batched as ``random_walker.expand_dataset``:
    raw items in index order, runs of consecutive slices of equal shape, at most GEO_BATCH per call.  Returns ``(maps, report)``:
    `maps` the per-index list of uint8 (h, w) label maps (what ``dataset.scribble_override`` takes), `report` a dict of per-slice
    numpy arrays -- sweeps / converged (n, K), coverage_before / coverage_after (n) = labelled share of the pixels, agreement (n) =
    share of the NEWLY labelled pixels whose label equals `lab` (NaN without any), and with `keep_mindist` mindist, a list of
    float16 (h, w) maps of the smallest distance over the classes.  Deterministic: every caller gets the same bits."""
    K, n = int(num_classes), len(dataset)
    if K > 255:
        raise NotImplementedError('the expanded maps are kept as uint8')
    maps, mindist = [None] * n, [None] * n
    rep = dict(sweeps=np.zeros((n, K), np.int32), converged=np.ones((n, K), bool), coverage_before=np.zeros(n),
               coverage_after=np.zeros(n), agreement=np.full(n, np.nan))

    def flush(idx, items):
        img = torch.from_numpy(np.stack([np.asarray(it[0], dtype=np.float32) for it in items])).to(device)
        scb_h = np.stack([np.asarray(it[2]).astype(np.uint8) for it in items])
        res = geodesic_expand_scribbles(img, torch.from_numpy(scb_h).to(device), K, None, lam=prm['lam'], ratio=prm['ratio'],
                                        max_dist=prm['max_dist'], max_sweeps=prm['max_sweeps'], return_stats=True,
                                        return_dist=keep_mindist)
        lab_new, st = res[0].cpu().numpy(), res[1].cpu().numpy()
        md = res[2].amin(1).to(torch.float16).cpu().numpy() if keep_mindist else None
        for j, i in enumerate(idx):
            maps[i] = np.ascontiguousarray(lab_new[j])
            if keep_mindist:
                mindist[i] = md[j]
            rep['sweeps'][i], rep['converged'][i] = st[j, :, 0], st[j, :, 1] > 0
            new = (scb_h[j] == K) & (lab_new[j] != K)
            rep['coverage_before'][i] = float((scb_h[j] != K).mean())
            rep['coverage_after'][i] = float((lab_new[j] != K).mean())
            if new.any():
                rep['agreement'][i] = float((lab_new[j][new] == np.asarray(items[j][1])[new]).mean())

    idx, items = [], []
    for i in range(n):
        it = dataset.raw_arrays(i)
        if items and (len(items) == GEO_BATCH or it[0].shape != items[0][0].shape):
            flush(idx, items)
            idx, items = [], []
        idx.append(i)
        items.append(it)
    if items:
        flush(idx, items)
    if keep_mindist:
        rep['mindist'] = mindist
    return maps, rep


def summarize_geo(rep) -> dict:
    """The figures of the summary line from an expand_dataset_geo report."""
    agree = rep['agreement'][~np.isnan(rep['agreement'])]
    bad = np.nonzero(~rep['converged'].all(1))[0]
    return dict(slices=int(len(rep['coverage_before'])), coverage_before=float(rep['coverage_before'].mean()),
                coverage_after=float(rep['coverage_after'].mean()), agreement=float(agree.mean()) if len(agree) else float('nan'),
                max_sweeps=int(rep['sweeps'].max()), unconverged=int((~rep['converged']).sum()),
                unconverged_slices=[int(i) for i in bad])


def summary_line_geo(s) -> str:
    return (f'geodesic scribbles: {s["slices"]} slices, mean coverage {100 * s["coverage_before"]:.2f} % -> '
            f'{100 * s["coverage_after"]:.2f} %, agreement with lab on newly labelled pixels {100 * s["agreement"]:.2f} %; '
            f'largest pass count {s["max_sweeps"]}, {s["unconverged"]} unconverged planes')
