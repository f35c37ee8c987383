"""Random-walker expansion of scribbles on the GPU (Grady 2006; used for scribble-supervised segmentation by Can et al. 2018, the
"RW" row of the WSL4MIS benchmark).  The reference trains on the scribbles as they are on disk; this is an addition, off by
default (``train_chaos.py --rw_scribbles``, ``scripts/expand_scribbles.py``).  It acts on the LABELS, once per slice, before the
first step: scribbles plus image become dense pseudo-labels, and everything downstream consumes them as an ordinary scribble map
with its ignore index.

For a slice of true size h x w inside a padded H x W plane, with scribble values 0 .. K (K = unlabelled)::

    g    = (img - mean) / (std + 1e-8)                  mean, population std over the slice's own h x w pixels
    w_ij = exp(-beta (g_i - g_j)^2) + eps                4-neighbour grid inside h x w
    L_UU x_k = b_k                                      U = {scb == K}, S = {scb < K}, for every class k with a seed
    (L_UU)_ii = sum_{j~i} w_ij,  (L_UU)_ij = -w_ij,  (b_k)_i = sum_{j~i, j in S, scb_j = k} w_ij
    prob[k] = x_k on U, one-hot of scb on S; exactly 0 for a class without a seed and outside h x w
    label   = argmax_k prob (first maximum) where max_k prob >= threshold, else K; seeds keep their class; K outside h x w

``beta = 13`` is skimage's default ``beta = 130`` under its ``beta / (10 std)`` scaling for a unit-variance image; ``eps`` keeps the
grid connected and bounds the conditioning for fp32.  ``beta``, ``eps`` and ``threshold`` are untuned first values.  The solver
(libpacingpseudo_prep.so, include/pacingpseudo_prep.h) is Jacobi-preconditioned conjugate gradients in fp32 with dot products in
double, one workgroup per (slice, class); results are the same bits in every run and whatever the batch.  No CPU path.

The second half of this file re-runs the walker during training with the network's soft-max as a unary prior
(``random_walker_prior``, ``refresh_scribbles``, ``refresh_dataset``, ``SharedMaps``; ``train_chaos.py --rw_refresh``)."""
import math

import numpy as np
import torch

from .._lib import stream_ptr

RW_MAX_CLASSES = 32
RW_MAX_SIZE = 1024
RW_BATCH = 32              # slices per call of expand_dataset


def check_rw_params(beta=13.0, eps=1e-4, tol=1e-6, max_iters=10000, threshold=0.9, K=None) -> dict:
    """The accepted ranges of pprep_rw_solve / pprep_rw_labels, checked before any launch: ValueError for values that are no weight
    scale / tolerance / count / probability at all, NotImplementedError for a class count beyond what the kernels run.  Returns
    the normalised parameters."""
    if isinstance(max_iters, bool) or int(max_iters) != max_iters:
        raise ValueError(f'random walker: max_iters must be an integer (got {max_iters!r})')
    beta, eps, tol, max_iters, threshold = float(beta), float(eps), float(tol), int(max_iters), float(threshold)
    if not (beta >= 0.0 and math.isfinite(beta)):
        raise ValueError(f'random walker: beta must be a finite number >= 0 (got {beta!r})')
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f'random walker: eps must be a positive finite number (got {eps!r})')
    if not (tol > 0.0 and math.isfinite(tol)):
        raise ValueError(f'random walker: tol must be a positive finite number (got {tol!r})')
    if max_iters < 1:
        raise ValueError(f'random walker: max_iters must be >= 1 (got {max_iters})')
    if max_iters >= 2 ** 31:
        raise NotImplementedError(f'random walker: max_iters < 2^31 (got {max_iters})')
    if not (0.0 < threshold <= 1.0):
        raise ValueError(f'random walker: threshold must lie in (0, 1] (got {threshold!r})')
    if K is not None:
        if isinstance(K, bool) or int(K) != K or int(K) < 1:
            raise ValueError(f'random walker: the class count must be an integer >= 1 (got {K!r})')
        if int(K) > RW_MAX_CLASSES:
            raise NotImplementedError(f'random walker: K <= {RW_MAX_CLASSES} classes (got {K})')
    return dict(beta=beta, eps=eps, tol=tol, max_iters=max_iters, threshold=threshold)


def add_rw_flags(parser) -> None:
    """--rw_scribbles and its parameters (train_chaos.py only: the fully-supervised driver trains on full labels)."""
    parser.add_argument('--rw_scribbles', action='store_true',
                        help='expand every training slice\'s scribbles ONCE before the first step with the random walker (dense '
                             'pseudo-labels where the walker is confident, the ignore index elsewhere); nothing runs per step, '
                             'validation data are untouched')
    parser.add_argument('--rw_beta', type=float, default=13.0,
                        help='edge weights exp(-beta (g_i - g_j)^2) + eps on the normalised image, beta >= 0 (an untuned first value: '
                             'skimage\'s default for a unit-variance image)')
    parser.add_argument('--rw_threshold', type=float, default=0.9,
                        help='a pixel takes the walker\'s class where its probability is at least this, in (0, 1] (an untuned first value)')
    parser.add_argument('--rw_eps', type=float, default=1e-4, help='floor of the edge weights, > 0 (an untuned first value)')
    parser.add_argument('--rw_tol', type=float, default=1e-6, help='relative residual at which the conjugate-gradient solver stops, > 0')
    parser.add_argument('--rw_max_iters', type=int, default=10000, help='iteration cap of the solver, >= 1')


def _inputs(image, scribble, num_classes, sizes):
    """(img (N, H, W) fp32, scb (N, H, W) int32, host sizes array or None, K), every check made before the library is touched."""
    for x, what in ((image, 'image'), (scribble, 'scribble')):
        if not torch.is_tensor(x):
            raise TypeError(f'{what} must be a torch tensor, got {type(x).__name__}')
        if not x.is_cuda:
            raise TypeError(f'{what} must be a CUDA tensor: the random walker has no CPU path')
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
    check_rw_params(K=num_classes)
    K = int(num_classes)
    if H > RW_MAX_SIZE or W > RW_MAX_SIZE:
        raise NotImplementedError(f'random walker: planes up to {RW_MAX_SIZE} x {RW_MAX_SIZE} (got {H} x {W})')
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


def _solve(img, scb, host_sizes, K, prm):
    from .._prep import prep
    N, H, W = img.shape
    prob = torch.empty((N, K, H, W), device=img.device, dtype=torch.float32)
    stats = torch.empty((N, K, 3), device=img.device, dtype=torch.float32)
    ws = torch.empty(prep.pprep_rw_workspace_bytes(N, K, H, W), device=img.device, dtype=torch.uint8)
    with torch.cuda.device(img.device):
        prep.pprep_rw_solve(img.data_ptr(), scb.data_ptr(), _sizes_ptr(host_sizes), N, K, H, W, prm['beta'], prm['eps'], prm['tol'],
                            prm['max_iters'], prob.data_ptr(), stats.data_ptr(), ws.data_ptr(), stream_ptr())
    return prob, stats


def _labels(prob, scb, host_sizes, K, threshold):
    from .._prep import prep
    N, H, W = scb.shape
    out = torch.empty((N, H, W), device=scb.device, dtype=torch.int32)
    with torch.cuda.device(scb.device):
        prep.pprep_rw_labels(prob.data_ptr(), scb.data_ptr(), _sizes_ptr(host_sizes), N, K, H, W, threshold, out.data_ptr(), stream_ptr())
    return out


def random_walker(image, scribble, num_classes, sizes=None, *, beta=13.0, eps=1e-4, tol=1e-6, max_iters=10000, return_stats=False):
    """Random-walker probabilities (the module docstring has the definition).  `image` is (N, H, W) or (N, 1, H, W) fp32 CUDA (raw
    intensities: the normalisation is part of the definition), `scribble` an (N, H, W) integer CUDA map with values 0 .. K, `sizes`
    an optional list of N (h, w): the true size of each slice in the top-left corner of its plane.  Returns prob (N, K, H, W)
    fp32, with ``return_stats`` also stats (N, K, 3) fp32 = (iterations, true relative residual, converged) per system.  Runs on
    the current stream."""
    prm = check_rw_params(beta, eps, tol, max_iters)
    img, scb, host_sizes, K = _inputs(image, scribble, num_classes, sizes)
    prob, stats = _solve(img, scb, host_sizes, K, prm)
    return (prob, stats) if return_stats else prob


def expand_scribbles(image, scribble, num_classes, sizes=None, threshold=0.9, *, beta=13.0, eps=1e-4, tol=1e-6, max_iters=10000,
                     return_stats=False, return_prob=False):
    """Dense pseudo-labels from scribbles: ``random_walker`` followed by the thresholded first-maximum arg-max.  Returns labels
    (N, H, W) with the dtype of `scribble`: the walker's class where its probability is >= `threshold`, K elsewhere and outside
    h x w; seeds keep their class.  With ``return_stats`` / ``return_prob`` a tuple (labels[, stats][, prob])."""
    prm = check_rw_params(beta, eps, tol, max_iters, threshold)
    img, scb, host_sizes, K = _inputs(image, scribble, num_classes, sizes)
    prob, stats = _solve(img, scb, host_sizes, K, prm)
    labels = _labels(prob, scb, host_sizes, K, prm['threshold']).to(scribble.dtype)
    out = (labels,) + ((stats,) if return_stats else ()) + ((prob,) if return_prob else ())
    return out if len(out) > 1 else labels


# ---- a whole data set, once (the training driver and scripts/expand_scribbles.py) ----------------------------------------------
def expand_dataset(dataset, num_classes, device, prm, keep_maxprob=False):
    """Expand every slice of a ``data.NpzSlices`` (or ``SyntheticPhantoms``) data set: raw items are read in index order and runs of
    consecutive slices of equal shape, at most RW_BATCH, go through one ``expand_scribbles`` call.  Returns ``(maps, report)``:
    `maps` the per-index list of uint8 (h, w) label maps (what ``dataset.scribble_override`` takes), `report` a dict of per-slice
    numpy arrays -- iterations / relres / converged (n, K), coverage_before / coverage_after (n) = labelled share of the pixels,
    agreement (n) = share of the NEWLY labelled pixels whose label equals `lab` (NaN without any), and with `keep_maxprob`
    maxprob, a list of float16 (h, w) maps.  Deterministic: every caller gets the same bits."""
    K, n = int(num_classes), len(dataset)
    if K > 255:
        raise NotImplementedError('the expanded maps are kept as uint8')
    maps, maxprob = [None] * n, [None] * n
    rep = dict(iterations=np.zeros((n, K), np.int32), relres=np.zeros((n, K), np.float32), converged=np.ones((n, K), bool),
               coverage_before=np.zeros(n), coverage_after=np.zeros(n), agreement=np.full(n, np.nan))

    def flush(idx, items):
        img = torch.from_numpy(np.stack([np.asarray(it[0], dtype=np.float32) for it in items])).to(device)
        scb_h = np.stack([np.asarray(it[2]).astype(np.uint8) for it in items])
        res = expand_scribbles(img, torch.from_numpy(scb_h).to(device), K, None, prm['threshold'], beta=prm['beta'], eps=prm['eps'],
                               tol=prm['tol'], max_iters=prm['max_iters'], return_stats=True, return_prob=keep_maxprob)
        lab_new, st = res[0].cpu().numpy(), res[1].cpu().numpy()
        mp = res[2].amax(1).to(torch.float16).cpu().numpy() if keep_maxprob else None
        for j, i in enumerate(idx):
            maps[i] = np.ascontiguousarray(lab_new[j])
            if keep_maxprob:
                maxprob[i] = mp[j]
            rep['iterations'][i], rep['relres'][i], rep['converged'][i] = st[j, :, 0], st[j, :, 1], st[j, :, 2] > 0.5
            new = (scb_h[j] == K) & (lab_new[j] != K)
            rep['coverage_before'][i] = float((scb_h[j] != K).mean())
            rep['coverage_after'][i] = float((lab_new[j] != K).mean())
            if new.any():
                rep['agreement'][i] = float((lab_new[j][new] == np.asarray(items[j][1])[new]).mean())

    idx, items = [], []
    for i in range(n):
        it = dataset.raw_arrays(i)
        if items and (len(items) == RW_BATCH or it[0].shape != items[0][0].shape):
            flush(idx, items)
            idx, items = [], []
        idx.append(i)
        items.append(it)
    if items:
        flush(idx, items)
    if keep_maxprob:
        rep['maxprob'] = maxprob
    return maps, rep


def summarize(rep) -> dict:
    """The figures of the summary line from an expand_dataset report."""
    agree = rep['agreement'][~np.isnan(rep['agreement'])]
    bad = np.nonzero(~rep['converged'].all(1))[0]
    return dict(slices=int(len(rep['coverage_before'])), coverage_before=float(rep['coverage_before'].mean()),
                coverage_after=float(rep['coverage_after'].mean()), agreement=float(agree.mean()) if len(agree) else float('nan'),
                max_iterations=int(rep['iterations'].max()), worst_relres=float(rep['relres'].max()),
                unconverged=int((~rep['converged']).sum()), unconverged_slices=[int(i) for i in bad])


def summary_line(s) -> str:
    return (f'random-walker scribbles: {s["slices"]} slices, mean coverage {100 * s["coverage_before"]:.2f} % -> '
            f'{100 * s["coverage_after"]:.2f} %, agreement with lab on newly labelled pixels {100 * s["agreement"]:.2f} %; '
            f'largest iteration count {s["max_iterations"]}, worst true residual {s["worst_relres"]:.2e}, '
            f'{s["unconverged"]} unconverged systems')


# ---- the walker with priors: pseudo-labels refreshed during training (train_chaos.py --rw_refresh) ------------
# Grady 2005: with q = softmax_k(logits) as a unary prior beside the scribble seeds,
#     (L_UU + gamma I) x_k = b_k + gamma q_k|U      for EVERY class k when gamma > 0
# (a class without a seed and a slice without any seed are ordinary systems; sum_k prob[k] = 1 on h x w); gamma = 0 is the plain
# walker.  S is ALWAYS the scribble as stored on disk, never an earlier pseudo-label.  libpacingpseudo_rwp.so, include/pacingpseudo_rwp.h.
def check_rw_prior_params(gamma=0.1) -> float:
    """The accepted range of prwp_solve's gamma, checked before any launch: a finite number >= 0 (an untuned first value)."""
    if isinstance(gamma, bool):
        raise ValueError(f'random walker: gamma must be a number (got {gamma!r})')
    gamma = float(gamma)
    if not (gamma >= 0.0 and math.isfinite(gamma)):
        raise ValueError(f'random walker: gamma must be a finite number >= 0 (got {gamma!r})')
    return gamma


def add_rw_refresh_flags(parser) -> None:
    """--rw_refresh and its parameters (train_chaos.py only); beta, eps, tol, max_iters and threshold are the --rw_* flags above."""
    parser.add_argument('--rw_refresh', type=int, default=0,
                        help='every N epochs re-run the random walker on every training slice with the network\'s own soft-max as a '
                             'unary prior beside the scribble seeds and replace the pseudo-labels (0 = off); runs between epochs, '
                             'never inside a step')
    parser.add_argument('--rw_refresh_start', type=int, default=0,
                        help='first epoch at whose start the pseudo-labels are refreshed (0 = the value of --rw_refresh)')
    parser.add_argument('--rw_prior_gamma', type=float, default=0.1,
                        help='weight of the soft-max prior in the refreshed walker, >= 0 (an untuned first value; 0 = no prior)')


def check_rw_refresh_flags(every, start, gamma):
    """(every, first epoch, gamma) of the three flags; ValueError for values that are no period / epoch / weight."""
    if every < 0:
        raise ValueError(f'--rw_refresh must be >= 0 (got {every})')
    if start < 0:
        raise ValueError(f'--rw_refresh_start must be >= 0 (got {start})')
    return int(every), int(start) if start else int(every), check_rw_prior_params(gamma)


def refresh_epochs(every, start, upto):
    """The epochs t <= `upto` at whose start a refresh runs: t >= start and (t - start) % every == 0."""
    every, start, _ = check_rw_refresh_flags(every, start, 0.0)
    return list(range(start, int(upto) + 1, every)) if every else []


def _prior_inputs(image, scribble, logits, num_classes, sizes):
    """``_inputs`` plus logits (N, K, H, W) fp32, every check made before the library is touched."""
    named = ((image, 'image'), (scribble, 'scribble'), (logits, 'logits'))
    for x, what in named:
        if not torch.is_tensor(x):
            raise TypeError(f'{what} must be a torch tensor, got {type(x).__name__}')
    for x, what in named:
        if not x.is_cuda:
            raise TypeError(f'{what} must be a CUDA tensor: the random walker has no CPU path')
    if logits.dtype != torch.float32:
        raise TypeError(f'logits must be float32, got {logits.dtype}')
    img, scb, host_sizes, K = _inputs(image, scribble, num_classes, sizes)
    N, H, W = img.shape
    if tuple(logits.shape) != (N, K, H, W):
        raise ValueError(f'logits must be (N, K, H, W) = {(N, K, H, W)}, got {tuple(logits.shape)}')
    if logits.device != img.device:
        raise ValueError(f'logits are on {logits.device}, image on {img.device}')
    if not bool(torch.isfinite(logits).all()):
        raise ValueError('logits hold non-finite values: no soft-max prior can be formed from them')
    return img, scb, logits.contiguous(), host_sizes, K


def _solve_prior(img, scb, logits, host_sizes, K, prm, gamma):
    from .._rwp import rwp
    N, H, W = img.shape
    prob = torch.empty((N, K, H, W), device=img.device, dtype=torch.float32)
    stats = torch.empty((N, K, 3), device=img.device, dtype=torch.float32)
    ws = torch.empty(rwp.prwp_workspace_bytes(N, K, H, W), device=img.device, dtype=torch.uint8)
    with torch.cuda.device(img.device):
        rwp.prwp_solve(img.data_ptr(), scb.data_ptr(), logits.data_ptr(), _sizes_ptr(host_sizes), N, K, H, W, prm['beta'], prm['eps'],
                       gamma, prm['tol'], prm['max_iters'], prob.data_ptr(), stats.data_ptr(), ws.data_ptr(), stream_ptr())
    return prob, stats


def random_walker_prior(image, scribble, logits, num_classes, sizes=None, *, gamma=0.1, beta=13.0, eps=1e-4, tol=1e-6, max_iters=10000,
                        return_stats=False):
    """Random-walker probabilities with the soft-max of `logits` ((N, K, H, W) fp32 CUDA on the image's device, finite) as a unary
    prior of weight `gamma`; everything else as ``random_walker``.  Returns prob (N, K, H, W) fp32, with ``return_stats`` also stats
    (N, K, 3) = (iterations, true relative residual, converged) per system.  Runs on the current stream."""
    prm, gamma = check_rw_params(beta, eps, tol, max_iters), check_rw_prior_params(gamma)
    img, scb, z, host_sizes, K = _prior_inputs(image, scribble, logits, num_classes, sizes)
    prob, stats = _solve_prior(img, scb, z, host_sizes, K, prm, gamma)
    return (prob, stats) if return_stats else prob


def refresh_scribbles(image, scribble, logits, num_classes, sizes=None, threshold=0.9, *, gamma=0.1, beta=13.0, eps=1e-4, tol=1e-6,
                      max_iters=10000, return_stats=False, return_prob=False):
    """Refreshed pseudo-labels: ``random_walker_prior`` followed by the thresholded first-maximum arg-max of ``expand_scribbles``
    (pprep_rw_labels).  `scribble` is the scribble as stored on disk.  Returns labels (N, H, W) with the dtype of `scribble`; with
    ``return_stats`` / ``return_prob`` a tuple (labels[, stats][, prob])."""
    prm, gamma = check_rw_params(beta, eps, tol, max_iters, threshold), check_rw_prior_params(gamma)
    img, scb, z, host_sizes, K = _prior_inputs(image, scribble, logits, num_classes, sizes)
    prob, stats = _solve_prior(img, scb, z, host_sizes, K, prm, gamma)
    labels = _labels(prob, scb, host_sizes, K, prm['threshold']).to(scribble.dtype)
    out = (labels,) + ((stats,) if return_stats else ()) + ((prob,) if return_prob else ())
    return out if len(out) > 1 else labels


class SharedMaps:
    """The per-slice uint8 (h, w) label maps of a data set in ONE shared-memory buffer with per-slice offsets: what
    ``dataset.scribble_override`` takes when the maps change during a run.  The train loader's workers are persistent, so a list
    replaced in the parent never reaches them; ``update`` writes in place into memory the workers map too.  One flat buffer, not one
    tensor per slice: every shared tensor holds a file descriptor."""

    def __init__(self, maps):
        maps = [np.asarray(m) for m in maps]
        if any(m.ndim != 2 or m.dtype != np.uint8 for m in maps):
            raise TypeError('SharedMaps takes uint8 (h, w) maps')
        self.shapes = [tuple(int(s) for s in m.shape) for m in maps]
        self.offsets = np.concatenate([[0], np.cumsum([h * w for h, w in self.shapes])]).astype(np.int64)
        self.buffer = torch.zeros(max(int(self.offsets[-1]), 1), dtype=torch.uint8).share_memory_()
        for i, m in enumerate(maps):
            self.update(i, m)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self.shapes):
            raise IndexError(i)
        return self.buffer.numpy()[self.offsets[i]:self.offsets[i + 1]].reshape(self.shapes[i])

    def update(self, i, m):
        m = np.asarray(m)
        if tuple(m.shape) != self.shapes[int(i)] or m.dtype != np.uint8:
            raise ValueError(f'map {i} must be uint8 {self.shapes[int(i)]}, got {m.dtype} {tuple(m.shape)}')
        self[i][...] = m


def refresh_dataset(dataset, forward, num_classes, device, prm, stride=1):
    """Refresh the pseudo-labels of every slice of a ``data.NpzSlices`` data set with the network's prediction as prior.  Batching
    as in ``expand_dataset``.  `forward` maps an (n, 1, h, w) fp32 device batch -- the slices normalised on the host exactly as
    ``NpzSlices._sample`` does for evaluation items -- to logits (n, K, h, w); `prm` is ``check_rw_params(...)`` plus ``gamma``.  A
    slice whose h or w is no multiple of `stride` (the encoder's) cannot go through the network: it keeps the map in force
    (``dataset.scribble_override``, else its scribble).  Returns ``(maps, report)``: `maps` as ``expand_dataset``; `report` has its
    fields (coverage_before / agreement relative to the scribble on disk) plus skipped (n, bool) and changed (n) = share of the
    pixels whose label differs from the map in force before.  The data set itself is not modified.  Deterministic."""
    K, n = int(num_classes), len(dataset)
    if K > 255:
        raise NotImplementedError('the refreshed maps are kept as uint8')
    stride, gamma = int(stride), check_rw_prior_params(prm['gamma'])
    over = dataset.scribble_override
    maps = [None] * n
    rep = dict(iterations=np.zeros((n, K), np.int32), relres=np.zeros((n, K), np.float32), converged=np.ones((n, K), bool),
               coverage_before=np.zeros(n), coverage_after=np.zeros(n), agreement=np.full(n, np.nan),
               skipped=np.zeros(n, bool), changed=np.zeros(n))

    def flush(idx, items):
        raw = np.stack([np.asarray(it[0], dtype=np.float32) for it in items])
        scb_h = np.stack([np.asarray(it[2]).astype(np.uint8) for it in items])
        norm = np.stack([(x - x.mean()) / (x.std() + 1e-8) for x in raw])            # MeanStdNorm of NpzSlices._sample
        with torch.no_grad():
            logits = forward(torch.from_numpy(norm[:, None]).to(device)).float().contiguous()
        res = refresh_scribbles(torch.from_numpy(raw).to(device), torch.from_numpy(scb_h).to(device), logits, K, None, prm['threshold'],
                                gamma=gamma, beta=prm['beta'], eps=prm['eps'], tol=prm['tol'], max_iters=prm['max_iters'],
                                return_stats=True)
        lab_new, st = res[0].cpu().numpy(), res[1].cpu().numpy()
        for j, i in enumerate(idx):
            maps[i] = np.ascontiguousarray(lab_new[j])
            rep['iterations'][i], rep['relres'][i], rep['converged'][i] = st[j, :, 0], st[j, :, 1], st[j, :, 2] > 0.5
            new = (scb_h[j] == K) & (lab_new[j] != K)
            if new.any():
                rep['agreement'][i] = float((lab_new[j][new] == np.asarray(items[j][1])[new]).mean())

    idx, items, before = [], [], [None] * n
    for i in range(n):
        it = dataset.raw_arrays(i)
        h, w = it[0].shape
        before[i] = np.array(over[i] if over is not None else it[2]).astype(np.uint8)      # a copy: `over` may be updated in place
        rep['coverage_before'][i] = float((np.asarray(it[2]) != K).mean())
        if h % stride or w % stride:
            rep['skipped'][i] = True
            maps[i] = before[i]
            continue
        if items and (len(items) == RW_BATCH or it[0].shape != items[0][0].shape):
            flush(idx, items)
            idx, items = [], []
        idx.append(i)
        items.append(it)
    if items:
        flush(idx, items)
    for i in range(n):
        rep['coverage_after'][i] = float((maps[i] != K).mean())
        rep['changed'][i] = float((maps[i] != before[i]).mean())
    return maps, rep


def refresh_forward(model, num_classes):
    """The `forward` of ``refresh_dataset`` for a ``ConsistencyRegulr``: the eval-mode forward validation uses (``mode='val'``,
    ``'segmentation/logits'``) with the live weights.  Every module's train / eval flag is put back afterwards; an eval-mode forward
    updates no buffer and draws from no generator."""
    K = int(num_classes)

    def forward(image):
        B, _, H, W = image.shape
        scribble = torch.zeros((B, K + 1, H, W), device=image.device, dtype=torch.float32)
        scribble[:, K] = 1.0                                  # nothing labelled: the forward's loss_pce is not used
        flags = [(m, m.training) for m in model.modules()]
        model.eval()
        try:
            with torch.no_grad():
                return model({'image': image, 'scribble': scribble}, mode='val')['segmentation/logits']
        finally:
            for m, was in flags:
                m.training = was
    return forward


def refresh_summary_line(s, epoch, skipped, changed) -> str:
    return (f'random-walker refresh at epoch {epoch:03d}: {s["slices"]} slices ({skipped} skipped), mean coverage '
            f'{100 * s["coverage_before"]:.2f} % -> {100 * s["coverage_after"]:.2f} %, agreement with lab on newly labelled pixels '
            f'{100 * s["agreement"]:.2f} %, {100 * changed:.2f} % of the pixels changed; largest iteration count '
            f'{s["max_iterations"]}, worst true residual {s["worst_relres"]:.2e}, {s["unconverged"]} unconverged systems')
