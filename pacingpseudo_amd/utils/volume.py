"""Volume-wise evaluation of hard class maps on the GPU (libpacingpseudo_vol.so, include/pacingpseudo_vol.h): what the field
reports for CHAOS, ACDC and LVSC is Dice, HD95 and ASSD per PATIENT VOLUME, after keeping the largest 3-D component of every organ.
The reference -- and ``inference.py`` without ``--volumes`` -- scores every slice on its own.

    label_components_3d(class_map, connectivity)             int32 labels: the smallest linear index z*H*W + y*W + x of the component
    keep_largest_components_3d(class_map, K, connectivity)   per foreground class the largest 3-D component stays, the rest becomes 0
    distance_transform_edt_3d(mask, spacing, squared)        scipy.ndimage.distance_transform_edt(mask, sampling=spacing), +inf
                                                             in a volume without a zero voxel
    volume_surface_metrics(pred, label, K, spacing, ...)     hd, hdp (HD95), assd, nsd per class, medpy's surfaces in 3-D
    volume_dice(pred, label, K)                              Dice per class on voxel counts
    group_volumes(names, pattern)                            slice names -> {volume id: slice indices in slice order} (host only)

``connectivity`` 1, 2, 3 = 6, 18, 26 neighbours (``scipy.ndimage.generate_binary_structure(3, c)``); ``spacing`` = (sz, sy, sx).
The device functions take ONE (D, H, W) CUDA tensor per call -- volumes differ in depth --, allocate their workspace, enqueue on
the current stream and raise ValueError before the library is touched."""
import math
import re
from collections import OrderedDict

import numpy as np
import torch

from .._lib import lib, stream_ptr
from .metrics import surface_metrics_from_reduction

_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
MAX_CLASSES = 32
MAX_DEPTH = 4096
MAX_SIDE = 2048
# everything before a trailing run of digits -- optionally preceded by `_`, `-` or `slice` -- is the volume id, the digits the slice number
DEFAULT_VOLUME_PATTERN = r'^(?P<volume>.+?)(?:[_-]?slice)?[_-]?(?P<slice>[0-9]+)$'


def _check_volume(x, what, dtypes):
    if not torch.is_tensor(x):
        raise ValueError(f'{what} must be a torch tensor, got {type(x).__name__}')
    if x.dtype not in dtypes:
        raise ValueError(f'{what} must be one of {", ".join(str(d) for d in dtypes)}, got {x.dtype}')
    if x.dim() != 3:
        raise ValueError(f'{what} must be one (D, H, W) volume, got {tuple(x.shape)}')
    if min(x.shape) < 1:
        raise ValueError(f'{what} has an empty axis: {tuple(x.shape)}')
    if x.shape[0] > MAX_DEPTH or max(x.shape[1:]) > MAX_SIDE:
        raise ValueError(f'{what} is {tuple(x.shape)}; the kernels take D <= {MAX_DEPTH} and H, W <= {MAX_SIDE}')
    if x.numel() >= 2 ** 31:
        raise ValueError(f'{what} has {x.numel()} voxels; the kernels index with 32 bits (D*H*W < 2^31)')
    if not x.is_cuda:
        raise ValueError(f'{what} must be a CUDA tensor: there is no CPU path')
    return x


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (1, 2, 3):
        raise ValueError(f'connectivity must be 1 (6 neighbours), 2 (18) or 3 (26), got {connectivity!r}')
    return int(connectivity)


def _check_classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f'num_classes must be an integer in 1 .. {MAX_CLASSES}, got {num_classes!r}')
    return int(num_classes)


def check_spacing_3d(spacing):
    """-> (sz, sy, sx) as floats; ValueError unless three finite numbers > 0."""
    try:
        sz, sy, sx = (float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f'spacing must be three numbers (sz, sy, sx), got {spacing!r}') from None
    if not all(math.isfinite(v) and v > 0.0 for v in (sz, sy, sx)):
        raise ValueError(f'spacing must be finite and > 0, got {(sz, sy, sx)!r}')
    return sz, sy, sx


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes) // 8, 1), device=device, dtype=torch.float64)      # 8-byte aligned, a multiple of 8 bytes


def label_components_3d(class_map, connectivity=1):
    """int32 tensor (D, H, W): for every voxel the smallest linear index ``z * H * W + y * W + x`` among the voxels of its component.
    Two voxels are connected when they are neighbours and hold the same value; every value is labelled, 0 included."""
    c = _check_connectivity(connectivity)
    x = _check_volume(class_map, 'class_map', _INT_DTYPES).to(torch.int64).contiguous()
    from .._vol import vol
    D, H, W = x.shape
    labels = torch.empty((D, H, W), device=x.device, dtype=torch.int32)
    with torch.cuda.device(x.device):
        nws = vol.pvol_label_workspace(D, H, W)
        ws = _workspace(nws, x.device)
        vol.pvol_label_components(x.data_ptr(), D, H, W, c, labels.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return labels


def keep_largest_components_3d(class_map, num_classes, connectivity=1, return_stats=False):
    """For every foreground class ``k`` in ``1 .. num_classes - 1`` the voxels of class ``k`` outside that class's largest 3-D
    component become 0 (of components of equal size the one with the smallest label stays); class 0 and any value outside
    ``[0, num_classes)`` are copied.  Returns a new tensor of class_map's shape and dtype; with ``return_stats`` also an int32
    tensor ``(num_classes, 2)``: components of the class before filtering, voxels removed."""
    K = _check_classes(num_classes)
    c = _check_connectivity(connectivity)
    x = _check_volume(class_map, 'class_map', _INT_DTYPES).to(torch.int64).contiguous()
    from .._vol import vol
    D, H, W = x.shape
    out = torch.empty_like(x)
    stats = torch.empty((K, 2), device=x.device, dtype=torch.int32)
    with torch.cuda.device(x.device):
        nws = vol.pvol_keep_largest_workspace(K, D, H, W)
        ws = _workspace(nws, x.device)
        vol.pvol_keep_largest_components(x.data_ptr(), K, D, H, W, c, out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                         stream_ptr())
    out = out.to(class_map.dtype)
    return (out, stats) if return_stats else out


def distance_transform_edt_3d(mask, spacing=(1., 1., 1.), squared=False):
    """fp32 tensor (D, H, W): at a non-zero voxel the Euclidean distance (voxel pitch ``spacing`` = (sz, sy, sx)) to the nearest zero
    voxel, 0 at a zero voxel, +inf in a volume without a zero voxel.  ``squared`` returns the squared distances; with unit spacing
    they are exact integers."""
    sz, sy, sx = check_spacing_3d(spacing)
    if not isinstance(squared, (bool, int)) or squared not in (0, 1):
        raise ValueError(f'squared must be a bool, got {squared!r}')
    x = _check_volume(mask, 'mask', (torch.bool,) + _INT_DTYPES)
    from .._vol import vol
    m = (x != 0).to(torch.uint8).contiguous()
    D, H, W = m.shape
    out = torch.empty((D, H, W), device=m.device, dtype=torch.float32)
    with torch.cuda.device(m.device):
        nws = vol.pvol_edt_workspace(D, H, W)
        ws = _workspace(nws, m.device)
        vol.pvol_edt(m.data_ptr(), D, H, W, sz, sy, sx, int(bool(squared)), out.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return out


def _pair(pred, label):
    p = _check_volume(pred, 'pred', _INT_DTYPES)
    t = _check_volume(label, 'label', _INT_DTYPES)
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f'pred {tuple(p.shape)} on {p.device} and label {tuple(t.shape)} on {t.device} must agree')
    return p.to(torch.int64).contiguous(), t.to(torch.int64).contiguous()


def volume_surface_metrics(pred, label, num_classes, spacing, tolerance=2.0, percentile=95.0):
    """Hausdorff distance, percentile Hausdorff distance (HD95 by default), average symmetric surface distance and surface Dice at
    ``tolerance`` (in the unit of ``spacing`` = (sz, sy, sx)) per class of one pair of (D, H, W) class maps: dict of (K,) float64
    arrays ``hd``, ``hdp``, ``assd``, ``nsd``.  Surfaces as medpy takes them in 3-D (mask XOR erosion by the 6-neighbour cross);
    the two directed distance sets (pvol_surface_distances) stay on the device, pp_surface_reduce turns them into eight numbers per
    class.  NaN where the prediction or the label is empty or fills the volume."""
    K = _check_classes(num_classes)
    sz, sy, sx = check_spacing_3d(spacing)
    tolerance, percentile = float(tolerance), float(percentile)
    if not (np.isfinite(tolerance) and tolerance >= 0.0):
        raise ValueError(f'tolerance = {tolerance!r}: a finite distance >= 0')
    if not 0.0 < percentile <= 100.0:
        raise ValueError(f'percentile = {percentile!r}: 0 < percentile <= 100')
    p, t = _pair(pred, label)
    D, H, W = p.shape
    n = D * H * W
    if K * 2 * n >= 2 ** 31:
        raise ValueError(f'{K} classes x 2 x {n} voxels: the distance sets are indexed with 32 bits (K*2*D*H*W < 2^31)')
    from .._vol import vol
    dist = torch.empty((K, 2, n), device=p.device, dtype=torch.float32)
    counts = torch.empty((K, 4), device=p.device, dtype=torch.int32)
    out = torch.empty((K, 8), device=p.device, dtype=torch.float64)
    with torch.cuda.device(p.device):
        nws = vol.pvol_surface_workspace(K, D, H, W)
        ws = _workspace(nws, p.device)
        vol.pvol_surface_distances(p.data_ptr(), t.data_ptr(), K, D, H, W, sz, sy, sx, dist.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                   ws.numel() * 8, stream_ptr())
        lib.pp_surface_reduce(dist.data_ptr(), counts.data_ptr(), K, n, percentile, tolerance, out.data_ptr(), stream_ptr())
    return surface_metrics_from_reduction(counts.cpu().numpy(), out.cpu().numpy(), n, percentile)


def volume_dice(pred, label, num_classes):
    """(K,) float64 Dice per class of one pair of (D, H, W) class maps on voxel counts, by the rules the slice driver applies to
    pixel counts: 2 |P & T| / max(|P| + |T|, 1e-8), NaN where both are empty."""
    K = _check_classes(num_classes)
    p, t = _pair(pred, label)
    D, H, W = p.shape
    from .._vol import vol
    counts = torch.empty((K, 3), device=p.device, dtype=torch.int32)
    with torch.cuda.device(p.device):
        vol.pvol_dice_counts(p.data_ptr(), t.data_ptr(), K, D, H, W, counts.data_ptr(), stream_ptr())
    c = counts.cpu().numpy().astype(np.float64)
    inter, ps, ts = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        dice = 2.0 * inter / np.maximum(ps + ts, 1e-8)
    dice[(ps == 0) & (ts == 0)] = np.nan
    return dice


def group_volumes(names, pattern=None):
    """Slice names (file stems, in data-set order) -> OrderedDict {volume id: [indices into names, sorted by slice number]}, volumes
    in the order of their first slice.  ``pattern``: a regular expression with the named groups ``volume`` and ``slice`` (digits),
    matched against the whole name; default DEFAULT_VOLUME_PATTERN.  A name that does not match, a (volume, slice) pair that occurs
    twice or a gap in a volume's slice numbers raises ValueError naming the file."""
    try:
        rx = re.compile(DEFAULT_VOLUME_PATTERN if pattern is None else pattern)
    except re.error as e:
        raise ValueError(f'volume pattern {pattern!r} is not a regular expression: {e}') from None
    if not {'volume', 'slice'} <= set(rx.groupindex):
        raise ValueError(f'volume pattern {rx.pattern!r} needs the named groups (?P<volume>...) and (?P<slice>...)')
    seen = OrderedDict()
    for i, name in enumerate(names):
        m = rx.match(str(name))
        if m is None or m.group('volume') is None or m.group('slice') is None:
            raise ValueError(f'{name!r} does not match the volume pattern {rx.pattern!r}')
        try:
            number = int(m.group('slice'))
        except ValueError:
            raise ValueError(f'{name!r}: the slice group {m.group("slice")!r} is not a number') from None
        slices = seen.setdefault(m.group('volume'), {})
        if number in slices:
            raise ValueError(f'{name!r} repeats slice {number} of volume {m.group("volume")!r} ({names[slices[number]]!r})')
        slices[number] = i
    out = OrderedDict()
    for vid, slices in seen.items():
        order = sorted(slices)
        for a, b in zip(order, order[1:]):
            if b != a + 1:
                raise ValueError(f'{names[slices[b]]!r}: volume {vid!r} has no slice {a + 1} (slice numbers must be consecutive)')
        out[vid] = [slices[s] for s in order]
    return out
