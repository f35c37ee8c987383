"""Exact Euclidean distance transforms on the GPU and the signed level-set maps of the boundary loss (Kervadec et al., MIDL 2019,
"Boundary loss for highly unbalanced segmentation").  The published code precomputes its maps on the host, once per slice; the
fully supervised trainer's labels exist only on the device, after the weak augmentation, so the maps are recomputed per step from
the augmented label (pdist_edt / pdist_signed_maps, include/pacingpseudo_dist.h: a column pass and a row pass, exact, no
host synchronisation, no floating-point atomics -- the same bits in every run).

    distance_transform_edt(mask, spacing)        scipy.ndimage.distance_transform_edt(mask, sampling=spacing); a plane without a
                                                 zero pixel gives +inf everywhere (scipy's values there mean nothing)
    signed_distance_maps(class_map, K, spacing)  phi_k = +d(x, S_k) outside S_k, -(d(x, S_k^c) - min(spacing)) inside: with unit
                                                 spacing Kervadec's one_hot2dist; phi_k = 0 where S_k is empty (as there) and also
                                                 where S_k is the whole image (no boundary, no force)

Both take CUDA tensors, (H, W) as well as batched input, and raise ValueError before the library is touched."""
import math

import torch

from .._lib import stream_ptr

_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
MAX_CLASSES = 32
MAX_SIDE = 2048


def check_spacing(spacing):
    """-> (sy, sx) as floats; ValueError unless two finite numbers > 0."""
    try:
        sy, sx = (float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f'spacing must be two numbers (sy, sx), got {spacing!r}') from None
    if not (math.isfinite(sy) and math.isfinite(sx) and sy > 0.0 and sx > 0.0):
        raise ValueError(f'spacing must be finite and > 0, got {(sy, sx)!r}')
    return sy, sx


def check_num_classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f'num_classes must be an integer in 1 .. {MAX_CLASSES}, got {num_classes!r}')
    return int(num_classes)


def _check(x, what, dtypes, planes=1):
    """-> (contiguous (N, H, W) view, whether the input was (H, W)); ValueError before the library is touched."""
    if not torch.is_tensor(x):
        raise ValueError(f'{what} must be a torch tensor, got {type(x).__name__}')
    if x.dtype not in dtypes:
        raise ValueError(f'{what} must be one of {", ".join(str(d) for d in dtypes)}, got {x.dtype}')
    if x.dim() not in (2, 3):
        raise ValueError(f'{what} must be (N, H, W) or (H, W), got {tuple(x.shape)}')
    if min(x.shape) < 1:
        raise ValueError(f'{what} has an empty axis: {tuple(x.shape)}')
    if max(x.shape[-2:]) > MAX_SIDE:
        raise ValueError(f'{what} is {tuple(x.shape)}; the kernels take H, W <= {MAX_SIDE} (squared pixel distances stay below 2^24)')
    if x.numel() * planes >= 2 ** 31:
        raise ValueError(f'{what} asks for {x.numel() * planes} output elements; the kernels index with 32 bits (< 2^31)')
    if not x.is_cuda:
        raise ValueError(f'{what} must be a CUDA tensor: there is no CPU path')
    single = x.dim() == 2
    return (x[None] if single else x), single


def distance_transform_edt(mask, spacing=(1., 1.), squared=False):
    """fp32 tensor of mask's shape: at a non-zero pixel the Euclidean distance (pixel pitch `spacing` = (sy, sx)) to the nearest
    zero pixel of the same plane, 0 at a zero pixel, +inf in a plane without a zero pixel.  `mask`: bool or integer CUDA tensor
    (P, H, W) or (H, W).  ``squared`` returns the squared distances; with unit spacing they are exact integers."""
    sy, sx = check_spacing(spacing)
    if not isinstance(squared, (bool, int)) or squared not in (0, 1):
        raise ValueError(f'squared must be a bool, got {squared!r}')
    x, single = _check(mask, 'mask', (torch.bool,) + _INT_DTYPES)
    from .._dist import dist
    m = (x != 0).to(torch.uint8).contiguous()
    P, H, W = m.shape
    out = torch.empty((P, H, W), device=m.device, dtype=torch.float32)
    with torch.cuda.device(m.device):
        nws = dist.pdist_edt_workspace(P, H, W)
        ws = torch.empty(max(nws // 8, 1), device=m.device, dtype=torch.float64)
        dist.pdist_edt(m.data_ptr(), P, H, W, sy, sx, int(bool(squared)), out.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return out[0] if single else out


def signed_distance_maps(class_map, num_classes, spacing=(1., 1.)):
    """phi fp32 (N, K, H, W) -- (K, H, W) for an (H, W) map -- from the integer class map: for class k with S the pixels of value k,
    +d(x, S) outside S and -(d(x, complement of S) - min(spacing)) inside; 0 everywhere where S is empty or the whole image.  A
    value outside [0, K) belongs to no class."""
    K = check_num_classes(num_classes)
    sy, sx = check_spacing(spacing)
    x, single = _check(class_map, 'class_map', _INT_DTYPES, planes=K)
    from .._dist import dist
    c = x.to(torch.int64).contiguous()
    N, H, W = c.shape
    phi = torch.empty((N, K, H, W), device=c.device, dtype=torch.float32)
    with torch.cuda.device(c.device):
        nws = dist.pdist_signed_maps_workspace(N, K, H, W)
        ws = torch.empty(max(nws // 8, 1), device=c.device, dtype=torch.float64)
        dist.pdist_signed_maps(c.data_ptr(), N, K, H, W, sy, sx, phi.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return phi[0] if single else phi
