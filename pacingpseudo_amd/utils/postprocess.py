"""Post-processing of hard class maps on the GPU: connected-component labelling and the keep-largest-component filter that
usually follows the arg-max of a scribble-supervised network (its typical error is a few small false-positive islands far from
the organ: Dice hardly sees them, HD95 is dominated by them).  The reference scores its raw arg-max (inference.py:159-190); this
is an addition, off by default in ``inference.py`` (``--keep_largest_cc``).

Two pixels of one slice are connected when they are neighbours -- ``connectivity`` 1: the 4-neighbourhood, 2: the
8-neighbourhood, scipy.ndimage's naming -- and hold the same value.  Both functions take ``(N, H, W)`` or ``(H, W)`` integer
CUDA tensors, allocate their workspace and enqueue on the current stream (pp_label_components / pp_keep_largest_components:
a launch sequence fixed by the shape, no host synchronisation, integer atomics only -- the same bits in every run)."""
import torch

from .._lib import lib, stream_ptr

_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
MAX_CLASSES = 32


def _check(class_map, connectivity):
    """-> (int64 contiguous (N, H, W) view or copy, whether the input was (H, W)); ValueError before the library is touched."""
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (1, 2):
        raise ValueError(f'connectivity must be 1 (4-neighbourhood) or 2 (8-neighbourhood), got {connectivity!r}')
    if not torch.is_tensor(class_map):
        raise ValueError(f'class_map must be a torch tensor, got {type(class_map).__name__}')
    if class_map.dtype not in _INT_DTYPES:
        raise ValueError(f'class_map must hold integers, got {class_map.dtype}')
    if class_map.dim() not in (2, 3):
        raise ValueError(f'class_map must be (N, H, W) or (H, W), got {tuple(class_map.shape)}')
    if min(class_map.shape) < 1:
        raise ValueError(f'class_map has an empty axis: {tuple(class_map.shape)}')
    if class_map.numel() >= 2 ** 31:
        raise ValueError(f'class_map has {class_map.numel()} pixels; the kernels index with 32 bits (N*H*W < 2^31)')
    if not class_map.is_cuda:
        raise ValueError('class_map must be a CUDA tensor: there is no CPU path')
    single = class_map.dim() == 2
    x = class_map[None] if single else class_map
    return x.to(torch.int64).contiguous(), single


def label_components(class_map, connectivity=1):
    """int32 tensor of class_map's shape: for every pixel the smallest row-major index ``y * W + x`` among the pixels of its
    component within its slice.  Every value is labelled, background included, in one pass."""
    x, single = _check(class_map, connectivity)
    N, H, W = x.shape
    labels = torch.empty((N, H, W), device=x.device, dtype=torch.int32)
    nws = lib.pp_components_workspace(N, 1, H, W)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    with torch.cuda.device(x.device):
        lib.pp_label_components(x.data_ptr(), N, H, W, int(connectivity), labels.data_ptr(), ws.data_ptr(), nws, stream_ptr())
    return labels[0] if single else labels


def keep_largest_components(class_map, num_classes, connectivity=1, return_stats=False):
    """For every slice and every foreground class ``k`` in ``1 .. num_classes - 1`` the pixels of class ``k`` outside that class's
    largest component become 0; everything else -- class 0, and any value outside ``[0, num_classes)`` -- is copied.  Of
    components of equal size the one that holds the lowest row-major pixel stays (``numpy.argmax(numpy.bincount(labels)[1:])``
    on scipy's labels).  Returns a new tensor of class_map's shape and dtype; with ``return_stats`` also an int32 tensor
    ``(N, num_classes, 2)`` (``(num_classes, 2)`` for an ``(H, W)`` map): components of the class before filtering, pixels kept."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f'num_classes must be an integer in 1 .. {MAX_CLASSES}, got {num_classes!r}')
    x, single = _check(class_map, connectivity)
    N, H, W = x.shape
    K = int(num_classes)
    out = torch.empty_like(x)
    stats = torch.empty((N, K, 2), device=x.device, dtype=torch.int32)
    nws = lib.pp_components_workspace(N, K, H, W)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    with torch.cuda.device(x.device):
        lib.pp_keep_largest_components(x.data_ptr(), N, K, H, W, int(connectivity), out.data_ptr(), stats.data_ptr(), ws.data_ptr(), nws,
                                       stream_ptr())
    out = out.to(class_map.dtype)
    if single:
        out, stats = out[0], stats[0]
    return (out, stats) if return_stats else out
