"""A size threshold per class and hole filling on hard class maps, on the GPU (libpacingpseudo_morph.so,
include/pacingpseudo_morph.h): the two clean-up steps evaluation pipelines pair with keep-largest (``utils.postprocess``,
``utils.volume``).  The reference scores its raw arg-max; both are additions, off by default in ``inference.py``
(``--min_component_size``, ``--fill_holes``).

    remove_small_components(class_map, K, min_size, connectivity)      per slice: components of a class k in 1 .. K - 1 with fewer than
    remove_small_components_3d(class_map, K, min_size, connectivity)   min_size[k] pixels / voxels become 0 (exactly min_size[k] stay:
                                                                       skimage.morphology.remove_small_objects)
    fill_holes(class_map, K, connectivity)                             a component of value-0 pixels that does not reach the border
    fill_holes_3d(class_map, K, connectivity)                          and touches ONE class k in 1 .. K - 1 becomes k; one that touches
                                                                       several classes, or a value outside [0, K), is left alone
    binary_fill_holes(mask, connectivity)                              scipy.ndimage.binary_fill_holes(mask,
                                                                       generate_binary_structure(mask.ndim, connectivity))
    check_morph_params(...)                                            the driver's flags, checked

``connectivity`` follows scipy's naming: 1, 2 in 2-D (4 / 8 neighbours), 1, 2, 3 in 3-D (6 / 18 / 26).  For the threshold it says
which pixels of a class form one component; for hole filling it says which value-0 pixels form one cavity and which pixels a cavity
touches (scipy's ``structure``; 1 is scipy's default).  The 2-D functions take ``(N, H, W)`` or ``(H, W)``, the 3-D ones one
``(D, H, W)`` volume; all take integer CUDA tensors, label with the existing labellers (pp_label_components,
pvol_label_components), allocate their workspace, enqueue on the current stream and raise ValueError before a library is touched.
Integer atomics only, a launch sequence fixed by the shape, no host synchronisation: the same bits in every run."""
import torch

from .._lib import lib, stream_ptr
from .postprocess import _check as _check_slices
from .volume import _check_connectivity as _check_connectivity_3d
from .volume import _check_volume, _workspace

_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
MAX_CLASSES = 32
MAX_SIDE = 2048


def _check_classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f'num_classes must be an integer in 1 .. {MAX_CLASSES}, got {num_classes!r}')
    return int(num_classes)


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _check_min_size(min_size, K):
    """-> K thresholds as a list of ints (entry 0 is never read); ValueError unless an int >= 0 or K of them."""
    if _is_int(min_size):
        sizes = [min_size] * K
    else:
        try:
            sizes = list(min_size)
        except TypeError:
            raise ValueError(f'min_size must be an integer or a sequence of num_classes = {K} integers, got {min_size!r}') from None
        if len(sizes) != K:
            raise ValueError(f'min_size has {len(sizes)} entries, need one per class: num_classes = {K}')
    for s in sizes:
        if not _is_int(s) or not 0 <= s < 2 ** 31:
            raise ValueError(f'min_size must hold integers in 0 .. 2^31 - 1, got {s!r}')
    return [int(s) for s in sizes]


def _check_slice_sides(x):
    if max(x.shape[1:]) > MAX_SIDE:
        raise ValueError(f'class_map is {tuple(x.shape)}; the kernels take H, W <= {MAX_SIDE}')


def _label_slices(x, connectivity):
    N, H, W = x.shape
    labels = torch.empty((N, H, W), device=x.device, dtype=torch.int32)
    nws = lib.pp_components_workspace(N, 1, H, W)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    lib.pp_label_components(x.data_ptr(), N, H, W, int(connectivity), labels.data_ptr(), ws.data_ptr(), nws, stream_ptr())
    return labels


def _label_volume(x, connectivity):
    from .._vol import vol
    D, H, W = x.shape
    labels = torch.empty((D, H, W), device=x.device, dtype=torch.int32)
    ws = _workspace(vol.pvol_label_workspace(D, H, W), x.device)
    vol.pvol_label_components(x.data_ptr(), D, H, W, int(connectivity), labels.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return labels


def _remove_small(x, K, sizes, connectivity, dims):
    """x int64 contiguous (N, H, W) [dims 2] or (D, H, W) [dims 3] -> (out int64, stats int32 (N, K, 2))."""
    import ctypes
    from .._morph import morph
    N, D, H, W = (x.shape[0], 1) + tuple(x.shape[1:]) if dims == 2 else (1,) + tuple(x.shape)
    out = torch.empty_like(x)
    stats = torch.empty((N, K, 2), device=x.device, dtype=torch.int32)
    thresholds = (ctypes.c_int32 * K)(*sizes)
    with torch.cuda.device(x.device):
        labels = _label_slices(x, connectivity) if dims == 2 else _label_volume(x, connectivity)
        ws = _workspace(morph.pmor_workspace(N, K, D, H, W, dims), x.device)
        morph.pmor_remove_small(x.data_ptr(), labels.data_ptr(), N, K, D, H, W, dims, thresholds, out.data_ptr(), stats.data_ptr(),
                                ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return out, stats


def _fill(x, K, connectivity, dims):
    from .._morph import morph
    N, D, H, W = (x.shape[0], 1) + tuple(x.shape[1:]) if dims == 2 else (1,) + tuple(x.shape)
    out = torch.empty_like(x)
    stats = torch.empty((N, K, 2), device=x.device, dtype=torch.int32)
    with torch.cuda.device(x.device):
        labels = _label_slices(x, connectivity) if dims == 2 else _label_volume(x, connectivity)
        ws = _workspace(morph.pmor_workspace(N, K, D, H, W, dims), x.device)
        morph.pmor_fill_holes(x.data_ptr(), labels.data_ptr(), N, K, D, H, W, dims, int(connectivity), out.data_ptr(), stats.data_ptr(),
                              ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return out, stats


def remove_small_components(class_map, num_classes, min_size, connectivity=1, return_stats=False):
    """For every slice and every foreground class ``k`` in ``1 .. num_classes - 1`` the components of class ``k`` with fewer than
    ``min_size[k]`` pixels become 0 (``min_size``: one integer for all classes or ``num_classes`` of them; <= 1 leaves the class
    alone); everything else -- class 0, values outside ``[0, num_classes)`` -- is copied.  Returns a new tensor of class_map's shape
    and dtype; with ``return_stats`` also an int32 tensor ``(N, num_classes, 2)`` (``(num_classes, 2)`` for an ``(H, W)`` map):
    components removed, pixels removed."""
    K = _check_classes(num_classes)
    sizes = _check_min_size(min_size, K)
    x, single = _check_slices(class_map, connectivity)
    _check_slice_sides(x)
    out, stats = _remove_small(x, K, sizes, connectivity, 2)
    out = out.to(class_map.dtype)
    if single:
        out, stats = out[0], stats[0]
    return (out, stats) if return_stats else out


def remove_small_components_3d(class_map, num_classes, min_size, connectivity=1, return_stats=False):
    """The same on one ``(D, H, W)`` volume with 3-D components (``connectivity`` 1, 2, 3 = 6, 18, 26 neighbours); stats
    ``(num_classes, 2)``: components removed, voxels removed."""
    K = _check_classes(num_classes)
    sizes = _check_min_size(min_size, K)
    c = _check_connectivity_3d(connectivity)
    x = _check_volume(class_map, 'class_map', _INT_DTYPES).to(torch.int64).contiguous()
    out, stats = _remove_small(x, K, sizes, c, 3)
    out = out.to(class_map.dtype)
    return (out, stats[0]) if return_stats else out


def fill_holes(class_map, num_classes, connectivity=1, return_stats=False):
    """For every slice: a component of value-0 pixels (under ``connectivity``) without a pixel in the first or last row or column
    is a cavity; if all the non-zero pixels its pixels touch (under the same connectivity) hold one class ``k`` in
    ``1 .. num_classes - 1`` it becomes ``k``.  A cavity that touches two or more classes is left and counted; one that touches a
    value outside ``[0, num_classes)`` is left.  Nothing non-zero changes.  Returns a new tensor of class_map's shape and dtype;
    with ``return_stats`` also an int32 tensor ``(N, num_classes, 2)`` (``(num_classes, 2)`` for an ``(H, W)`` map): row ``k >= 1``
    = cavities filled with k, pixels filled; row 0 = cavities left for their mixed contacts, their pixels."""
    K = _check_classes(num_classes)
    x, single = _check_slices(class_map, connectivity)
    _check_slice_sides(x)
    out, stats = _fill(x, K, connectivity, 2)
    out = out.to(class_map.dtype)
    if single:
        out, stats = out[0], stats[0]
    return (out, stats) if return_stats else out


def fill_holes_3d(class_map, num_classes, connectivity=1, return_stats=False):
    """The same on one ``(D, H, W)`` volume: cavities are 3-D components of value-0 voxels that reach none of the six faces (a
    volume of one slice has none); stats ``(num_classes, 2)``."""
    K = _check_classes(num_classes)
    c = _check_connectivity_3d(connectivity)
    x = _check_volume(class_map, 'class_map', _INT_DTYPES).to(torch.int64).contiguous()
    out, stats = _fill(x, K, c, 3)
    out = out.to(class_map.dtype)
    return (out, stats[0]) if return_stats else out


def binary_fill_holes(mask, connectivity=1):
    """``scipy.ndimage.binary_fill_holes(mask, generate_binary_structure(mask.ndim, connectivity))`` for one bool CUDA tensor of 2
    or 3 dimensions -- ``(H, W)`` or ``(D, H, W)``; a stack of slices goes through ``fill_holes(mask.long(), 2)`` -- as a bool tensor."""
    if not torch.is_tensor(mask):
        raise ValueError(f'mask must be a torch tensor, got {type(mask).__name__}')
    if mask.dtype != torch.bool:
        raise ValueError(f'mask must be a bool tensor, got {mask.dtype}')
    if mask.dim() not in (2, 3):
        raise ValueError(f'mask must be (H, W) or (D, H, W), got {tuple(mask.shape)}')
    x = mask.to(torch.uint8)
    out = fill_holes(x, 2, connectivity) if mask.dim() == 2 else fill_holes_3d(x, 2, connectivity)
    return out != 0


def check_morph_params(min_component_size=0, fill_holes=False, fill_holes_connectivity=1, min_component_size_3d=0,
                       fill_holes_connectivity_3d=1, volumes=False):
    """The driver's flags -> dict(min_component_size, fill_holes, fill_holes_connectivity, min_component_size_3d,
    fill_holes_connectivity_3d); ValueError naming the flag otherwise.  The two ``*_3d`` values belong to ``volumes``."""
    for name, v in (('min_component_size', min_component_size), ('min_component_size_3d', min_component_size_3d)):
        if not _is_int(v) or not 0 <= v < 2 ** 31:
            raise ValueError(f'--{name} {v!r}: a number of pixels, an integer >= 0 (0 = off)')
    if not isinstance(fill_holes, (bool, int)) or fill_holes not in (0, 1):
        raise ValueError(f'--fill_holes is on or off, got {fill_holes!r}')
    if not _is_int(fill_holes_connectivity) or fill_holes_connectivity not in (1, 2):
        raise ValueError(f'--fill_holes_connectivity {fill_holes_connectivity!r}: 1 (4 neighbours, scipy\'s default) or 2 (8)')
    if not _is_int(fill_holes_connectivity_3d) or fill_holes_connectivity_3d not in (1, 2, 3):
        raise ValueError(f'--fill_holes_connectivity_3d {fill_holes_connectivity_3d!r}: 1 (6 neighbours), 2 (18) or 3 (26)')
    if not volumes:
        if min_component_size_3d:
            raise ValueError('--min_component_size_3d belongs to --volumes: pass --volumes as well')
        if fill_holes_connectivity_3d != 1:
            raise ValueError('--fill_holes_connectivity_3d belongs to --volumes: pass --volumes as well')
    return dict(min_component_size=int(min_component_size), fill_holes=bool(fill_holes),
                fill_holes_connectivity=int(fill_holes_connectivity), min_component_size_3d=int(min_component_size_3d),
                fill_holes_connectivity_3d=int(fill_holes_connectivity_3d))
