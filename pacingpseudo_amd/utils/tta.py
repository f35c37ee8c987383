"""Test-time augmentation over flips and quarter turns on the GPU: the mean soft-max over the mirrored and rotated views of a
slice, the step that usually accompanies the largest-component filter in the evaluation of a scribble-supervised network.  The
reference scores one forward pass per slice (inference.py:159-190); this is an addition, off by default in ``inference.py``
(``--tta``).

A view is an ``op`` in ``0 .. 7``: bit 0 flips the last axis (W), bit 1 flips the second-to-last axis (H), bit 2 transposes
them.  The forward view of ``a[..., H, W]`` is built as transpose, flip H, flip W -- in that order -- and the inverse undoes
the steps in reverse order; a transposing view of an ``(H, W)`` plane has shape ``(W, H)``.  ``TTA_MODES``: ``none`` is the view
set ``{0}``, ``flips`` is ops ``0 .. 3`` (no shape change), ``d4`` is ops ``0 .. 7``, the whole dihedral group.

``tta_predict`` runs the views in ascending op order: one forward call and one pp_tta_accumulate launch per view (the soft-max
of the view's logits, fp32 with the maximum subtracted, stored -- first view -- or added at the inverse-mapped position of one
accumulator), then one pp_tta_finalize launch (scale by the exact 1 / V, first-maximum arg-max).  No atomics, no host
synchronisation, a fixed order of additions: the same bits in every run."""
import torch

from .._lib import lib, stream_ptr

TTA_MODES = ('none', 'flips', 'd4')
MAX_CLASSES = 32
_OPS = {'none': (0,), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def tta_ops(mode):
    """The ops of a mode in the order they are accumulated."""
    if not isinstance(mode, str) or mode not in _OPS:
        raise ValueError(f'tta mode must be one of {TTA_MODES}, got {mode!r}')
    return _OPS[mode]


def view_shape(H, W, op):
    """Shape of the forward view of an (H, W) plane."""
    return (W, H) if op & 4 else (H, W)


def _check_op(op):
    if isinstance(op, bool) or not isinstance(op, int) or not 0 <= op <= 7:
        raise ValueError(f'op must be an integer in 0 .. 7 (bit 0 flips W, bit 1 flips H, bit 2 transposes), got {op!r}')


def _check_cuda(x, what):
    if not x.is_cuda:
        raise ValueError(f'{what} must be a CUDA tensor: there is no CPU path')


def _check(x, what, cuda=True):
    """ValueError before the library is touched, unless x is an fp32 CUDA (N, C, H, W) tensor the kernels can index."""
    if not torch.is_tensor(x):
        raise ValueError(f'{what} must be a torch tensor, got {type(x).__name__}')
    if x.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {x.dtype}')
    if x.dim() != 4:
        raise ValueError(f'{what} must be (N, C, H, W), got {tuple(x.shape)}')
    if min(x.shape) < 1:
        raise ValueError(f'{what} has an empty axis: {tuple(x.shape)}')
    if x.numel() >= 2 ** 31:
        raise ValueError(f'{what} has {x.numel()} elements; the kernels index with 32 bits (N*C*H*W < 2^31)')
    if cuda:
        _check_cuda(x, what)


def _check_logits(z, N, H, W, op, K):
    """The checks of one view's network output: (N, K, H', W') of the view `op` of an (H, W) slice, K as in the views before it
    (None for the first)."""
    _check(z, f'the logits of view {op}', cuda=False)
    want = (N,) + view_shape(H, W, op)
    if (z.shape[0],) + tuple(z.shape[2:]) != want:
        raise ValueError(f'forward returned {tuple(z.shape)} for view {op}; expected ({N}, K, {want[1]}, {want[2]})')
    if z.shape[1] > MAX_CLASSES:
        raise ValueError(f'forward returned K = {z.shape[1]} classes; the kernels hold at most {MAX_CLASSES}')
    if K is not None and z.shape[1] != K:
        raise ValueError(f'forward returned K = {z.shape[1]} classes for view {op} and {K} for the views before it')
    _check_cuda(z, f'the logits of view {op}')


def tta_view(x, op):
    """The forward view `op` of an fp32 CUDA tensor (N, C, H, W): a new tensor (N, C, H', W') (pp_tta_view, one launch)."""
    _check_op(op)
    _check(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    out = torch.empty((N, C) + view_shape(H, W, op), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        lib.pp_tta_view(x.data_ptr(), N * C, H, W, op, out.data_ptr(), stream_ptr())
    return out


def tta_predict(forward, image, mode, return_class=True):
    """The mean over the views of `mode` of ``softmax(forward(view(image)), dim=1)`` mapped back to the frame of `image`.
    `forward` maps an fp32 CUDA batch (N, C, H', W') to logits (N, K, H', W'), K <= 32; `image` is (N, C, H, W).  Returns
    ``prob`` (N, K, H, W) fp32, with ``return_class`` ``(prob, cls)``, cls (N, H, W) int64 = the first-maximum arg-max of prob.
    One accumulator is held; each view's logits are consumed before the next forward call."""
    ops = tta_ops(mode)
    _check(image, 'image')
    image = image.contiguous()
    N, _, H, W = image.shape
    acc, K = None, None
    with torch.cuda.device(image.device):
        for op in ops:
            z = forward(image if op == 0 else tta_view(image, op))
            _check_logits(z, N, H, W, op, K)
            z = z.contiguous()
            if acc is None:
                K = z.shape[1]
                acc = torch.empty((N, K, H, W), device=image.device, dtype=torch.float32)     # the first view stores: never read
            lib.pp_tta_accumulate(z.data_ptr(), N, K, H, W, op, int(op == ops[0]), acc.data_ptr(), stream_ptr())
            del z
        cls = torch.empty((N, H, W), device=image.device, dtype=torch.int64) if return_class else None
        lib.pp_tta_finalize(acc.data_ptr(), N, K, H, W, len(ops), cls.data_ptr() if return_class else None, stream_ptr())
    return (acc, cls) if return_class else acc
