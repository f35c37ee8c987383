"""Segmented stable descending sort on the GPU (libpacingpseudo_lov.so): the radix sort the Lovasz-softmax loss orders its pixel
errors with (``losses.lovasz_softmax_loss``), on full 32-bit keys."""
import torch

from .._lib import stream_ptr


def sort_descending(values):
    """(sorted, perm) of `values`, a float32 CUDA tensor (S, n): every row in descending order, stable -- equal to
    ``torch.sort(values, dim=1, descending=True, stable=True)`` for every float32 input: -0 ties with +0, every NaN counts as the one
    value above +inf, equal values keep their order.  `sorted` holds the input's own bit patterns, `perm` is int32.  S * n < 2^31."""
    if not torch.is_tensor(values):
        raise ValueError(f'values must be a torch tensor, got {type(values).__name__}')
    if values.dtype != torch.float32 or values.dim() != 2:
        raise ValueError(f'values must be float32 (S, n), got {values.dtype} {tuple(values.shape)}')
    S, n = values.shape
    if S < 1 or n < 1 or S * n >= 2 ** 31:
        raise ValueError(f'values is {(S, n)}: need S >= 1, n >= 1 and S * n < 2^31')
    if not values.is_cuda:
        raise ValueError('values must be a CUDA tensor: there is no CPU path')
    from .._lov import lov
    v = values.detach().contiguous()
    out = torch.empty_like(v)
    perm = torch.empty((S, n), device=v.device, dtype=torch.int32)
    with torch.cuda.device(v.device):
        nws = lov.plov_sort_workspace(S, n)
        ws = torch.empty(max(nws // 8, 1), device=v.device, dtype=torch.float64)
        lov.plov_sort_descending(v.data_ptr(), S, n, out.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream_ptr())
    return out, perm
