"""Mean-field CRF refinement of a soft-max on the GPU: the post-processing step of scribble-supervised segmentation that looks at
the image between "probabilities" and "arg-max".  The reference scores its raw arg-max (inference.py:159-190); this is an
addition, off by default in ``inference.py`` (``--crf_refine T``).  It is the inference counterpart of ``losses.gated_crf_loss``:
the same window, the same bilateral kernel, the same limits.

With ``j = i + (dy, dx) * dilation``, ``dy, dx`` in ``[-radius, radius]`` without ``(0, 0)`` and ``j`` inside the image::

    kb_ij = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))
    ks_ij = exp(-(dy^2 + dx^2) / (2 sigma_smooth^2))
    Q^0 = softmax(logits),  u = log_softmax(logits)
    Q^{t+1}_i = softmax_c(u_ic + w_bilateral * sum_j kb_ij Q^t_jc / (sum_j kb_ij + 1e-6)
                               + w_smooth    * sum_j ks_ij Q^t_jc / (sum_j ks_ij + 1e-6))

Potts compatibility, normalised messages (the weights are in logit units and do not depend on the window size), parallel update.
One pp_crf_refine call: one launch per iteration, no atomics, no host synchronisation -- the same bits in every run and, per
slice, whatever the batch around it.  The window and the two sigmas of the bilateral kernel default to the loss's; ``sigma_smooth``
and the two weights are untuned first values."""
import math

import torch

from .._lib import lib, stream_ptr
from ..losses.losses import check_crf_params

MAX_ITERATIONS = 64


def check_crf_refine_params(iterations=5, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, sigma_smooth=1.5, w_bilateral=4.0,
                            w_smooth=1.0, K=None, C=None) -> dict:
    """The accepted ranges of pp_crf_refine (include/pacingpseudo_hip.h), checked before any launch, on top of
    losses.check_crf_params and with its split: ValueError for values that are no iteration count / width / weight at all,
    NotImplementedError for sizes beyond what the kernel runs.  Returns the normalised parameters."""
    prm = check_crf_params(radius, dilation, sigma_xy, sigma_rgb, K=K, C=C)
    if isinstance(iterations, bool) or int(iterations) != iterations:
        raise ValueError(f'CRF refinement: iterations must be an integer (got {iterations!r})')
    iterations, sigma_smooth, w_bilateral, w_smooth = int(iterations), float(sigma_smooth), float(w_bilateral), float(w_smooth)
    if iterations < 1:
        raise ValueError(f'CRF refinement: iterations must be >= 1 (got {iterations})')
    if not (sigma_smooth > 0.0 and math.isfinite(sigma_smooth)):
        raise ValueError(f'CRF refinement: sigma_smooth must be a positive finite number (got {sigma_smooth!r})')
    for name, v in (('w_bilateral', w_bilateral), ('w_smooth', w_smooth)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f'CRF refinement: {name} must be a finite number >= 0 (got {v!r})')
    if iterations > MAX_ITERATIONS:
        raise NotImplementedError(f'CRF refinement: iterations <= {MAX_ITERATIONS} (got {iterations})')
    prm.update(iterations=iterations, sigma_smooth=sigma_smooth, w_bilateral=w_bilateral, w_smooth=w_smooth)
    return prm


def _check(x, what):
    """ValueError before the library is touched, unless x is an fp32 (N, C, H, W) tensor the kernel can index."""
    if not torch.is_tensor(x):
        raise ValueError(f'{what} must be a torch tensor, got {type(x).__name__}')
    if x.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {x.dtype}')
    if x.dim() != 4:
        raise ValueError(f'{what} must be (N, C, H, W), got {tuple(x.shape)}')
    if min(x.shape) < 1:
        raise ValueError(f'{what} has an empty axis: {tuple(x.shape)}')
    if x.numel() >= 2 ** 31:
        raise ValueError(f'{what} has {x.numel()} elements; the kernel indexes with 32 bits (N*C*H*W < 2^31)')


def crf_refine(logits, image, iterations=5, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, sigma_smooth=1.5, w_bilateral=4.0,
               w_smooth=1.0, return_class=True):
    """``iterations`` mean-field steps on ``softmax(logits, 1)`` guided by ``image`` (the module docstring has the definition).
    `logits` is (N, K, H, W), K <= 32, `image` (N, C, H, W), C <= 4, both fp32 CUDA.  Returns ``(prob, cls)``: prob (N, K, H, W)
    fp32, cls (N, H, W) int64 = the first-maximum arg-max of prob, or None without ``return_class``."""
    _check(logits, 'logits')
    _check(image, 'image')
    N, K, H, W = logits.shape
    if image.shape[0] != N or tuple(image.shape[2:]) != (H, W):
        raise ValueError(f'image must be (N, C, H, W) with the N, H, W of logits {tuple(logits.shape)}, got {tuple(image.shape)}')
    for x, what in ((logits, 'logits'), (image, 'image')):
        if not x.is_cuda:
            raise ValueError(f'{what} must be a CUDA tensor: there is no CPU path')
    if image.device != logits.device:
        raise ValueError(f'image is on {image.device}, logits on {logits.device}')
    prm = check_crf_refine_params(iterations, radius, dilation, sigma_xy, sigma_rgb, sigma_smooth, w_bilateral, w_smooth, K=K,
                                  C=image.shape[1])
    logits, image = logits.contiguous(), image.contiguous()
    prob = torch.empty_like(logits)
    cls = torch.empty((N, H, W), device=logits.device, dtype=torch.int64) if return_class else None
    nws = lib.pp_crf_refine_workspace(N, K, H, W)
    ws = torch.empty(nws, device=logits.device, dtype=torch.uint8)
    with torch.cuda.device(logits.device):
        lib.pp_crf_refine(logits.data_ptr(), image.data_ptr(), N, K, image.shape[1], H, W, prm['iterations'], prm['radius'], prm['dilation'],
                          prm['sigma_xy'], prm['sigma_rgb'], prm['sigma_smooth'], prm['w_bilateral'], prm['w_smooth'], prob.data_ptr(),
                          cls.data_ptr() if return_class else None, ws.data_ptr(), nws, stream_ptr())
    return prob, cls
