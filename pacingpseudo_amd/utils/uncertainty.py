"""Uncertainty mask of the mean-teacher consistency term (UA-MT, Yu et al. 2019; its scribble variant USTM, Liu et al. 2022), on the
GPU.  The reference has no teacher; ``--cr_teacher ema`` added one, and this is what keeps it from pulling the student towards
regions where it is confidently wrong: the teacher runs T times on noise-perturbed inputs, the soft-max is averaged, and the
consistency term acts only where the predictive entropy is below a threshold that is relaxed over training.

    x_t   = x + clamp(sigma * n_t, -clip, +clip)            n_t ~ N(0, 1): Philox-4x32-10, Box-Muller (include/pacingpseudo_unc.h)
    pbar  = (1/T) sum_t softmax_k(teacher(x_t))             fp32, max-subtracted, t = 0 .. T-1 in order
    u     = -sum_k pbar_k ln pbar_k                         (a term with pbar_k = 0 is 0)
    m     = [u < theta] * valid_mask
    theta(e) = (start + (1 - start) * gaussian_ramp_up(e, 1.0, scale=ramp_up_scale)) * ln K

With sigma = 0 every pass would see the same input: T must be 1 and u is the plain entropy of the teacher's prediction.  The
stand-alone functions below are the pieces the training engine strings together (``StepEngine.set_uncertainty``); ``m`` is what
``losses.teacher_consistency_loss(..., valid_mask=m)`` takes.  All numeric defaults of the driver are untuned first values."""
import math

import torch

from .._lib import stream_ptr
from .utils import gaussian_ramp_up

MAX_PASSES = 16
MAX_CLASSES = 32
_U64 = (1 << 64) - 1


def check_uncertainty_params(passes=1, sigma=0.1, clip=0.2, start=0.75, seed=0, K=None) -> dict:
    """The accepted ranges of the punc_* entry points and of the threshold schedule, checked before any launch (no GPU needed):
    ValueError for values that are no pass count / width / fraction / seed at all or that contradict each other,
    NotImplementedError for sizes beyond what the kernels run.  Returns the normalised parameters."""
    if isinstance(passes, bool) or not isinstance(passes, (int, float)) or int(passes) != passes:
        raise ValueError(f'uncertainty: passes must be an integer (got {passes!r})')
    passes = int(passes)
    if passes < 1:
        raise ValueError(f'uncertainty: passes must be >= 1 (got {passes})')
    sigma, clip, start = float(sigma), float(clip), float(start)
    for name, v in (('sigma', sigma), ('clip', clip)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f'uncertainty: {name} must be a finite number >= 0 (got {v!r})')
    if not (0.0 < start <= 1.0):
        raise ValueError(f'uncertainty: start must lie in (0, 1] (got {start!r})')
    if sigma == 0.0 and passes != 1:
        raise ValueError(f'uncertainty: sigma = 0 makes every pass identical, so passes must be 1 (got {passes})')
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f'uncertainty: seed must be an integer (got {seed!r})')
    if not (0 <= seed <= _U64):
        raise ValueError(f'uncertainty: seed must fit 64 unsigned bits (got {seed})')
    if K is not None:
        if int(K) < 2:
            raise ValueError(f'uncertainty: the entropy of a soft-max over K = {K} class(es) is constant; K >= 2')
        if int(K) > MAX_CLASSES:
            raise NotImplementedError(f'uncertainty: K <= {MAX_CLASSES} classes (got {K})')
    if passes > MAX_PASSES:
        raise NotImplementedError(f'uncertainty: passes <= {MAX_PASSES} (got {passes})')
    return dict(passes=passes, sigma=sigma, clip=clip, start=start, seed=seed)


def uncertainty_threshold(epoch, start, num_classes, scale=5.0) -> float:
    """theta(epoch): ``start * ln K`` at the beginning (up to the ramp's own value at 0, exp(-scale)), ``ln K`` -- every pixel passes
    but the exactly uniform ones -- once the ramp has run out (gaussian_ramp_up's 80 epochs)."""
    if int(num_classes) < 2:
        raise ValueError(f'uncertainty: K >= 2 (got {num_classes})')
    if not (0.0 < float(start) <= 1.0):
        raise ValueError(f'uncertainty: start must lie in (0, 1] (got {start!r})')
    s = float(start)
    return (s + (1.0 - s) * gaussian_ramp_up(epoch, 1.0, scale=scale)) * math.log(int(num_classes))


def state_tensor(seed, step, device) -> torch.Tensor:
    """The (seed, step) pair as the kernels read it: two 64-bit words on the device (int64 holding the unsigned bits)."""
    def signed(v):
        v = int(v) & _U64
        return v - (1 << 64) if v >= (1 << 63) else v
    return torch.tensor([signed(seed), signed(step)], dtype=torch.int64, device=device)


def _check_cuda_f32(x, what):
    if not torch.is_tensor(x):
        raise ValueError(f'{what} must be a torch tensor, got {type(x).__name__}')
    if x.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {x.dtype}')
    if not x.is_cuda:
        raise ValueError(f'{what} must be a CUDA tensor: there is no CPU path')
    if x.numel() < 1:
        raise ValueError(f'{what} is empty: {tuple(x.shape)}')


def add_noise(image, sigma, clip, seed, step, pass_index, out=None) -> torch.Tensor:
    """``image + clamp(sigma * n, -clip, +clip)`` with the noise of (seed, step, pass_index); element i of the flattened tensor
    always receives the same value, whatever the shape.  `image` fp32 CUDA, contiguous (a contiguous slice works: the kernel takes
    4-byte accesses where a pointer is not 16-byte aligned, with the same bits)."""
    from .._unc import unc
    _check_cuda_f32(image, 'image')
    prm = check_uncertainty_params(1 if float(sigma) == 0.0 else 2, sigma, clip, 1.0, int(seed))
    if isinstance(pass_index, bool) or int(pass_index) != pass_index or not (0 <= int(pass_index) < MAX_PASSES):
        raise ValueError(f'uncertainty: pass_index must be an integer in [0, {MAX_PASSES}) (got {pass_index!r})')
    if not image.is_contiguous():
        image = image.contiguous()
    if out is None:
        out = torch.empty_like(image)
    elif out.shape != image.shape or out.dtype != torch.float32 or out.device != image.device or not out.is_contiguous():
        raise ValueError('out must be a contiguous float32 tensor of the image\'s shape on its device')
    with torch.cuda.device(image.device):
        state = state_tensor(seed, step, image.device)
        unc.punc_noise_add(image.data_ptr(), image.numel(), prm['sigma'], prm['clip'], state.data_ptr(), int(pass_index),
                           out.data_ptr(), stream_ptr())
        state.record_stream(torch.cuda.current_stream())
    return out


def uncertainty_mask(logits, threshold, valid_mask=None, return_uncertainty=False, return_stats=False):
    """Mask of the pixels whose mean-soft-max entropy is below `threshold`.  `logits`: a list / tuple of T (N, K, H, W) fp32 CUDA
    tensors (the teacher's outputs for the T noisy inputs), or a callable ``t -> logits`` paired with its pass count as
    ``(callable, T)``.  `valid_mask` (N, 1, H, W) or (N, H, W) fp32, or None.  Returns the mask (N, 1, H, W) fp32; with
    ``return_uncertainty`` also u (N, H, W); with ``return_stats`` also a float64 device tensor (sum of the mask, sum of u over
    valid pixels, number of valid pixels)."""
    from .._unc import unc
    if isinstance(logits, tuple) and len(logits) == 2 and callable(logits[0]):
        fn, T = logits
        get = fn
    elif callable(logits):
        raise ValueError('uncertainty_mask: pass a callable together with its number of passes, as (callable, T)')
    else:
        seq = list(logits)
        T = len(seq)
        get = seq.__getitem__
    threshold = float(threshold)
    if not math.isfinite(threshold):
        raise ValueError(f'uncertainty: the threshold must be finite (got {threshold!r})')
    if T < 1:
        raise ValueError('uncertainty_mask: no logits')
    if T > MAX_PASSES:
        raise NotImplementedError(f'uncertainty: passes <= {MAX_PASSES} (got {T})')
    first = get(0)
    _check_cuda_f32(first, 'logits')
    if first.dim() != 4:
        raise ValueError(f'logits must be (N, K, H, W), got {tuple(first.shape)}')
    N, K, H, W = first.shape
    check_uncertainty_params(T, 1.0, 0.0, 1.0, 0, K=K)
    if N * H * W >= 2 ** 31:
        raise NotImplementedError(f'uncertainty: N * H * W < 2^31 (got {N * H * W})')
    dev = first.device
    if valid_mask is not None:
        _check_cuda_f32(valid_mask, 'valid_mask')
        if valid_mask.numel() != N * H * W or valid_mask.device != dev:
            raise ValueError(f'valid_mask must hold one value per pixel of logits {tuple(first.shape)} on {dev}, got {tuple(valid_mask.shape)}')
        valid_mask = valid_mask.contiguous()
    with torch.cuda.device(dev):
        nws = unc.punc_workspace_bytes(N, K, H * W)
        ws = torch.empty(max(nws // 8, 1), device=dev, dtype=torch.float64)
        acc = torch.empty((N, K, H, W), device=dev, dtype=torch.float32) if T > 1 else first
        mask = torch.empty((N, 1, H, W), device=dev, dtype=torch.float32)
        u = torch.empty((N, H, W), device=dev, dtype=torch.float32) if return_uncertainty else None
        stats = torch.empty(3, device=dev, dtype=torch.float64)
        for t in range(T):
            z = first if t == 0 else get(t)
            if t:
                _check_cuda_f32(z, f'logits[{t}]')
                if z.shape != first.shape or z.device != dev:
                    raise ValueError(f'logits[{t}] is {tuple(z.shape)} on {z.device}, logits[0] {tuple(first.shape)} on {dev}')
            z = z.contiguous()
            unc.punc_accumulate(z.data_ptr(), N, K, H * W, t, T, valid_mask.data_ptr() if valid_mask is not None else None, threshold,
                                acc.data_ptr(), mask.data_ptr(), u.data_ptr() if u is not None else None, stats.data_ptr(),
                                ws.data_ptr(), ws.numel() * 8, stream_ptr())
    res = (mask,) + ((u,) if return_uncertainty else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res
