"""Loss functions of PacingPseudo with the reference's names and call signatures (losses/losses.py:9-116),
evaluated by the fused HIP loss kernels of libpacingpseudo_hip.so.

Inside ``ConsistencyRegulr`` the five losses of a step are produced by ONE fused forward and ONE fused backward
launch sequence (pacingpseudo_amd/engine.py).  The functions below expose the same kernels one loss at a time for
code that calls the reference's functional API directly; each is a ``torch.autograd.Function`` whose backward
runs the matching HIP gradient kernel.  Inputs are NCHW float32 CUDA tensors, exactly as in the reference.

``soft_label_cross_entropy_loss`` / ``l1_loss`` / ``l2_loss`` receive the target as probabilities and, like the
reference's (losses/losses.py:45-96), differentiate through it: the gradient with respect to ``input`` comes from the
HIP kernel, the one with respect to ``target`` -- element-wise, -mask * log_softmax(input) / D and its L1 / L2
counterparts -- is attached by ``_TargetGrad`` when the target requires one (round 4; before, the target was silently
a constant).  The in-model path evaluates both gradients inside the fused kernels (consistency_reglur_memory.py:53-54).
The targets are expected to be normalised distributions (they pass through log / soft-max on their way to the kernels).
"""
from __future__ import annotations

import torch

from .._lib import lib, stream_ptr
from ..regop import (CRF_MAX_CHANNELS, CRF_MAX_CLASSES, CRF_MAX_DILATION, CRF_MAX_HALO, CRF_MAX_RADIUS, MS_MAX_CHANNELS,  # noqa: F401
                     MS_MAX_CLASSES, REGULARISERS, RegOp, check_crf_params, check_ms_params, check_nc_params)

# cr_variant codes of pp_seg_losses_fwd / _bwd (include/pacingpseudo_hip.h); engine.CR_VARIANTS is this table
_VARIANT = {'ce_loss': 1, 'l1_loss': 2, 'l2_loss': 3, 'kl_loss': 4, 'bikl_loss': 5, 'js_loss': 6, 'hard_ce_loss': 7}


def _check(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise TypeError(f'{name} must be a 4-D float32 CUDA tensor (N,C,H,W)')
    return t.contiguous()


class _SegLoss(torch.autograd.Function):
    """which: 0 = partial CE, 1 = entropy, 2 = consistency(variant)."""

    @staticmethod
    def forward(ctx, zw, zs, target, mask, ignore_index, which, variant, detach_weak):
        N, K, H, W = zw.shape
        st = stream_ptr()
        dev = zw.device
        sums = torch.zeros(6, device=dev, dtype=torch.float64)
        nws = lib.pp_seg_losses_workspace(N, H * W)
        ws = torch.empty(nws + 64, device=dev, dtype=torch.uint8)
        if target is None:
            target = torch.full((N, H, W), ignore_index, device=dev, dtype=torch.int64)
        lib.pp_seg_losses_fwd(zw.data_ptr(), zs.data_ptr() if zs is not None else None, target.data_ptr(),
                              mask.data_ptr() if mask is not None else None, N, K, H * W, ignore_index,
                              1 if which == 1 else 0, variant if which == 2 else 0, sums.data_ptr(), ws.data_ptr(), nws, st)
        out = torch.empty((), device=dev, dtype=torch.float32)
        ptrs = [None, None, None]
        ptrs[which] = out.data_ptr()
        lib.pp_losses_finalize(sums.data_ptr(), 1 if mask is not None else 0, *ptrs, st)
        ctx.save_for_backward(zw, zs if zs is not None else zw, target, mask if mask is not None else zw, sums)
        ctx.cfg = (zs is not None, mask is not None, ignore_index, which, variant, detach_weak)
        return out

    @staticmethod
    def backward(ctx, g):
        zw, zs, target, mask, sums = ctx.saved_tensors
        has_s, has_m, ignore_index, which, variant, detach_weak = ctx.cfg
        N, K, H, W = zw.shape
        g = g.to(torch.float32).contiguous()
        gp = [None, None, None]
        gp[which] = g.data_ptr()
        dzw = torch.empty_like(zw)
        dzs = torch.empty_like(zs) if has_s else None
        lib.pp_seg_losses_bwd(zw.data_ptr(), zs.data_ptr() if has_s else None, target.data_ptr(),
                              mask.data_ptr() if has_m else None, N, K, H * W, ignore_index, 1 if which == 1 else 0,
                              variant if which == 2 else 0, 1 if detach_weak else 0, sums.data_ptr(), gp[0], gp[1], gp[2],
                              1.0, dzw.data_ptr(), dzs.data_ptr() if has_s else None, stream_ptr())
        return dzw, dzs, None, None, None, None, None, None


def partial_cross_entropy_loss(input, target, ignore_index):
    """F.cross_entropy(input, target, ignore_index): mean over labelled pixels (losses/losses.py:35-43)."""
    zw = _check(input, 'input')
    t = target.to(torch.int64).contiguous()
    return _SegLoss.apply(zw, None, t, None, int(ignore_index), 0, 0, False)


def cross_entropy_loss(input, target):
    """Plain mean cross entropy on (N,C,H,W) logits / (N,H,W) targets or (N,C) / (N) (losses/losses.py:26-33)."""
    if input.dim() == 2:
        input = input.t().contiguous()[None, :, :, None].contiguous()      # (1,C,N,1)
        target = target[None, :, None]
    return partial_cross_entropy_loss(input, target, -100)


def entropy_minimization_loss(input, valid_mask=None):
    """Masked mean of the per-pixel soft-max entropy (losses/losses.py:9-24)."""
    zw = _check(input, 'input')
    m = _check(valid_mask, 'valid_mask') if valid_mask is not None else None
    return _SegLoss.apply(zw, None, None, m, -100, 1, 0, False)


def _consistency(strong_logits, weak_logits, valid_mask, variant, detach_weak):
    zs, zw = _check(strong_logits, 'input'), _check(weak_logits, 'target')
    m = _check(valid_mask, 'valid_mask') if valid_mask is not None else None
    return _SegLoss.apply(zw, zs, None, m, -100, 2, _VARIANT[variant], detach_weak)


def _logits_of(prob):
    return torch.log(prob.detach().clamp_min(1e-38))


class _TargetGrad(torch.autograd.Function):
    """A zero-valued term that carries d loss / d target for the probability-target losses: forward returns 0, backward
    returns g * dLdt, where dLdt is the closed-form element-wise derivative (no reduction: plain tensor plumbing)."""

    @staticmethod
    def forward(ctx, target, dLdt):
        ctx.save_for_backward(dLdt)
        return torch.zeros((), device=target.device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        (dLdt,) = ctx.saved_tensors
        return g * dLdt, None


def _with_target_grad(loss, target, make_dLdt, valid_mask, per_pixel: bool):
    """loss + 0 * (term whose gradient w.r.t. `target` is make_dLdt() * mask / denominator).  Denominators as in the
    reference: max(sum(mask), 1e-8) when masked; else the element count of the un-reduced loss tensor -- (N,C,H,W) for the
    soft-label CE, (N,1,H,W) for L1 / L2 (losses/losses.py:56-61, 74-78, 91-95)."""
    if not (torch.is_tensor(target) and target.requires_grad and torch.is_grad_enabled()):
        return loss
    with torch.no_grad():
        d = make_dLdt()
        if valid_mask is not None:
            d = d * valid_mask / valid_mask.sum().clamp_min(1e-8)
        else:
            N, C, H, W = target.shape
            d = d / float(N * H * W * (1 if per_pixel else C))
    return loss + _TargetGrad.apply(target, d)


def soft_label_cross_entropy_loss(input, target, valid_mask=None):
    """-sum_c target_c * log_softmax(input)_c, masked mean (losses/losses.py:45-62).  `target`: probabilities; gradients
    flow into both arguments."""
    loss = _consistency(input, _logits_of(target), valid_mask, 'ce_loss', True)
    return _with_target_grad(loss, target, lambda: -torch.log_softmax(input.detach(), 1), valid_mask, per_pixel=False)


def l1_loss(input, target, valid_mask=None):
    """sum_c |input_c - target_c| on probabilities, masked mean (losses/losses.py:64-79)."""
    loss = _consistency(_logits_keep_grad(input), _logits_of(target), valid_mask, 'l1_loss', True)
    return _with_target_grad(loss, target, lambda: -torch.sign(input.detach() - target.detach()), valid_mask, per_pixel=True)


def l2_loss(input, target, valid_mask=None):
    """sum_c (input_c - target_c)^2 on probabilities, masked mean (losses/losses.py:81-96)."""
    loss = _consistency(_logits_keep_grad(input), _logits_of(target), valid_mask, 'l2_loss', True)
    return _with_target_grad(loss, target, lambda: -2.0 * (input.detach() - target.detach()), valid_mask, per_pixel=True)


def _logits_keep_grad(prob):
    # softmax(log p) == p for a normalised p, so the probability-space losses reuse the logit-space kernels
    return torch.log(prob.clamp_min(1e-38))


def kl_loss(input, target, valid_mask=None):
    """KL(softmax(target) || softmax(input)) element-wise, masked mean; both arguments are logits and both
    receive gradients (losses/losses.py:98-116)."""
    return _consistency(input, target, valid_mask, 'kl_loss', False)


def bidirectional_kl_loss(input, target, valid_mask=None):
    """(KL(softmax(target) || softmax(input)) + KL(softmax(input) || softmax(target))) / 2 element-wise, masked mean; both
    arguments are logits and both receive gradients (losses/losses.py:118-145)."""
    return _consistency(input, target, valid_mask, 'bikl_loss', False)


def js_loss(input, target, valid_mask=None):
    """Jensen-Shannon divergence of softmax(input) and softmax(target) per pixel (in [0, ln 2]), masked mean over the pixels (this
    implementation's addition; the reference has no such loss); both arguments are logits and both receive gradients."""
    return _consistency(input, target, valid_mask, 'js_loss', False)


def hard_label_cross_entropy_loss(input, target, valid_mask=None):
    """Cross entropy of softmax(input) against the arg-max over the channels of `target` (first maximum, as torch.argmax), masked
    mean over the pixels (this implementation's addition; the reference has no such loss).  `target` is a constant: it gets a zero
    gradient."""
    return _consistency(input, target.detach() if torch.is_tensor(target) else target, valid_mask, 'hard_ce_loss', True)


class _TeacherLoss(torch.autograd.Function):
    """The consistency term of a mean-teacher step, as StepEngine runs it (--cr_teacher ema): the TEACHER call of the two-call
    composition -- pp_seg_losses_fwd(teacher, student, ..., do_ent 0, variant) for the sums, pp_seg_losses_bwd with the partial-CE
    slot's upstream gradient a device zero, no entropy and the weak side detached for the gradient wrt the student logits; the
    gradient wrt the teacher logits lands in a buffer that is dropped."""

    @staticmethod
    def forward(ctx, zs, zt, mask, variant):
        N, K, H, W = zs.shape
        st = stream_ptr()
        dev = zs.device
        sums = torch.zeros(6, device=dev, dtype=torch.float64)
        nws = lib.pp_seg_losses_workspace(N, H * W)
        ws = torch.empty(nws + 64, device=dev, dtype=torch.uint8)
        target = torch.full((N, H, W), -100, device=dev, dtype=torch.int64)
        lib.pp_seg_losses_fwd(zt.data_ptr(), zs.data_ptr(), target.data_ptr(), mask.data_ptr() if mask is not None else None,
                              N, K, H * W, -100, 0, variant, sums.data_ptr(), ws.data_ptr(), nws, st)
        out = torch.empty((), device=dev, dtype=torch.float32)
        lib.pp_losses_finalize(sums.data_ptr(), 1 if mask is not None else 0, None, None, out.data_ptr(), st)
        ctx.save_for_backward(zs, zt, target, mask if mask is not None else zs, sums)
        ctx.cfg = (mask is not None, variant)
        return out

    @staticmethod
    def backward(ctx, g):
        zs, zt, target, mask, sums = ctx.saved_tensors
        has_m, variant = ctx.cfg
        N, K, H, W = zs.shape
        g = g.to(torch.float32).contiguous()
        zero = torch.zeros(1, device=zs.device, dtype=torch.float32)
        dzs, discard = torch.empty_like(zs), torch.empty_like(zt)
        lib.pp_seg_losses_bwd(zt.data_ptr(), zs.data_ptr(), target.data_ptr(), mask.data_ptr() if has_m else None, N, K, H * W,
                              -100, 0, variant, 1, sums.data_ptr(), zero.data_ptr(), None, g.data_ptr(), 1.0, discard.data_ptr(),
                              dzs.data_ptr(), stream_ptr())
        return dzs, None, None, None


def teacher_consistency_loss(student_logits, teacher_logits, variant='ce_loss', valid_mask=None):
    """Consistency of a student's (strong-view) logits with a teacher's (weak-view) logits, the teacher a constant (mean teacher):
    the form `variant` of --loss_cr_variants with softmax(teacher_logits) -- hard_ce_loss: its arg-max -- as the target, masked
    mean.  Returns the 0-dim loss; differentiable in `student_logits` only (the teacher's ``.grad`` stays None).

    `valid_mask` (N, 1, H, W) fp32 is any per-pixel weight of the masked mean ``sum(m d) / max(sum(m), 1e-8)``: the batch's valid
    mask, or the uncertainty mask ``m = utils.uncertainty_mask(noisy teacher logits, theta, valid_mask)`` of ``--cr_uncertainty``
    (which already holds the valid mask).  An all-zero mask gives a loss of 0 with a zero gradient."""
    zs, zt = _check(student_logits, 'student_logits'), _check(teacher_logits, 'teacher_logits')
    if variant not in _VARIANT:
        raise ValueError(f'variant must be one of {sorted(_VARIANT)}, got {variant!r}')
    if zs.shape != zt.shape:
        raise ValueError(f'student_logits {tuple(zs.shape)} and teacher_logits {tuple(zt.shape)} must have the same shape')
    m = None
    if valid_mask is not None:
        m = _check(valid_mask, 'valid_mask')
        if tuple(m.shape) != (zs.shape[0], 1) + tuple(zs.shape[2:]):
            raise ValueError(f'valid_mask must be {(zs.shape[0], 1) + tuple(zs.shape[2:])}, got {tuple(m.shape)}')
    return _TeacherLoss.apply(zs, zt.detach(), m, _VARIANT[variant])


class _DiceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, label):
        N, K, H, W = z.shape
        st = stream_ptr()
        sums = torch.empty((N, K, 3), device=z.device, dtype=torch.float64)
        nws = lib.pp_dice_loss_workspace(N, K)
        ws = torch.empty(nws, device=z.device, dtype=torch.uint8)
        out = torch.empty((), device=z.device, dtype=torch.float32)
        lib.pp_dice_loss_fwd(z.data_ptr(), label.data_ptr(), N, K, H * W, sums.data_ptr(), out.data_ptr(), ws.data_ptr(), nws, st)
        ctx.save_for_backward(z, label, sums)
        return out

    @staticmethod
    def backward(ctx, g):
        z, label, sums = ctx.saved_tensors
        N, K, H, W = z.shape
        g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        lib.pp_dice_loss_bwd(z.data_ptr(), label.data_ptr(), N, K, H * W, sums.data_ptr(), g.data_ptr(), 1.0, dz.data_ptr(), 0,
                             stream_ptr())
        return dz, None


def dice_loss_fn(input, target):
    """-mean_{n,c} 2 sum(p t) / (sum p + sum t + 1e-5) on softmax(input) vs the one-hot target (losses/losses.py:147-162;
    the fully-supervised trainer upper_bound_chaos.py:165 adds it to the cross entropy)."""
    return _DiceLoss.apply(_check(input, 'input'), _check(target, 'target'))


class _BoundaryLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, phi):
        from .._dist import dist
        N, K, H, W = z.shape
        with torch.cuda.device(z.device):
            nws = dist.pdist_boundary_loss_workspace(N, K, H, W)
            ws = torch.empty(max(nws // 8, 1), device=z.device, dtype=torch.float64)
            out = torch.empty((), device=z.device, dtype=torch.float32)
            dist.pdist_boundary_loss_fwd(z.data_ptr(), phi.data_ptr(), N, K, H, W, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                         stream_ptr())
        ctx.save_for_backward(z, phi)
        return out

    @staticmethod
    def backward(ctx, g):
        from .._dist import dist
        z, phi = ctx.saved_tensors
        N, K, H, W = z.shape
        g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        with torch.cuda.device(z.device):
            dist.pdist_boundary_loss_bwd(z.data_ptr(), phi.data_ptr(), N, K, H, W, g.data_ptr(), dz.data_ptr(), stream_ptr())
        return dz, None


def boundary_loss(input, target, dist_maps=None, spacing=(1., 1.)):
    """Boundary loss of Kervadec et al. (MIDL 2019): mean over n, the foreground classes k = 1 .. K-1 (k = 0 when K = 1) and the pixels
    of softmax_k(input) * phi_k, phi the signed distance maps of the label (``utils.signed_distance_maps``: negative inside a
    class, positive outside, in units of `spacing`).  `target`: the one-hot label (N, K, H, W) as ``dice_loss_fn`` takes it (its
    arg-max is the class map) or an int64 class map (N, H, W); with `dist_maps` (N, K, H, W) fp32 given, that phi is used as it is
    and `target` is not read.  phi receives no gradient.  The reference has no such loss (upper_bound_chaos.py --do_loss_boundary)."""
    from ..utils.distance import MAX_CLASSES, MAX_SIDE, check_spacing, signed_distance_maps
    if not (torch.is_tensor(input) and input.dtype == torch.float32 and input.dim() == 4):
        raise ValueError('input must be a 4-D float32 CUDA tensor (N,K,H,W)')
    N, K, H, W = input.shape
    if min(input.shape) < 1 or K > MAX_CLASSES or max(H, W) > MAX_SIDE or input.numel() >= 2 ** 31:
        raise ValueError(f'input is {tuple(input.shape)}: need 1 <= K <= {MAX_CLASSES}, 1 <= H, W <= {MAX_SIDE}, N*K*H*W < 2^31')
    spacing = check_spacing(spacing)
    if dist_maps is not None:
        if not (torch.is_tensor(dist_maps) and dist_maps.dtype == torch.float32 and tuple(dist_maps.shape) == (N, K, H, W)):
            raise ValueError(f'dist_maps must be a float32 tensor of input\'s shape {(N, K, H, W)}')
        if not (dist_maps.is_cuda and dist_maps.device == input.device):
            raise ValueError('dist_maps must be a CUDA tensor on input\'s device')
    else:
        if not torch.is_tensor(target):
            raise ValueError(f'target must be a torch tensor, got {type(target).__name__}')
        if target.dim() == 4:
            if tuple(target.shape) != (N, K, H, W):
                raise ValueError(f'a one-hot target must have input\'s shape {(N, K, H, W)}, got {tuple(target.shape)}')
        elif target.dim() == 3:
            if target.dtype != torch.int64 or tuple(target.shape) != (N, H, W):
                raise ValueError(f'a class-map target must be int64 {(N, H, W)}, got {target.dtype} {tuple(target.shape)}')
        else:
            raise ValueError(f'target must be one-hot (N, K, H, W) or an int64 class map (N, H, W), got {tuple(target.shape)}')
        if not (target.is_cuda and target.device == input.device):
            raise ValueError('target must be a CUDA tensor on input\'s device')
    if not input.is_cuda:
        raise ValueError('input must be a CUDA tensor: there is no CPU path')
    if dist_maps is None:
        with torch.no_grad():
            cls = torch.argmax(target, dim=1) if target.dim() == 4 else target
            dist_maps = signed_distance_maps(cls, K, spacing)
    return _BoundaryLoss.apply(input.contiguous(), dist_maps.detach().contiguous())


LOVASZ_MIN_CLASSES, LOVASZ_MAX_CLASSES = 2, 32


class _LovaszSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, cls, ignore_index, per_image, classes_all, parts):
        from .._lov import lov
        N, K, H, W = z.shape
        P = N * H * W
        has_ignore = int(ignore_index is not None)
        ign = int(ignore_index) if has_ignore else 0
        with torch.cuda.device(z.device):
            nws = lov.plov_loss_workspace(N, K, H, W, int(per_image))
            ws = torch.empty(max(nws // 8, 1), device=z.device, dtype=torch.float64)
            out = torch.empty((), device=z.device, dtype=torch.float32)
            weights = torch.empty((K, P), device=z.device, dtype=torch.float32)
            scale = torch.empty(N * K if per_image else K, device=z.device, dtype=torch.float32)
            errors = torch.empty((K, P), device=z.device, dtype=torch.float32) if parts else None
            perm = torch.empty((N * K, H * W) if per_image else (K, P), device=z.device, dtype=torch.int32) if parts else None
            lov.plov_loss_fwd(z.data_ptr(), cls.data_ptr(), N, K, H, W, has_ignore, ign, int(per_image), int(classes_all), out.data_ptr(),
                              weights.data_ptr(), scale.data_ptr(), errors.data_ptr() if parts else None,
                              perm.data_ptr() if parts else None, ws.data_ptr(), ws.numel() * 8, stream_ptr())
        ctx.save_for_backward(z, cls, weights, scale)
        ctx.flags = (has_ignore, ign, int(per_image))
        if parts:
            ctx.mark_non_differentiable(errors, perm, weights)
            return out, errors, perm, weights
        return out

    @staticmethod
    def backward(ctx, g, *unused):
        from .._lov import lov
        z, cls, weights, scale = ctx.saved_tensors
        N, K, H, W = z.shape
        has_ignore, ign, per_image = ctx.flags
        g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        with torch.cuda.device(z.device):
            lov.plov_loss_bwd(z.data_ptr(), cls.data_ptr(), N, K, H, W, has_ignore, ign, per_image, weights.data_ptr(), scale.data_ptr(),
                              g.data_ptr(), dz.data_ptr(), stream_ptr())
        return dz, None, None, None, None, None


def lovasz_softmax_loss(input, target, ignore_index=None, per_image=False, classes='present', return_parts=False):
    """Lovasz-softmax loss of Berman, Triki and Blaschko (CVPR 2018) on softmax(input): for every class c the errors
    e_i = |[target_i == c] - p_ci| of the valid pixels, sorted in descending order (ties in ascending (n, y, x) pixel index), weighted
    by the increments of the Jaccard loss along that order and summed; the mean over the classes that occur (``classes='present'``)
    or over all K (``'all'``).  ``per_image``: that loss per image, averaged over all N images (an image without a present class
    counts 0).  A pixel is valid when 0 <= target < K and target != ignore_index; any other value is ignored.  No valid pixel of a
    present class at all: loss 0, gradient 0.  A non-finite logit gives NaN.

    `input` fp32 (N, K, H, W) with 2 <= K <= 32 and N*K*H*W < 2^31; `target` the one-hot label (N, K, H, W) as ``dice_loss_fn`` takes
    it (its arg-max is the class map) or an int64 class map (N, H, W).  Sorted, scanned and reduced on the device
    (libpacingpseudo_lov.so) without a device-to-host read; same bits in every run.

    ``return_parts=True`` returns (loss, errors, perm, weights), the last three detached: errors fp32 (K, N*H*W), e in pixel order (0
    at ignored pixels); perm int32, one row per segment -- (K, N*H*W), or (N*K, H*W) image-major with ``per_image`` -- of FLATTENED
    (n, y, x) pixel indices into N*H*W in sorted order, in both modes, the segment's ignored pixels last in ascending index order;
    weights fp32 (K, N*H*W), the increment g at every pixel's rank in its segment, in pixel order (0 at ignored pixels).
    The reference has no such loss (upper_bound_chaos.py --do_loss_lovasz)."""
    if not (torch.is_tensor(input) and input.dtype == torch.float32 and input.dim() == 4):
        raise ValueError('input must be a 4-D float32 CUDA tensor (N,K,H,W)')
    N, K, H, W = input.shape
    if min(input.shape) < 1 or not LOVASZ_MIN_CLASSES <= K <= LOVASZ_MAX_CLASSES or input.numel() >= 2 ** 31:
        raise ValueError(f'input is {tuple(input.shape)}: need {LOVASZ_MIN_CLASSES} <= K <= {LOVASZ_MAX_CLASSES}, no empty axis, N*K*H*W < 2^31')
    if classes not in ('present', 'all'):
        raise ValueError(f"classes must be 'present' or 'all', got {classes!r}")
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not -2 ** 63 <= ignore_index < 2 ** 63):
        raise ValueError(f'ignore_index must be None or an integer, got {ignore_index!r}')
    for name, flag in (('per_image', per_image), ('return_parts', return_parts)):
        if not isinstance(flag, (bool, int)) or flag not in (0, 1):
            raise ValueError(f'{name} must be a bool, got {flag!r}')
    if not torch.is_tensor(target):
        raise ValueError(f'target must be a torch tensor, got {type(target).__name__}')
    if target.dim() == 4:
        if tuple(target.shape) != (N, K, H, W):
            raise ValueError(f'a one-hot target must have input\'s shape {(N, K, H, W)}, got {tuple(target.shape)}')
    elif target.dim() == 3:
        if target.dtype != torch.int64 or tuple(target.shape) != (N, H, W):
            raise ValueError(f'a class-map target must be int64 {(N, H, W)}, got {target.dtype} {tuple(target.shape)}')
    else:
        raise ValueError(f'target must be one-hot (N, K, H, W) or an int64 class map (N, H, W), got {tuple(target.shape)}')
    if not (target.is_cuda and target.device == input.device):
        raise ValueError('target must be a CUDA tensor on input\'s device')
    if not input.is_cuda:
        raise ValueError('input must be a CUDA tensor: there is no CPU path')
    with torch.no_grad():
        cls = (torch.argmax(target, dim=1) if target.dim() == 4 else target).contiguous()
    return _LovaszSoftmax.apply(input.contiguous(), cls, ignore_index, bool(per_image), classes == 'all', bool(return_parts))


class _RegLoss(torch.autograd.Function):
    """One regulariser of regop.REGULARISERS on its own: a RegOp over buffers of this call."""

    @staticmethod
    def forward(ctx, z, image, mask, reg, prm):
        N, K, H, W = z.shape
        st = stream_ptr()
        # [2:4] = the regulariser's pair: where pp_losses_finalize's ratio slot reads it
        sums = torch.zeros(4, device=z.device, dtype=torch.float64)
        op = RegOp.alloc(lib, reg, prm, sums[2:], sums, N, K, image.shape[1], H, W, ctx.needs_input_grad[0])
        op.fwd(z.data_ptr(), image.data_ptr(), mask.data_ptr() if mask is not None else None, N, K, image.shape[1], H, W,
               op.unit is not None, st)
        out = torch.empty((), device=z.device, dtype=torch.float32)
        op.finalize(out.data_ptr(), mask is not None, st)
        ctx.op, ctx.has_mask = op, mask is not None
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32).contiguous()
        dz = torch.zeros_like(ctx.op.unit)
        ctx.op.bwd(g.data_ptr(), ctx.has_mask, 1.0, dz.data_ptr(), dz.numel(), stream_ptr())
        return dz, None, None, None, None


def _reg_loss(name, input, image, valid_mask, **prm):
    z, x = _check(input, 'input'), _check(image, 'image')
    N, K, H, W = z.shape
    if x.shape[0] != N or tuple(x.shape[2:]) != (H, W):
        raise ValueError(f'image must be (N,C,H,W) with the N, H, W of input {tuple(z.shape)}, got {tuple(x.shape)}')
    m = None
    if valid_mask is not None:
        m = _check(valid_mask, 'valid_mask')
        if tuple(m.shape) != (N, 1, H, W):
            raise ValueError(f'valid_mask must be {(N, 1, H, W)}, got {tuple(m.shape)}')
    reg = REGULARISERS[name]
    return _RegLoss.apply(z, x, m, reg, reg.check(K=K, C=x.shape[1], **prm))


def gated_crf_loss(input, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1):
    """Local pairwise gated-CRF / Potts regulariser (this implementation's addition; the reference has no such loss):
    (1/D) sum_i sum_j m_i m_j k_ij (1 - <p_i, p_j>) with p = softmax(input), j = i + (dy, dx) * dilation over dy, dx in
    [-radius, radius] \\ (0, 0) inside the image, k_ij = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))
    on the `image` channels, D = N H W or max(sum(valid_mask), 1e-8).  Differentiable in `input` only."""
    return _reg_loss('crf', input, image, valid_mask, radius=radius, dilation=dilation, sigma_xy=sigma_xy, sigma_rgb=sigma_rgb)


def normalized_cut_loss(input, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1):
    """Normalised cut over the local bilateral window of gated_crf_loss (this implementation's addition; the reference has no such
    loss): (1/(N K)) sum_n sum_c (1 - A_nc / V_nc) with p = softmax(input), q_ic = sum_j m_j k_ij p_jc, d_i = sum_j m_j k_ij,
    A_nc = sum_i m_i p_ic q_ic, V_nc = sum_i m_i p_ic d_i; a class with V_nc <= 1e-6 in an image adds 0 and gets no gradient.
    Differentiable in `input` only."""
    return _reg_loss('nc', input, image, valid_mask, radius=radius, dilation=dilation, sigma_xy=sigma_xy, sigma_rgb=sigma_rgb)


def mumford_shah_loss(input, image, valid_mask=None, tv_weight=1.0):
    """Mumford-Shah level-set loss with an anisotropic total-variation term (this implementation's addition; the reference has no
    such loss): (1/D) (sum_nci m_i p_ic |x_i - mu_nc|^2 + tv_weight sum_nc sum_(i,j) m_i m_j |p_ic - p_jc|) with p = softmax(input),
    mu_nc the m p-weighted mean of the `image` channels over image n (a class with sum_i m_i p_ic <= 1e-6 in an image adds no
    level-set term), (i, j) the vertical and horizontal neighbour pairs, D = N H W or max(sum(valid_mask), 1e-8).  Differentiable
    in `input` only."""
    return _reg_loss('ms', input, image, valid_mask, tv_weight=tv_weight)


class _WeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        import ctypes
        n = len(terms)
        for t in terms:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                raise TypeError('weighted_loss_sum: every term must be a one-element float32 CUDA tensor')
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in terms])
        w = (ctypes.c_float * n)(*[float(x) for x in weights])
        out = torch.empty((), device=terms[0].device, dtype=torch.float32)
        lib.pp_weighted_sum_fwd(ptrs, w, n, out.data_ptr(), stream_ptr())
        ctx.w, ctx.n = w, n
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32).contiguous()
        gout = torch.empty(ctx.n, device=g.device, dtype=torch.float32)
        lib.pp_weighted_sum_bwd(g.data_ptr(), ctx.w, ctx.n, gout.data_ptr(), stream_ptr())
        return (None,) + tuple(gout[i] for i in range(ctx.n))


def weighted_loss_sum(terms, weights):
    """total = terms[0] * weights[0] + terms[1] * weights[1] + ... -- the loss assembly of the training loop
    (train_chaos.py:273-310) as ONE launch forward and ONE backward instead of a chain of element-wise launches on 0-dim
    tensors.  Same arithmetic as that chain (fp32 products and sums, left to right): bit-identical totals and gradients.
    terms: 0-dim float32 CUDA tensors (at most 8); weights: Python floats."""
    terms = list(terms)
    if len(terms) != len(weights) or not 1 <= len(terms) <= 8:
        raise ValueError('weighted_loss_sum: 1..8 terms, one weight each')
    return _WeightedSum.apply(tuple(float(w) for w in weights), *terms)

