"""Float64 torch references of the three consistency forms behind cr_variant 5 - 7 of pp_seg_losses_fwd / _bwd (bikl_loss, js_loss,
hard_ce_loss), differentiated by autograd.  Nothing here is device-specific: the functions run wherever their arguments live.

`bidirectional_kl_loss` is pinned to the reference's own function (losses/losses.py:118-145) by tests/golden/cr_bikl.npz
(tests/test_cr_variants.py).  `js_loss` and `hard_label_cross_entropy_loss` have no counterpart in the reference: they are UNPINNED,
their definitions are the ones written here, and the finite-difference test of tests/test_cr_variants.py checks their gradients.

Signatures as in the reference's functional API: (input, target, valid_mask=None) with `input` = strong logits, `target` = weak
logits, both (N, K, H, W); valid_mask (N, 1, H, W) or None.
"""
import math

import torch


def _masked_mean(per_elem, valid_mask):
    """The reduction of losses/losses.py: sum(loss * mask) / max(mask.sum(), 1e-8), or the mean over every element."""
    if valid_mask is not None:
        return (per_elem * valid_mask).sum() / valid_mask.sum().clamp_min(1e-8)
    return per_elem.mean()


def bidirectional_kl_loss(input, target, valid_mask=None):
    """(KL(q || s) + KL(s || q)) / 2 element-wise over (N, K, H, W), q = softmax(target), s = softmax(input)."""
    ls, lq = torch.log_softmax(input, 1), torch.log_softmax(target, 1)
    p_loss = lq.exp() * (lq - ls)
    q_loss = ls.exp() * (ls - lq)
    return (_masked_mean(p_loss, valid_mask) + _masked_mean(q_loss, valid_mask)) / 2


def js_loss(input, target, valid_mask=None):
    """Jensen-Shannon divergence per pixel, (KL(q || m) + KL(s || m)) / 2 with m = (q + s) / 2, channels summed first: (N, 1, H, W)."""
    ls, lq = torch.log_softmax(input, 1), torch.log_softmax(target, 1)
    lm = torch.logaddexp(ls, lq) - math.log(2.0)
    per_pixel = 0.5 * ((lq.exp() * (lq - lm)).sum(1, keepdim=True) + (ls.exp() * (ls - lm)).sum(1, keepdim=True))
    return _masked_mean(per_pixel, valid_mask)


def hard_label_cross_entropy_loss(input, target, valid_mask=None):
    """-log softmax(input)[argmax_k target] per pixel (torch.argmax: the first maximum), (N, 1, H, W); `target` is a constant."""
    c = target.detach().argmax(1, keepdim=True)
    per_pixel = -torch.log_softmax(input, 1).gather(1, c)
    return _masked_mean(per_pixel, valid_mask)


BY_NAME = {'bikl_loss': bidirectional_kl_loss, 'js_loss': js_loss, 'hard_ce_loss': hard_label_cross_entropy_loss}
CODE = {'bikl_loss': 5, 'js_loss': 6, 'hard_ce_loss': 7}


def consistency(name, strong_logits, weak_logits, valid_mask=None, detach_weak=False):
    """The consistency term as the model forms it: --detach_weak_cr makes the weak view a constant target."""
    return BY_NAME[name](strong_logits, weak_logits.detach() if detach_weak else weak_logits, valid_mask)
