"""The image-pairwise regularisers on the weak logits -- gated CRF, normalised cut, Mumford-Shah -- declared once, and the one object
per regulariser and set of buffers that makes its launches.

`REGULARISERS` is the ordered table of what exists.  Its order, and nothing else, decides where a regulariser's pair sits in a plan's
sums block, where its key sits in the step's outputs, the order of its forward / backward launches (the fp32 adds onto dlogits), of
its term in the assembled loss (the left-to-right sum of pp_weighted_sum_fwd) and of its column in the epoch's meter.  `RegOp` binds
one entry to its buffers -- a plan's (engine.py) or those of one stand-alone call (losses/losses.py) -- and, like convop.py / normop.py,
launches through the entry-point table K it was given, looked up at call time.
"""
from __future__ import annotations

import math

import torch

CRF_MAX_RADIUS, CRF_MAX_DILATION, CRF_MAX_HALO, CRF_MAX_CHANNELS, CRF_MAX_CLASSES = 8, 4, 16, 4, 32
MS_MAX_CHANNELS, MS_MAX_CLASSES = 4, 32


def _check_window(label, radius, dilation, sigma_xy, sigma_rgb, K, C) -> dict:
    """The local bilateral window the gated-CRF and normalised-cut kernels walk; `label` names the loss in the messages."""
    if int(radius) != radius or int(dilation) != dilation:
        raise ValueError(f'{label}: radius and dilation must be integers (got {radius!r}, {dilation!r})')
    radius, dilation, sigma_xy, sigma_rgb = int(radius), int(dilation), float(sigma_xy), float(sigma_rgb)
    if radius < 1 or dilation < 1:
        raise ValueError(f'{label}: radius and dilation must be >= 1 (got {radius}, {dilation})')
    for name, v in (('sigma_xy', sigma_xy), ('sigma_rgb', sigma_rgb)):
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f'{label}: {name} must be a positive finite number (got {v!r})')
    if radius > CRF_MAX_RADIUS or dilation > CRF_MAX_DILATION or radius * dilation > CRF_MAX_HALO:
        raise NotImplementedError(f'{label}: radius <= {CRF_MAX_RADIUS}, dilation <= {CRF_MAX_DILATION} and radius * dilation <= '
                                  f'{CRF_MAX_HALO} (got {radius}, {dilation})')
    if K is not None and not 1 <= K <= CRF_MAX_CLASSES:
        raise NotImplementedError(f'{label}: 1 .. {CRF_MAX_CLASSES} classes (got {K})')
    if C is not None and not 1 <= C <= CRF_MAX_CHANNELS:
        raise NotImplementedError(f'{label}: 1 .. {CRF_MAX_CHANNELS} image channels (got {C})')
    return dict(radius=radius, dilation=dilation, sigma_xy=sigma_xy, sigma_rgb=sigma_rgb)


def check_crf_params(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, K=None, C=None) -> dict:
    """The accepted ranges of the gated-CRF loss (include/pacingpseudo_hip.h: pp_crf_loss_fwd), checked before any launch:
    ValueError for values that are no neighbourhood / no kernel width at all, NotImplementedError for sizes beyond what the
    kernel stages in LDS.  Returns the normalised parameters."""
    return _check_window('gated CRF', radius, dilation, sigma_xy, sigma_rgb, K, C)


def check_nc_params(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, K=None, C=None) -> dict:
    """The accepted ranges of the normalised-cut loss (include/pacingpseudo_hip.h: pp_nc_loss_fwd) -- those of check_crf_params: the
    two losses walk the same window -- checked before any launch.  Returns the normalised parameters."""
    return _check_window('normalised cut', radius, dilation, sigma_xy, sigma_rgb, K, C)


def check_ms_params(tv_weight=1.0, K=None, C=None) -> dict:
    """The accepted ranges of the Mumford-Shah level-set loss (include/pacingpseudo_hip.h: pp_ms_loss_fwd), checked before any
    launch: ValueError for a total-variation weight that is negative or not finite, NotImplementedError for more classes or image
    channels than the kernels take.  Returns the normalised parameters."""
    try:
        tv_weight = float(tv_weight)
    except (TypeError, ValueError):
        raise ValueError(f'Mumford-Shah: tv_weight must be a number (got {tv_weight!r})') from None
    if not (tv_weight >= 0.0 and math.isfinite(tv_weight)):
        raise ValueError(f'Mumford-Shah: tv_weight must be >= 0 and finite (got {tv_weight!r})')
    if K is not None and not 1 <= K <= MS_MAX_CLASSES:
        raise NotImplementedError(f'Mumford-Shah: 1 .. {MS_MAX_CLASSES} classes (got {K})')
    if C is not None and not 1 <= C <= MS_MAX_CHANNELS:
        raise NotImplementedError(f'Mumford-Shah: 1 .. {MS_MAX_CHANNELS} image channels (got {C})')
    return dict(tv_weight=tv_weight)


class Regulariser:
    """One row of the table.  name: everything else follows from it -- the flag do_loss_<name>, the output key loss_<name>, the weight
    loss_<name>_weight, the ramp flag ramp_up_loss_<name>, the run's parameters <name>_<parameter> and the entry points
    pp_<name>_loss_workspace / _fwd / _bwd.  params: {parameter: default}, in the order the forward entry point takes them and
    `check` returns them.  masked: the ratio's denominator is max(sum(valid_mask), 1e-8) when the batch has a mask, and finalize /
    backward are told so; else the pair is (sum, count) whatever the mask.  ws_dims: what the workspace query takes, of B K C H W.
    state_cols: last dimension, from the image channels, of the (B, K, .) float64 buffer the forward leaves its per-class statistics
    in; None: no such buffer."""
    __slots__ = ('name', 'params', 'check', 'masked', 'ws_dims', 'state_cols', 'flag', 'key', 'weight', 'ramp')

    def __init__(self, name, params, check, masked, ws_dims, state_cols=None):
        self.name, self.params, self.check, self.masked, self.ws_dims, self.state_cols = name, params, check, masked, ws_dims, state_cols
        self.flag, self.key, self.weight, self.ramp = f'do_loss_{name}', f'loss_{name}', f'loss_{name}_weight', f'ramp_up_loss_{name}'

    def args_params(self, args) -> dict:
        """The run's parameters, unchecked: <name>_<parameter> of the namespace, the default where it lacks the attribute."""
        return {p: getattr(args, f'{self.name}_{p}', d) for p, d in self.params.items()}


_WINDOW = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
REGULARISERS = {r.name: r for r in (
    Regulariser('crf', _WINDOW, check_crf_params, masked=True, ws_dims='BHW'),
    Regulariser('nc', _WINDOW, check_nc_params, masked=False, ws_dims='BKHW', state_cols=lambda C: 2),           # assoc, vol
    Regulariser('ms', dict(tv_weight=1.0), check_ms_params, masked=True, ws_dims='BKCHW', state_cols=lambda C: 1 + C),      # S, mu
)}


def active_regularisers(args):
    """The table's rows whose flag is on in `args` (a namespace that lacks the attribute: off), in table order."""
    return [r for r in REGULARISERS.values() if getattr(args, r.flag, False)]


class RegOp:
    """One regulariser bound to one set of buffers.  prm: its parameters as its checker returned them; sums: its (numerator,
    denominator) pair, float64; fin: the view that starts two doubles earlier -- pp_losses_finalize's ratio slot reads [2] / [3];
    ws / ws_bytes: its workspace; unit: the unit gradient the forward leaves for the backward, None in a forward-only binding;
    state: see Regulariser.state_cols.  Pointer arguments of the methods are device addresses, None for a null pointer."""
    __slots__ = ('K', 'reg', 'prm', 'sums', 'fin', 'ws', 'ws_bytes', 'unit', 'state')

    def __init__(self, K, reg, prm, sums, fin, ws, ws_bytes, unit, state):
        self.K, self.reg, self.prm, self.sums, self.fin = K, reg, prm, sums, fin
        self.ws, self.ws_bytes, self.unit, self.state = ws, ws_bytes, unit, state

    @classmethod
    def alloc(cls, K, reg, prm, sums, fin, B, Kc, C, H, W, trainable):
        """Workspace, unit gradient (trainable only) and state for B images of Kc classes and C channels at H x W, around the
        caller's sums / fin."""
        dev = sums.device
        dims = dict(B=B, K=Kc, C=C, H=H, W=W)
        nws = getattr(K, f'pp_{reg.name}_loss_workspace')(*(dims[d] for d in reg.ws_dims))
        return cls(K, reg, prm, sums, fin, torch.empty(nws, device=dev, dtype=torch.uint8), nws,
                   torch.empty((B, Kc, H, W), device=dev, dtype=torch.float32) if trainable else None,
                   torch.zeros((B, Kc, reg.state_cols(C)), device=dev, dtype=torch.float64) if reg.state_cols else None)

    def fwd(self, logits, image, mask, N, K, C, H, W, need_grad, st):
        """The pair into `sums` (and, need_grad, the unit gradient) from the (N,K,H,W) logits, the (N,C,H,W) image and the
        (N,1,H,W) mask or None."""
        state = (self.state.data_ptr(),) if self.state is not None else ()
        getattr(self.K, f'pp_{self.reg.name}_loss_fwd')(logits, image, mask, N, K, C, H, W, *self.prm.values(),
                                                        self.unit.data_ptr() if need_grad else None, *state, self.sums.data_ptr(),
                                                        self.ws.data_ptr(), self.ws_bytes, st)

    def finalize(self, out, has_mask, st):
        """out = sums[0] / sums[1], the sums as they stand (all-reduced over the ranks by then); a masked ratio with a mask:
        / max(sums[1], 1e-8)."""
        self.K.pp_losses_finalize(self.fin.data_ptr(), 1 if (has_mask and self.reg.masked) else 0, None, out, None, st)

    def bwd(self, g_up, has_mask, grad_scale, dlogits, n, st):
        """dlogits[:n] += grad_scale * g_up * d loss / d logits: a streaming add of the unit gradient the forward left, behind the
        kernel that WRITES dlogits."""
        mask = (1 if has_mask else 0,) if self.reg.masked else ()
        getattr(self.K, f'pp_{self.reg.name}_loss_bwd')(self.unit.data_ptr(), self.sums.data_ptr(), *mask, g_up, grad_scale, dlogits, n, st)
