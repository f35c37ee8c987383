"""Which 3x3-convolution kernel family a layer runs on, and the one object per layer and plan that calls it.

`select` decides once per (layer, shape, storage); `ConvOp` turns "this operation, these operands" into the one C-ABI call of that
family.  Streams, events and the choice of workspace stay in the engine; everything BatchNorm / GroupNorm is normop.py's.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

from ._lib import PpPackItem, PpWinoPackItem, lib


class ConvSel(NamedTuple):
    """Kernel family of one conv layer at one shape."""
    kind: str       # 'wino': Winograd, 'f16x3': split-fp16 direct kernels, 'fp32': fp32 direct kernels
    tile: int       # Winograd output tile: 4 = F(4x4,3x3), 2 = F(2x2,3x3); 0 for the direct kinds
    split: bool     # the Winograd GEMMs (forward, data and weight gradient alike) run on pre-split fp16 operands


def select(L, h, w, h16) -> ConvSel:
    """Kernel family of conv layer L at (h, w) -- a pure function of the shape, the storage (h16: 16-bit activations) and the
    engine's switches, which are read when a plan is built (scripts and tests flip them on `engine`)."""
    from . import engine as E
    # Winograd F(4x4,3x3) / F(2x2,3x3) for the wide layers: 4x / 2.25x less MFMA work (measured 1.3-3.2x per
    # layer from 128 input channels up, scripts/bench_wino.py); narrow high-resolution layers stay direct
    use = (E.WINO_ENABLED and L.cin >= E.WINO_MIN_CIN and L.cout >= E.WINO_MIN_COUT and L.cin == L.cin_pad
           and h % (2 * L.dil) == 0 and w % (2 * L.dil) == 0 and L.stride == 1)
    tile = lib.pp_conv3x3_wino_tile(h, w, L.dil) if use else 0
    # split-fp16 GEMMs on pre-split operands (octets along the GEMM K: 8 channels); forward and weight gradient
    # share the kept transformed input, so they take the same path
    split = bool(use and E.F16X3_ENABLED and tile == 4 and L.cin % 8 == 0 and L.cout % 8 == 0)
    if h16 and use and not split:      # 16-bit storage has the split-fp16 F(4x4,3x3) Winograd path only
        use, tile = False, 0
    if use:
        return ConvSel('wino', tile, split)
    f16 = bool(E.F16X3_ENABLED and L.cin_pad == L.cin and L.cin % 4 == 0 and L.cout % 4 == 0 and L.cout >= E.F16X3_MIN_COUT)
    if h16 and not f16 and L.cin_pad == L.cin:
        raise NotImplementedError(f'16-bit storage: {L.name} ({L.cin}->{L.cout}) has no split-fp16 kernel '
                                  f'(needs >= {E.F16X3_MIN_COUT} output channels)')
    return ConvSel('f16x3' if f16 else 'fp32', 0, False)


class ConvOp:
    """One conv layer of one plan, bound to its kernel family.  K: the plan's entry-point table; wf / wb: packed forward / data-
    gradient weights (wb None: no data gradient, the first layer); vkeep: transformed input kept for the Winograd weight gradient
    (None in forward-only plans); amax: max |dz| of the step for the split-fp16 gradient kernels (None where nothing reads it).
    woff / boff: byte offsets added to the addresses of the layer's weight / bias wherever they are read -- 0: the live parameters;
    a teacher plan: the distance from the parameter slab to the optimizer's shadow slab (forward-only: the gradient calls ignore them).
    `ws` arguments are (pointer, bytes) of the workspace of the stream `st`."""
    __slots__ = ('sel', 'conv', 'cin', 'cin_pad', 'cout', 'dil', 'K', 'slope', 'wf', 'wb', 'vkeep', 'amax', 'woff', 'boff')

    def __init__(self, sel: ConvSel, L, K, slope, wf, wb, vkeep, amax, woff=0, boff=0):
        self.sel, self.conv, self.K, self.slope = sel, L.conv, K, slope
        self.woff, self.boff = woff, boff
        self.cin, self.cin_pad, self.cout, self.dil = L.cin, L.cin_pad, L.cout, L.dil
        self.wf, self.wb, self.vkeep, self.amax = wf, wb, vkeep, amax

    def _pack_args(self):
        return (self.conv.weight.data_ptr() + self.woff, self.cout, self.cin, self.sel.tile if self.sel.kind == 'wino' else self.cin_pad,
                self.wf.data_ptr(), self.wb.data_ptr() if self.wb is not None else None)

    def pack_item(self):
        """This layer's entry of the batched weight packs (one launch per family), or None: the layer packs on its own."""
        w, cout, cin, pad, wf, wb = self._pack_args()
        if self.sel.kind == 'wino':
            return PpWinoPackItem(w, cout, cin, wf, wb) if self.sel.split else None
        return PpPackItem(w, cout, cin, pad, wf, wb) if self.sel.kind == 'f16x3' else None

    def pack(self, st):
        """Kernel-side weight layouts of this layer: split-fp16 operands, Winograd-domain U."""
        K = self.K
        if self.sel.kind == 'wino':
            fn = K.pp_wino_pack_weights_f16x3 if self.sel.split else K.pp_wino_pack_weights
        else:
            fn = K.pp_pack_conv3x3_weights_f16x3 if self.sel.kind == 'f16x3' else K.pp_pack_conv3x3_weights
        fn(*self._pack_args(), st)

    def _fwd_args(self, x, out_ptr, ld_out):
        return (x.ptr, x.ld, x.C, self.wf.data_ptr(), self.conv.bias.data_ptr() + self.boff, out_ptr, ld_out, self.cout,
                x.N, x.H, x.W, self.dil)

    def fwd(self, x, out_ptr, ld_out, ws, st):
        """Plain convolution z = conv(x) + bias (stride-2 layers, GroupNorm blocks, the unfused BatchNorm path)."""
        assert not x.lazy, 'the plain convolution has no lazy-input form'
        a = self._fwd_args(x, out_ptr, ld_out)
        if self.sel.kind == 'wino':
            fn = self.K.pp_conv3x3_wino_fwd_f16x3 if self.sel.split else self.K.pp_conv3x3_wino_fwd
            fn(*a, 0, self.vkeep.data_ptr() if self.vkeep is not None else None, *ws, st)
        elif self.sel.kind == 'f16x3':
            self.K.pp_conv3x3_fwd_f16x3(*a, 0, None, st)
        else:
            self.K.pp_conv3x3_fwd(*a, 0, st)

    def fwd_bn(self, x, out_ptr, ld_out, groups, mode, scale, shift, stats, ws, rows, st):
        """Convolution with the BatchNorm side fused into its epilogue; mode 1: z + per-block statistics rows in `stats`
        ((pointer, bytes); their number per group lands in `rows` and is returned), mode 2: y = lrelu(z * scale + shift).
        A lazy x is normalised + activated while it is loaded."""
        a = self._fwd_args(x, out_ptr, ld_out)
        b = (mode, scale, shift, self.slope, groups, *stats, ctypes.byref(rows))
        lz = x.lazy_arg()
        if self.sel.kind == 'wino':
            assert lz is None, 'the Winograd path has no lazy-input form'
            self.K.pp_conv3x3_wino_fwd_bn(*a, 1 if self.sel.split else 0, self.vkeep.data_ptr() if self.vkeep is not None else None,
                                          *ws, *b, st)
        elif lz is not None:            # (a shape without a lazy form fails inside: plan.lazy_out asked pp_conv3x3_lazy_ok)
            self.K.pp_conv3x3_fwd_bn_lazy(*a, 1 if self.sel.kind == 'f16x3' else 0, None, *b, ctypes.byref(lz), st)
        else:
            self.K.pp_conv3x3_fwd_bn(*a, 1 if self.sel.kind == 'f16x3' else 0, None, *b, st)
        return rows.value

    def bwd_data(self, dz, x, dx, accumulate, ws, st):
        """dx (+)= data gradient of the output gradient at dz (dense, cout columns); x: the forward's input view (its shape)."""
        a = (dz, self.cout, self.cout, self.wb.data_ptr(), dx.ptr, dx.ld, self.cin, x.N, x.H, x.W, self.dil, 1 if accumulate else 0)
        if self.sel.kind == 'wino':
            if self.sel.split:
                self.K.pp_conv3x3_wino_bwd_data_f16x3(*a, *ws, self.amax.data_ptr(), st)
            else:
                self.K.pp_conv3x3_wino_bwd_data(*a, *ws, st)
        elif self.sel.kind == 'f16x3':
            self.K.pp_conv3x3_bwd_data_f16x3(*a, self.amax.data_ptr(), st)
        else:
            self.K.pp_conv3x3_bwd_data(*a, st)

    def bwd_weight(self, dz, x, gw, ws, lazy, st):
        """gw = weight gradient from dz and the forward's input x.  lazy: the pp_lazy_in of an x that holds the raw output of
        the layer in front (normalised + activated while it is staged; split-fp16 direct kernels only), else None."""
        C = self.cout
        if self.sel.kind == 'wino':         # (reads the kept V, made from final values: never lazy)
            a = (dz, C, C, x.ptr, x.ld, self.cin, x.N, x.H, x.W, self.dil, gw, 0, self.vkeep.data_ptr(), *ws)
            if self.sel.split:
                self.K.pp_conv3x3_wino_bwd_weight_f16x3(*a, self.amax.data_ptr(), st)
            else:
                self.K.pp_conv3x3_wino_bwd_weight(*a, st)
            return
        a = (dz, C, C, x.ptr, x.ld, self.cin_pad, self.cin, x.N, x.H, x.W, self.dil, gw, 0, *ws)
        if self.sel.kind == 'fp32':
            self.K.pp_conv3x3_bwd_weight(*a, st)
        elif lazy is not None:
            self.K.pp_conv3x3_bwd_weight_f16x3_lazy(*a, self.amax.data_ptr(), ctypes.byref(lazy), st)
        else:               # split-fp16 halo kernel where the shape qualifies, the fp32 kernels otherwise
            self.K.pp_conv3x3_bwd_weight_f16x3(*a, self.amax.data_ptr(), st)
