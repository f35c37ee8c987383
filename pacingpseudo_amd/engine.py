"""StepEngine: the static execution plan of one PacingPseudo iteration on one MI355X.

The reference runs its step through PyTorch's dynamic autograd graph, one `aten` op at a time
(train_chaos.py:263-315 -> models/consistency_reglur_memory.py:24-102 -> models/unet.py:62-98).  The network is
fixed, so here the whole step is a *static plan*: every activation, gradient and workspace buffer is laid out once
per input shape in HBM (NHWC, the weak and the strong view back to back along the batch axis), the forward and
the hand-derived backward are fixed sequences of C-ABI kernel launches on the current HIP stream, and weight
gradients land directly in one flat slab that the fused Adam kernel (and the RCCL all-reduce) consume.

Layout decisions
  * activations NHWC fp32; `torch.cat((up(x), skip), 1)` (models/unet.py:151) never runs: producers write
    straight into channel slices of pre-allocated concatenation buffers (pixel stride = lower+skip channels),
    and the matching gradient buffers are filled by the consumers' data-gradient kernels with an
    accumulate flag, so multi-consumer tensors need no separate add.
  * the weak and strong passes of the siamese step (consistency_reglur_memory.py:29,48) share every launch:
    batch = [weak | strong]; BatchNorm statistics / running-stat updates are per group and in order, exactly
    as two module calls would produce; weight gradients of both passes fall out of ONE wgrad reduction.
  * cat5 = [stage6 | stage5] is also the auxiliary path's input (aux_path_memory.py:49), so that concat is
    shared as well.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from ._lib import PpBnCoefItem, PpLazyIn, PpPackItem, PpWinoPackItem, lib, lib_for, prof_range, stream_ptr
from .convop import ConvOp, select as conv_select
from .normop import NormOp
from .regop import REGULARISERS, RegOp, active_regularisers
from .losses.losses import _VARIANT

WINO_ENABLED = os.environ.get('PP_WINO', '1') != '0'      # A/B switch for the Winograd path
# split-fp16 ("f16x3") direct convolution for the non-Winograd layers with at least this many output channels
# (scripts/bench_conv.py --f16x3: 1.05-1.9x the fp32 kernels from 64 outputs up, about equal on the 32-output 256x256
# layers in isolation; on the whole step 32 beats 64 by 0.8 ms, r01 sweep)
F16X3_ENABLED = os.environ.get('PP_F16X3', '1') != '0'
F16X3_MIN_COUT = 32
# BatchNorm fused into the convolution epilogues (train: batch statistics emitted by the conv kernel; eval: scale /
# shift / LeakyReLU applied in the epilogue, one-pass backward from y).  PP_FUSE_BN=0 runs the separate kernels (A/B).
FUSE_BN = os.environ.get('PP_FUSE_BN', '1') != '0'
# train-mode BatchNorm + LeakyReLU applied by the CONSUMER of a tensor while it loads (no bn_lrelu_fwd pass, y never stored);
# PP_LAZY_BN=0 restores the separate apply pass (A/B, same results up to the order of one multiply-add)
LAZY_BN = os.environ.get('PP_LAZY_BN', '1') != '0'
# gradient of nn.MaxPool2d folded into the BatchNorm backward of the layer in front of it (pp_bn_lrelu_bwd[_eval]_pool): no
# separate pp_maxpool2_bwd pass over the skip-gradient buffer.  PP_FUSE_POOL_BWD=0: the separate pass (A/B, same results).
FUSE_POOL_BWD = os.environ.get('PP_FUSE_POOL_BWD', '1') != '0'
# ... and the forward max-pooling folded into the BatchNorm apply pass in front of it (pp_bn_lrelu_fwd_pool, train mode)
FUSE_POOL_FWD = os.environ.get('PP_FUSE_POOL_FWD', '1') != '0'
# weight gradients on a SECOND HIP stream: wgrad(L) needs only dz(L) and x(L) and nothing downstream needs it before the
# optimizer, so it runs beside the critical chain dgrad(L) -> BatchNorm backward(L-1) -> ... (two dz buffers in turn, its own
# workspace; the main stream waits for it at bucket boundaries and at the end of the backward pass).  PP_WGRAD_STREAM=0: one stream.
WGRAD_STREAM = os.environ.get('PP_WGRAD_STREAM', '1') != '0'
# CU budget of the persistent direct weight-gradient kernels while they run on that stream (pp_set_wgrad_cus): with the whole chip
# (256) their first blocks occupy every CU and the data-gradient / BatchNorm chain on the main stream queues behind them; 192 leaves
# it room.  Same-box sweep (r05, profiles/r05_experiments/wgrad_cu_budget_sweep.log): 256 -> 32.43 ms, 224 -> 31.88, 192 -> 31.71,
# 160 -> 32.0, 128 -> 32.09, 96 -> 32.7 (one stream: 32.52).  A budget for the Winograd weight-gradient GEMM (PP_WINO_WGRAD_CUS)
# only lost; the stream's HIP priority has no effect (the device offers two levels and the default is the lower one).
# the auxiliary path's forward (bottleneck conv + BN, classifier, its partial CE, the memory-bank update: ~0.4 ms of small,
# latency-bound launches) on the second stream beside the decoder's forward pass, which does not depend on it
AUX_SIDE = os.environ.get('PP_AUX_SIDE', '1') != '0'
# weight gradient of the FIRST convolution (one input channel, no data gradient wanted) folded into the BatchNorm backward that
# forms its dz (pp_bn_lrelu_bwd[_eval]_wgrad_c1): dz is not written and the conv3x3_c4_wgrad launch -- the last kernel of every
# backward pass, alone on the chip -- does not run.  PP_FUSE_WG1=0: the separate launches (A/B).
FUSE_WG1 = os.environ.get('PP_FUSE_WG1', '1') != '0'
# the per-layer weight packs of a step as one launch per family (pp_*_pack_weights_f16x3_batch); False: one launch per layer
PACK_BATCH = True      # (module attribute, no environment switch: tests flip it to compare with the per-layer calls)
COEF_BATCH = True       # eval-mode BatchNorm coefficient rows of the whole backbone in one launch (module attribute: tests compare both)
WGRAD_CUS_SIDE = int(os.environ.get('PP_WGRAD_CUS_SIDE', '192'))
WGRAD_CUS_FULL = 256                                               # the budget without a second stream: the whole chip
# (Round 4 also built on-load BatchNorm for the Winograd input transform, bilinear x2 up-sampling and max-pooling, and moved the
# data-gradient weight packs to the second stream; all four measured slower or neutral on the benchmark step -- DESIGN.md section 3
# "Round 4", profiles/r04_experiments/ -- and were removed in round 5: kernels, entry points, engine branches and tests.)
# On-load BatchNorm in the patch staging of the two-half halo kernel + the halo-tile weight-gradient kernels, for the MID tensor of a
# DoubleConv (conv -> conv, one consumer): ON.  The P phase of that kernel spends most of its time waiting for memory (r04
# phase trace), so the three VALU operations per element ride along and the mid tensor's bn_lrelu_fwd pass disappears
# (four layers of the benchmark network: enc1 / enc2 / dec2 / dec1).  PP_LAZY_HALO=0 restores the separate pass (A/B).
LAZY_HALO = os.environ.get('PP_LAZY_HALO', '1') != '0'
LAZY_HALO_H16 = False      # the same in 16-bit storage plans: measured a wash (r04 A/B: BatchNorm -0.23 ms, halo +0.20, weight gradients +0.10)
WINO_MIN_CIN = int(os.environ.get('PP_WINO_MIN_CIN', '256'))   # tuning knobs (scripts/bench_wino.py)
WINO_MIN_COUT = 64
SLOPE = 1e-2
BN_EPS = 1e-5
BN_MOM = 0.1
CR_VARIANTS = _VARIANT      # --loss_cr_variants name -> cr_variant code of pp_seg_losses_*: the functional API's table, one object

class View:
    """NHWC view: element (n,y,x,c) lives at ptr + es*(((n*H+y)*W+x)*ld + c), es = bytes per element (4: fp32, 2: the fp16
    tensors of a 16-bit-storage plan).  `base`/`n0`/`c0` remember the
    owning torch tensor and the slice, so tests and debuggers can look at the same memory through torch.

    LAZY tensors (round 4; pp_lazy_in in include/pacingpseudo_hip.h): a buffer that can hold a train-mode BatchNorm layer's
    raw convolution output z instead of y = LeakyReLU(BN(z)) owns coefficient rows `coef` ([groups][3][ld]: scale, shift,
    slope; identity rows for channels with final values) and a flag shared by all its views, set by the forward while the
    buffer is lazy.  Consumers with a *_lazy kernel form read y on the fly (`lazy_arg`)."""
    __slots__ = ('ptr', 'ld', 'C', 'N', 'H', 'W', 'base', 'n0', 'c0', 'coef', 'cptr', 'cg', 'flag', 'es')

    def __init__(self, ptr, ld, C, N, H, W, base=None, n0=0, c0=0, coef=None, cptr=0, cg=1, flag=None, es=4):
        self.ptr, self.ld, self.C, self.N, self.H, self.W = ptr, ld, C, N, H, W
        self.base, self.n0, self.c0 = base, n0, c0
        self.coef, self.cptr, self.cg, self.flag = coef, cptr, cg, flag
        self.es = es

    @property
    def storage(self) -> str:
        """'fp32' / 'fp16' / 'bf16': how the elements of this view are stored (the owning tensor's dtype)."""
        if self.es == 4:
            return 'fp32'
        return 'bf16' if (self.base is not None and self.base.dtype == torch.bfloat16) else 'fp16'

    @property
    def dtype(self):
        return {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}[self.storage]

    def torch(self) -> torch.Tensor:
        """(N,H,W,C) strided torch view of this memory (RAW contents: z where the buffer is lazy, see values())."""
        return self.base[self.n0:self.n0 + self.N, :, :, self.c0:self.c0 + self.C]

    @property
    def lazy(self) -> bool:
        return self.flag is not None and self.flag[0]

    def lazy_arg(self):
        """ctypes pp_lazy_in of this view, or None when it holds final values."""
        if not self.lazy:
            return None
        return PpLazyIn(self.cptr, self.ld, self.cg)

    def coef_rows(self) -> torch.Tensor:
        """(groups, 3, C) coefficient rows of this view's channels (a torch view of the owning buffer's rows)."""
        g0 = (self.cptr - self.coef.data_ptr()) // 4 // (3 * self.ld)
        return self.coef[g0:g0 + self.cg, :, self.c0:self.c0 + self.C]

    def values(self) -> torch.Tensor:
        """(N,H,W,C) LOGICAL values: y = lrelu(z * scale + shift) where the buffer is lazy (a test / debugging aid; the
        product path never calls it)."""
        t = self.torch()
        if not self.lazy:
            return t
        out = torch.empty((self.N, self.H, self.W, self.C), device=t.device, dtype=t.dtype)
        lz = self.lazy_arg()
        lib_for(self.storage).pp_lazy_materialize(self.ptr, self.ld, ctypes.byref(lz), out.data_ptr(), self.C, self.C, self.N, self.H * self.W, stream_ptr())
        return out


def _pad4(c):
    return (c + 3) // 4 * 4


def _sub(v: View, c0: int, c: int) -> View:
    """Channel slice [c0, c0+c) of a view."""
    return View(v.ptr + v.es * c0, v.ld, c, v.N, v.H, v.W, v.base, v.n0, v.c0 + c0,
                v.coef, v.cptr + 4 * c0 if v.coef is not None else 0, v.cg, v.flag, v.es)


def _batch(v: View, n0: int, n: int) -> View:
    """Sample range [n0, n0+n) of a view (whole statistics groups when the view can be lazy)."""
    cptr, cg = v.cptr, v.cg
    if v.coef is not None and v.cg > 1:
        per = v.N // v.cg
        assert n0 % per == 0 and n % per == 0, 'a batch slice of a lazy buffer must cover whole statistics groups'
        cptr, cg = v.cptr + 4 * (n0 // per) * 3 * v.ld, n // per
    return View(v.ptr + v.es * n0 * v.H * v.W * v.ld, v.ld, v.C, n, v.H, v.W, v.base, v.n0 + n0, v.c0, v.coef, cptr, cg, v.flag, v.es)


class _Layer:
    """Runtime record of one conv3x3 + BN + LeakyReLU layer."""

    def __init__(self, name, conv, bn, dil):
        self.name, self.conv, self.bn, self.dil = name, conv, bn, dil
        # nn.GroupNorm holder (--norm_op group): per-(image, channel group) statistics in both modes, no running state
        self.gn = isinstance(bn, nn.GroupNorm)
        self.stride = int(conv.stride[0])     # 2: first convolution of a down-sampling stage under --is_stride_conv (unet.py:113-116)
        self.cout, self.cin = conv.weight.shape[0], conv.weight.shape[1]
        self.cin_pad = _pad4(self.cin)
        # per-plan state (set by _Plan)
        self.x: Optional[View] = None
        self.y: Optional[View] = None
        self.groups = 1


class _Plan:
    """All HBM buffers for one (batch per group, H, W, groups) shape."""

    def __init__(self, eng: 'StepEngine', B: int, H: int, W: int, G: int, trainable: bool = True, storage: str = 'fp32',
                 teacher=None):
        # trainable = False: a forward-only ("light") plan for no-grad calls -- validation / inference at native slice
        # sizes creates one plan per shape, and those need no gradient buffers, kept Winograd inputs or scratch slabs
        # teacher = callable(parameter) -> byte offset: a forward-only plan of the BACKBONE whose ops read every parameter at
        # `address + offset` -- the optimizer's shadow slab (--cr_teacher ema).  Owned by the training plan it serves
        # (_Plan.teacher_plan), never in StepEngine.plans; no auxiliary path, no loss buffers of its own.
        self.B, self.H, self.W, self.G = B, H, W, G
        self.trainable = trainable
        self.teacher = teacher
        self.teacher_plan = None                      # (a training plan: its teacher plan, StepEngine._teacher_plan_for)
        off = teacher if teacher is not None else (lambda p: 0)
        # 16-bit storage (BASELINE config 5): every NHWC activation / activation-gradient buffer of this plan is fp16 and the
        # launches go to the _h16 entry points (include/pacingpseudo_hip_h16.h); weights, logits, statistics, parameter
        # gradients and workspaces stay fp32.  The loss gradients are multiplied by a static power-of-two scale so that the
        # small activation gradients stay inside fp16's normal range; the gradient slab is divided by it after the backward.
        # Round 6: storage 'bf16' (what BASELINE.json configs[4] names) -- the same plan with bfloat16 buffers and the _bf16 entry
        # points.  bfloat16 has fp32's exponent range, so its gradients need no loss scale to stay representable; the scale is
        # kept (same default, exact power of two) because the matrix kernels stage 16-bit operands as fp16 numbers.
        self.storage = storage
        self.h16 = storage != 'fp32'              # "16-bit storage" (either kind): what the layout / kernel-family decisions ask
        self.es = 2 if self.h16 else 4
        self.K = lib_for(storage)
        self.loss_scale = eng.loss_scale if self.h16 else 1.0
        adt = {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}[storage]
        self.act_dtype = adt
        self.Bt = B * G
        self.generation = 0
        dev = eng.device
        self._keep: List[torch.Tensor] = []
        f32 = dict(device=dev, dtype=torch.float32)

        self.lazy_coefs: List[torch.Tensor] = []      # coefficient rows of every buffer that can be lazy
        self.lazy_flags: List[list] = []
        self.lazy_mode = None                         # (backbone BN training, aux BN training) of the last forward
        self.packed_key = None                        # StepEngine._weights_key() of the weights this plan's packs were made from

        def act(n, h, w, c, groups=0):
            """A fresh (n, h, w, c) buffer and its view; groups > 0: the buffer may hold a LAZY tensor (coefficient rows)."""
            t = torch.empty((n, h, w, c), device=dev, dtype=adt)
            self._keep.append(t)
            if not groups:
                return t, View(t.data_ptr(), c, c, n, h, w, t, es=self.es)
            coef = torch.empty((groups, 3, c), **f32)
            flag = [False]
            self.lazy_coefs.append(coef)
            self.lazy_flags.append(flag)
            return t, View(t.data_ptr(), c, c, n, h, w, t, 0, 0, coef, coef.data_ptr(), groups, flag, self.es)

        Bt = self.Bt
        net = eng.backbone
        encs, decs = net.enc_blocks(), net.dec_blocks()
        ch = net.ch_ls
        # spatial size per encoder stage
        sizes = []
        h, w = H, W
        for e in encs:
            if e.pooling is not None or getattr(e, 'stride', 1) == 2:
                if h % 2 or w % 2:
                    raise ValueError(f'input {H}x{W} is not divisible by the encoder stride')
                h, w = h // 2, w // 2
            sizes.append((h, w))
        self.sizes = sizes
        # decoder stage k concatenates up(lower) with encoder stage k's output at that stage's size
        self.cat: Dict[int, View] = {}
        self.dcat: Dict[int, View] = {}
        for k in (5, 4, 3, 2, 1):
            d = decs[k]
            hk, wk = sizes[k - 1]
            _, self.cat[k] = act(Bt, hk, wk, d.up_ch + d.skip_ch, G)
            if trainable:
                _, self.dcat[k] = act(Bt, hk, wk, d.up_ch + d.skip_ch)
        self.x0 = act(Bt, H, W, _pad4(net.input_ch))[1]

        max_elems = 0
        self.layers: List[_Layer] = eng.layers
        self.enc_out: Dict[int, View] = {}
        self.enc_in: Dict[int, View] = {}
        self.pooled: Dict[int, View] = {}
        self.dpooled: Dict[int, View] = {}
        self.mid: Dict[str, View] = {}
        self.zbuf: Dict[str, torch.Tensor] = {}
        self.coef: Dict[str, torch.Tensor] = {}
        self.conv: Dict[str, ConvOp] = {}  # per layer: its kernel family (.sel) and packed weights, bound to self.K
        self.norm: Dict[str, NormOp] = {}  # per layer: its BatchNorm / GroupNorm launches, bound to self.K and the buffers above
        self.wino_ws = 0
        self.wg_ws_bytes = 0               # workspace of the weight-gradient calls alone (they may run on a second stream)
        self.ct_ws = 0                     # ConvTranspose2d weight-gradient workspace (--is_trans_conv)

        # ---- which layer outputs stay LAZY in train-mode BN (static per plan): every consumer of the tensor must have a
        # kernel form that applies BatchNorm + LeakyReLU while loading.  Decided before any buffer is laid out, because a
        # lazy layer writes its raw convolution output z straight into the buffer y would have occupied.
        stages = [int(s_.rsplit('stage', 1)[1]) for s_ in eng.aux.feat_stage] if eng.aux is not None else []
        aux_alias = bool(stages == [6, 5] and decs[5].identity_up and len({sizes[s_ - 1] for s_ in stages}) == 1)
        def halo_lazy_ok(Lc: _Layer, h, w):
            """The direct (two-half halo) forward kernel and the halo-tile weight-gradient kernels of layer Lc read a lazy input."""
            sel = conv_select(Lc, h, w, self.h16)
            # (fp32 storage by default: with fp16 tensors the saved pass is half as long -- same-box A/B by family: BatchNorm
            # -0.5 ms, halo +0.16, weight gradients +0.07 with fp32 storage; -0.23 / +0.20 / +0.10 with 16-bit storage, i.e. nothing:
            # engine.LAZY_HALO_H16 switches it on there)
            return bool(LAZY_HALO and (not self.h16 or LAZY_HALO_H16) and sel.kind == 'f16x3' and Lc.stride == 1 and G <= 2
                        and self.K.pp_conv3x3_lazy_ok(Lc.cin, Lc.cout, self.Bt, h, w, Lc.dil) == 1)
        self.lazy_out: Dict[str, bool] = self._decide_lazy(eng, sizes, halo_lazy_ok)

        def conv_bufs(L: _Layer, n, h, w):
            """Packed-weight buffers of one conv layer and the choice direct vs Winograd."""
            nonlocal max_elems
            sel = conv_select(L, h, w, self.h16)
            vkeep = amax = None
            if sel.kind == 'wino':
                planes = (sel.tile + 2) ** 2                                    # 16 or 36
                wf = torch.empty((planes, L.cout, L.cin), **f32)                # Uf
                wb = torch.empty((planes, L.cin, L.cout), **f32)                # Ub
                # transformed input of the forward pass, kept for the weight gradient (2.25-4x the activation, a few
                # GB in total at the benchmark shape: cheaper in 288 GB of HBM than a second transform pass)
                if trainable:
                    vkeep = torch.empty(lib.pp_conv3x3_wino_vkeep_elems(L.cin, n, h, w, L.dil), **f32)
                    self.wino_ws = max(self.wino_ws, lib.pp_conv3x3_wino_workspace(L.cout, L.cin, n, h, w, L.dil),
                                       lib.pp_conv3x3_wino_bwd_weight_workspace(L.cout, L.cin, n, h, w, L.dil))
                    self.wg_ws_bytes = max(self.wg_ws_bytes, lib.pp_conv3x3_wino_bwd_weight_workspace(L.cout, L.cin, n, h, w, L.dil))
                self.wino_ws = max(self.wino_ws, lib.pp_conv3x3_wino_workspace(L.cin, L.cout, n, h, w, L.dil))
            else:
                # (the same buffers hold the [hi4 | lo4] fp16 pairs when the layer runs on the split-fp16 kernels)
                wf = torch.empty((L.cout, 9, L.cin_pad), **f32)
                wb = torch.empty((L.cin, 9, L.cout), **f32) if L.cin_pad == L.cin else None
            if trainable and (sel.kind == 'f16x3' or sel.split):
                amax = torch.zeros(1, **f32)                    # max |dz| of the step, written by the BN backward
            self.conv[L.name] = ConvOp(sel, L, self.K, SLOPE, wf, wb, vkeep, amax, off(L.conv.weight), off(L.conv.bias))
            max_elems = max(max_elems, n * h * w * max(L.cout, L.cin_pad))

        self.bn_stats_bytes = 0

        def layer_bufs(L: _Layer, n, h, w, groups):
            self.bn_stats_bytes = max(self.bn_stats_bytes, lib.pp_conv3x3_bn_stats_bytes(L.cout, n, h, w, groups))
            # pre-BatchNorm output z: a lazy layer keeps it in its OUTPUT buffer (train mode) or never stores it (eval mode,
            # fused epilogue), so only the other layers -- and every layer of the unfused A/B path -- own a z buffer
            if not (self.lazy_out[L.name] and FUSE_BN):
                self.zbuf[L.name] = act(n, h, w, L.cout)[0]
            # GroupNorm: [mean, invstd, scale, shift, xbar] rows per IMAGE (pp_gn_stats), whatever the statistics groups
            coef = self.coef[L.name] = torch.empty((5, n, L.cout) if L.gn else (4, groups, L.cout), **f32)
            # per-channel sums of the split (synchronised) BatchNorm calls: [0] forward, [1] backward local, [2] backward global
            sums = torch.zeros((3, groups, 2, L.cout), device=dev, dtype=torch.float64)
            # a stride-2 convolution runs as a stride-1 convolution at the input resolution, (2 h, 2 w) for the output size (h, w):
            # full-resolution z and (zero-stuffed) dz
            s = L.stride
            zfull = act(n, 2 * h, 2 * w, L.cout)[0] if s == 2 else None
            dzfull = act(n, 2 * h, 2 * w, L.cout)[0] if (s == 2 and trainable) else None
            conv_bufs(L, n, s * h, s * w)
            self.norm[L.name] = NormOp(self.K, L, SLOPE, BN_EPS, BN_MOM, coef, self.zbuf.get(L.name), self.lazy_out[L.name], sums,
                                       zfull, dzfull, self.conv[L.name].amax, off(L.bn.weight), off(L.bn.bias))

        cur = self.x0
        for k, e in enumerate(encs, start=1):
            hk, wk = sizes[k - 1]
            if e.pooling is not None:
                self.pooled[k] = act(Bt, hk, wk, cur.C)[1]
                if trainable:
                    self.dpooled[k] = act(Bt, hk, wk, cur.C)[1]
                cur = self.pooled[k]
            self.enc_in[k] = cur
            L1, L2 = eng.enc_layers[k]
            layer_bufs(L1, Bt, hk, wk, G)
            layer_bufs(L2, Bt, hk, wk, G)
            self.mid[L1.name] = act(Bt, hk, wk, L1.cout, G)[1]
            if k <= 5:      # skip slot of decoder stage k
                d = decs[k]
                out = _sub(self.cat[k], d.up_ch, d.skip_ch)
            else:           # stage 6 feeds decoder stage 5 as its lower input
                out = self._lower_slot(5, decs, sizes, act, L2.cout, hk, wk)
            self.enc_out[k] = out
            cur = out
        self.dec_out: Dict[int, View] = {}
        self.gdec: Dict[int, View] = {}
        self.low_src: Dict[int, View] = {5: self.enc_out[6]}
        for k in (5, 4, 3, 2, 1):
            hk, wk = sizes[k - 1]
            L1, L2 = eng.dec_layers[k]
            layer_bufs(L1, Bt, hk, wk, G)
            layer_bufs(L2, Bt, hk, wk, G)
            self.mid[L1.name] = act(Bt, hk, wk, L1.cout, G)[1]
            if k > 1:
                out = self._lower_slot(k - 1, decs, sizes, act, L2.cout, hk, wk)
                self.low_src[k - 1] = out
            else:
                out = act(Bt, hk, wk, L2.cout, G)[1]
            self.dec_out[k] = out
        # gradient wrt each stage output that is NOT a slice of a dcat buffer
        self.g_low: Dict[int, View] = {}
        for k in (5, 4, 3, 2, 1):
            d = decs[k]
            if not d.identity_up and trainable:
                src = self.low_src[k]
                self.g_low[k] = act(Bt, src.H, src.W, src.C)[1]
            if d.trans and trainable:
                self.ct_ws = max(self.ct_ws, lib.pp_convtranspose_bwd_weight_workspace(d.lower_ch, d.skip_ch, d.scale, Bt,
                                                                                       self.low_src[k].H, self.low_src[k].W))
        if trainable:
            self.g_head = act(Bt, H, W, ch[0])[1]
            self.dlogits = torch.empty((Bt, net.num_classes, H, W), **f32)

        # auxiliary path (one group of B samples at the stage-5/6 resolution)
        self.aux = None
        self.aux_error = None
        hs = {sizes[s - 1] for s in stages}
        if len(hs) > 1:
            # the reference fails in torch.cat here (aux_path_memory.py:49) -- but only when the path is used
            self.aux_error = ('Sizes of tensors must match except in dimension 1: the auxiliary path concatenates '
                              f'stages {eng.aux.feat_stage} of different spatial size')
        if eng.aux is not None and self.aux_error is None and teacher is None:
            ax = eng.aux
            ha, wa = sorted(hs)[0]
            LA = eng.aux_layer
            a = dict(h=ha, w=wa, stages=stages)
            a['alias_cat5'] = aux_alias
            if not a['alias_cat5']:
                a['in'] = act(B, ha, wa, LA.cin_pad)[1]
                if trainable:
                    a['din'] = act(B, ha, wa, LA.cin_pad)[1]
            layer_bufs(LA, B, ha, wa, 1)        # (never lazy: the aux features are always materialised, memory_update reads them)
            a['feat'] = act(B, ha, wa, LA.cout)[1]
            if trainable:
                a['dfeat'] = act(B, ha, wa, LA.cout)[1]
            if ax.aux_drop_prob > 0:        # Dropout2d (aux_path_memory.py:22,31): masked copies + their gradients
                a['drop_in'] = act(B, ha, wa, LA.cin_pad)[1]
                a['drop_feat'] = act(B, ha, wa, LA.cout)[1]
                a['drop_bank'] = torch.empty((ax.num_classes, ax.hid_ch), **f32)
                if trainable:
                    a['drop_din'] = act(B, ha, wa, LA.cin_pad)[1]
                    a['drop_dfeat'] = act(B, ha, wa, LA.cout)[1]
            a['lo'] = torch.empty((B, ax.num_classes, ha, wa), **f32)
            if trainable:
                a['dlo'] = torch.empty((B, ax.num_classes, ha, wa), **f32)
            self.aux = a

        # per-block BatchNorm partial sums emitted by the fused convolution epilogues (one buffer, stream-ordered reuse)
        self.bn_stats = torch.empty(self.bn_stats_bytes // 8 + 2, device=dev, dtype=torch.float64)
        self.rows_out = ctypes.c_int(0)
        # two scratch slabs for the transient gradients (dz of the current layer / dy of the layer below)
        if trainable:
            self.s1 = torch.empty(max_elems, device=dev, dtype=adt)
            self.s2 = torch.empty(max_elems, device=dev, dtype=adt)
            # second dz buffer + events: layer L + 1 writes its dz while the weight gradient of layer L still reads the other one
            self.s1b = torch.empty(max_elems, device=dev, dtype=adt) if WGRAD_STREAM else None
            self.dz_ready = [torch.cuda.Event(), torch.cuda.Event()]
            # (events are created here, not lazily inside a step; wg_pending: recorded during the backward pass in flight --
            # every backward starts with both slots free, the previous one having joined the second stream before it returned,
            # so no step waits on an event of an earlier step and a backward is self-contained for hipGraph capture)
            self.wg_done = [torch.cuda.Event(), torch.cuda.Event()]
            self.wg_pending = [False, False]
            self.dz_slot = 0
            self.bucket_ev = torch.cuda.Event() if WGRAD_STREAM else None      # main -> second stream, at gradient-bucket boundaries

        # workspaces (the weight-gradient query sizes for the largest CU budget a launch may run under, whatever this thread set)
        self.res = None                  # (workspace, bytes, stats buffer, bytes) of the SECOND stream while the aux forward runs there
        self.bn_stats_side = None
        aux_side_ws = 0
        loss_ws = max(lib.pp_seg_losses_workspace(B, H * W), 1024 * 16)
        if eng.aux is not None:
            loss_ws = max(loss_ws, lib.pp_memory_update_workspace(net.num_classes, eng.aux.hid_ch))
        wg = 0
        bn = 0
        for L in eng.layers + ([eng.aux_layer] if self.aux is not None else []):
            n = Bt if L is not eng.aux_layer else B
            g = G if L is not eng.aux_layer else 1
            hL, wL = self._layer_hw(eng, L)
            if trainable:
                wg = max(wg, lib.pp_conv3x3_bwd_weight_workspace(L.cout, L.cin_pad, n, hL, wL))
                self.wg_ws_bytes = max(self.wg_ws_bytes, lib.pp_conv3x3_bwd_weight_workspace(L.cout, L.cin_pad, n, hL, wL))
            bn = max(bn, lib.pp_bn_workspace(L.cout, (n // g) * hL * wL, g) + 12 * g * L.cout)
            if L.gn:
                bn = max(bn, lib.pp_gn_workspace(L.cout, hL * wL, n))
            if trainable and L.cin == 1:
                bn = max(bn, lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(L.cout, (n // g) * hL * wL, g),
                         lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(L.cout, n * hL * wL, 1))
            if L is eng.aux_layer:      # what the auxiliary forward needs when it runs on the second stream (its own workspace / statistics rows)
                aux_side_ws = max(lib.pp_bn_workspace(L.cout, (n // g) * hL * wL, g) + 12 * g * L.cout, loss_ws,
                                  lib.pp_conv1x1_bwd_workspace(net.num_classes, L.cout, n, hL * wL),
                                  lib.pp_conv3x3_wino_workspace(L.cin, L.cout, n, hL, wL, L.dil) if self.conv[L.name].sel.kind == 'wino' else 0)
        head = lib.pp_conv1x1_bwd_workspace(net.num_classes, ch[0], Bt, H * W)
        if self.aux is not None:
            head = max(head, lib.pp_conv1x1_bwd_workspace(net.num_classes, eng.aux_layer.cout, B,
                                                          self.aux['h'] * self.aux['w']))
        self.ws_bytes = max(wg, bn, head, loss_ws, self.wino_ws, self.ct_ws) + 256
        self.ws = torch.empty(self.ws_bytes, device=dev, dtype=torch.uint8)
        self.ws_wg = None
        if trainable and WGRAD_STREAM:
            self.wg_ws_bytes = max(self.wg_ws_bytes, aux_side_ws) + 256
            self.ws_wg = torch.empty(self.wg_ws_bytes, device=dev, dtype=torch.uint8)
            if self.aux is not None:
                LA_ = eng.aux_layer
                self.bn_stats_side_bytes = lib.pp_conv3x3_bn_stats_bytes(LA_.cout, B, self.aux['h'], self.aux['w'], 1)
                self.bn_stats_side = torch.empty(self.bn_stats_side_bytes // 8 + 2, device=dev, dtype=torch.float64)
                self.aux_fork, self.aux_join = torch.cuda.Event(), torch.cuda.Event()
        # loss denominators / numerators, packed so that data-parallel runs all-reduce them ONCE per step:
        # [0:6] segmentation losses (pp_seg_losses_fwd), [6:8] auxiliary partial CE (pp_aux_pce_fwd)
        # The pairs of the regularisers that are on (regop.REGULARISERS, in its order) sit between them from [6:8] on, the auxiliary
        # pair last: a step without the auxiliary path still reduces one contiguous block, [0:6 + 2 * len(regs)].
        # --cr_teacher ema: the six sums of the teacher's pp_seg_losses_fwd call (student-strong against teacher-weak) sit BEHIND
        # the auxiliary pair in the same allocation -- all_sums keeps its length, and a data-parallel step with the teacher on
        # reduces sums_store whole, still one collective.
        n_sums = 8 + 2 * len(eng.regs)
        self.sums_store = torch.zeros(n_sums + 6, device=dev, dtype=torch.float64)
        self.all_sums = self.sums_store[:n_sums]
        self.sums_teacher = self.sums_store[n_sums:]
        # parameters the forward reads outside the ConvOp / NormOp objects: the 1x1 head, the transposed convolutions
        fc = net.final_conv
        self.head_off = (off(fc.weight), off(fc.bias))
        self.up_off = {k: off(d.up_samp.weight) for k, d in decs.items() if d.trans}
        self.regs = {}                   # {name: RegOp}; a teacher plan evaluates no loss
        for i, (name, prm) in enumerate(eng.regs.items() if teacher is None else ()):
            REGULARISERS[name].check(K=net.num_classes, C=net.input_ch, **prm)
            s0 = 6 + 2 * i
            self.regs[name] = RegOp.alloc(self.K, REGULARISERS[name], prm, self.all_sums[s0:s0 + 2], self.all_sums[s0 - 2:], B,
                                          net.num_classes, net.input_ch, H, W, trainable)
        self.sums = self.all_sums[:6]
        if self.aux is not None:
            s0 = 6 + 2 * len(self.regs)
            self.aux['sums'] = self.all_sums[s0:s0 + 2]
        self.target = torch.empty((B, H, W), device=dev, dtype=torch.int64)

    def ws_args(self):
        """(pointer, bytes) of the workspace of the stream that is being launched on (the second stream's while `res` is set)."""
        return (self.res[0].data_ptr(), self.res[1]) if self.res is not None else (self.ws.data_ptr(), self.ws_bytes)

    def stats_args(self):
        """(pointer, bytes) of the buffer the fused convolution epilogues leave their per-block BatchNorm sums in."""
        return (self.res[2].data_ptr(), self.res[3]) if self.res is not None else (self.bn_stats.data_ptr(), self.bn_stats_bytes)

    def begin_forward(self, mode):
        """Start of a forward through this plan: no buffer is lazy yet (the lazy layers of this forward set their flags as
        they run); when the BatchNorm mode differs from the previous forward's, the coefficient rows go back to the identity
        (1, 0, 1), because slices a lazy layer wrote last time may now receive final values."""
        self.generation += 1             # any forward through this plan overwrites its activation buffers
        for f in self.lazy_flags:
            f[0] = False
        if mode != self.lazy_mode:
            for c in self.lazy_coefs:
                c[:, 0].fill_(1.0)
                c[:, 1].zero_()
                c[:, 2].fill_(1.0)
            self.lazy_mode = mode

    def _lower_slot(self, k, decs, sizes, act, c, h, w) -> View:
        """Where the tensor feeding decoder stage k as `lower` is written: straight into cat_k when the
        up-sampling factor is 1 (an exact identity), else into its own buffer (then resized into cat_k)."""
        if decs[k].identity_up:
            return _sub(self.cat[k], 0, c)
        return act(self.Bt, h, w, c, self.G)[1]

    @staticmethod
    def _decide_lazy(eng, sizes, halo_lazy_ok=None) -> Dict[str, bool]:
        """{layer name: its output is a lazy tensor in train-mode BN}.  The consumers of a layer output are: the next
        convolution (directly, or through a concatenation buffer it is a slice of), the max-pooling / up-sampling in front
        of the next stage, the 1x1 head, the auxiliary path.  Each must be able to apply BatchNorm + LeakyReLU on load."""
        def hw(L, k):
            h, w = sizes[k - 1]
            return (2 * h, 2 * w) if L.stride == 2 else (h, w)

        def mid_ok(Lc, k):
            """The second convolution of a DoubleConv as the ONLY consumer of the first one's output: the two-half halo kernel +
            halo-tile weight gradient read it lazily (halo_lazy_ok)."""
            return halo_lazy_ok is not None and halo_lazy_ok(Lc, *hw(Lc, k))

        out = {L.name: False for L in eng.layers}
        if eng.aux_layer is not None:
            out[eng.aux_layer.name] = False
        if not (LAZY_BN and FUSE_BN):       # the lazy forms hang off the fused conv + BN entry points
            return out
        if any(L.gn for L in eng.layers):   # GroupNorm outputs are always materialised (the lazy consumers know <= 2 statistics groups)
            return out
        # stage outputs (skip connections, pooled / up-sampled / concatenated tensors, the auxiliary input) are always
        # materialised: their consumers (max-pooling, bilinear x2, Winograd input transform) have no on-load form (measured
        # slower, round 4).  Lazy are: the mid tensor of a DoubleConv whose second convolution runs on the halo kernels, and the
        # last decoder output (read by the 1x1 head only: pp_conv1x1_*_lazy).
        for k in range(1, 7):
            L1, L2 = eng.enc_layers[k]
            out[L1.name] = mid_ok(L2, k) and L1.stride == 1
        for k in (5, 4, 3, 2, 1):
            L1, L2 = eng.dec_layers[k]
            out[L1.name] = mid_ok(L2, k)
        out[eng.dec_layers[1][1].name] = True
        return out

    def _layer_hw(self, eng, L):
        if eng.aux is not None and L is eng.aux_layer:
            return self.aux['h'], self.aux['w']
        for k in range(1, 7):
            if L in eng.enc_layers[k]:
                h, w = self.sizes[k - 1]
                return (2 * h, 2 * w) if L.stride == 2 else (h, w)      # the size the convolution kernels run at
        for k in (5, 4, 3, 2, 1):
            if L in eng.dec_layers[k]:
                return self.sizes[k - 1]
        raise KeyError(L.name)


class StepEngine:
    def __init__(self, backbone, aux_path, args):
        self.backbone, self.aux, self.args = backbone, aux_path, args
        self.enc_layers: Dict[int, tuple] = {}
        self.dec_layers: Dict[int, tuple] = {}
        self.layers: List[_Layer] = []
        for k, e in enumerate(backbone.enc_blocks(), start=1):
            cb = e.conv_block
            p = f'enc_block{k}.conv_block.conv_layer'
            pair = (_Layer(p + '1', cb.conv_layer1.conv, cb.conv_layer1.norm_op, e.dilation),
                    _Layer(p + '2', cb.conv_layer2.conv, cb.conv_layer2.norm_op, e.dilation))
            self.enc_layers[k] = pair
            self.layers += list(pair)
        for k, d in backbone.dec_blocks().items():
            cb = d.conv_block
            p = f'dec_block{k}.conv_block.conv_layer'
            pair = (_Layer(p + '1', cb.conv_layer1.conv, cb.conv_layer1.norm_op, 1),
                    _Layer(p + '2', cb.conv_layer2.conv, cb.conv_layer2.norm_op, 1))
            self.dec_layers[k] = pair
            self.layers += list(pair)
        self.aux_layer = None
        if aux_path is not None:
            for s in aux_path.feat_stage:
                if not s.startswith('encoder/stage'):
                    raise NotImplementedError('auxiliary features must be encoder stages')
            self.aux_layer = _Layer('aux.bottleneck', aux_path.layer_bottleneck[1], aux_path.layer_bottleneck[2], 1)
        for L in self.layers[1:] + ([self.aux_layer] if self.aux_layer is not None else []):
            if L.cin % 4 or L.cout % 4:
                raise NotImplementedError(f'{L.name}: channel counts must be multiples of 4 (got {L.cin}->{L.cout})')
        if self.layers[0].cout % 4:
            raise NotImplementedError('init_ch must be a multiple of 4')
        self.plans: 'OrderedDict[tuple, _Plan]' = OrderedDict()      # least recently used first
        self.plans_built = 0
        self.world = 1
        self.rank = 0
        self.comm = None                 # set by pacingpseudo_amd.parallel.attach()
        self.sync_bn = False             # data-parallel only: BatchNorm batch statistics over the GLOBAL batch (epoch 0)
        self.bucket_hook = None          # callable(tag) fired as gradient buckets complete during backward
        self.last = None                 # state saved by forward for backward
        self._rec = None                 # per-layer (x, y, groups) views recorded by the forward in flight
        self.last_drop_masks = None      # Dropout2d masks of the most recent auxiliary forward (tests read them)
        self._bwd_rec = None
        self.last_plan = None            # plan of the most recent forward (tests look at its buffers)
        self._wg_stream = None           # second HIP stream of the weight gradients (created on first use)
        self._coefs_ready = frozenset()  # layers whose eval-mode coefficient rows the running forward has written in one batch
        self._bwd_plan = None            # plan of the backward pass in flight
        self._frozen = 0                 # frozen encoder stages of the forward in flight (backbone.frozen_stages, checked per forward)
        # --cr_teacher ema (ConsistencyRegulr.attach_teacher): {id(FlatSlab): (FlatSlab, shadow slab)} -- the weak view's prediction
        # of the consistency term comes from a forward-only pass that reads the optimizer's EMA shadow.  None: the step as it was.
        self.teacher = None
        self.teacher_resync = None       # callable: shadow := parameters wherever the optimizer has not averaged yet (invalidate_packed)
        # --cr_uncertainty (set_uncertainty): the teacher call of the consistency term is masked by the entropy of the teacher's mean
        # soft-max over noisy passes.  None: the step as it was -- no launch, no buffer, no output key, libpacingpseudo_unc.so not loaded.
        self.unc = None                  # dict(passes, sigma, clip, start, seed)
        self.unc_state = None            # (seed, step) of the noise generator: ONE int64[2] device buffer, owned by the engine
        # 16-bit storage of activations / activation gradients for TRAINING plans (`--storage fp16`, BASELINE config 5; PP_ACT_H16=1
        # forces it for A/B runs).  Forward-only plans (validation, inference at native slice sizes) stay fp32.
        # the regularisers on the weak logits that are switched on: {name: parameters}, constants of the run (checked here, before
        # any launch).  Absent: no launch, no buffer, no output key.
        self.regs = {r.name: r.check(K=backbone.num_classes, **r.args_params(args)) for r in active_regularisers(args)}
        self.storage = getattr(args, 'storage', 'fp32') or 'fp32'
        if os.environ.get('PP_ACT_H16', '0') == '1' and self.storage == 'fp32':
            self.storage = 'fp16'
        if self.storage not in ('fp32', 'fp16', 'bf16'):
            raise ValueError(f"--storage must be fp32, fp16 or bf16 (got {self.storage!r})")
        self.h16 = self.storage != 'fp32'
        self.loss_scale = float(os.environ.get('PP_LOSS_SCALE', '1024'))      # static, a power of two (exact to remove)
        if self.h16:
            if any(L.stride != 1 for L in self.layers) or any(d.trans for d in backbone.dec_blocks().values()):
                raise NotImplementedError('16-bit storage: the strided / transposed-convolution U-Net variant has no fp16 kernels')
            if not (F16X3_ENABLED and FUSE_BN):
                raise NotImplementedError('16-bit storage needs the split-fp16 matrix kernels and the fused BatchNorm epilogues')
        if any(L.gn for L in self.layers):
            if self.h16:
                raise NotImplementedError(f'--norm_op group has fp32 kernels only: --storage {self.storage} is not supported with it')
            if any(L.stride != 1 for L in self.layers) or any(d.trans for d in backbone.dec_blocks().values()):
                raise NotImplementedError('--norm_op group: the strided / transposed-convolution U-Net variant is not supported')

    # ------------------------------------------------------------------ plumbing
    @property
    def device(self):
        return self.backbone.final_conv.weight.device

    MAX_TRAIN_PLANS = 2       # a training run has one shape (plus, at most, the ragged last batch)
    MAX_INFER_PLANS = 8       # validation / inference at native slice sizes: one light plan per (batch, H, W)

    def plan_for(self, B, H, W, G, trainable: bool = True) -> _Plan:
        """Buffers for one shape.  Training plans and forward-only plans are cached separately, least recently used out
        first, and the plan of a forward that still awaits its backward is never evicted: a validation epoch over many
        slice sizes cannot push out (and so force the re-allocation of) the multi-GB training plan."""
        storage = self.storage if trainable else 'fp32'
        key = (B, H, W, G, self.device.index, bool(trainable), storage)
        p = self.plans.get(key)
        if p is not None:
            self.plans.move_to_end(key)
            return p
        limit = self.MAX_TRAIN_PLANS if trainable else self.MAX_INFER_PLANS
        same = [k for k in self.plans if k[5] == bool(trainable)]
        live = self.last['plan'] if self.last is not None else None
        for k in same:
            if len(same) < limit:
                break
            if self.plans[k] is not live:
                del self.plans[k]
                same = [q for q in same if q != k]
        p = _Plan(self, B, H, W, G, trainable, storage)
        self.plans_built += 1
        self.plans[key] = p
        return p

    def _check_input(self, t, name):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise TypeError(f'{name} must be a float32 tensor on the GPU (got {t.dtype} on {t.device})')
        return t.contiguous()

    # ------------------------------------------------------------------ layer primitives
    def _weights_key(self):
        """Changes whenever a convolution weight may have changed: the optimizer's slab version (the fused optimizers write
        through raw pointers and bump it), torch's in-place version counters (load_state_dict, user code) and the addresses."""
        ws = [L.conv.weight for L in self.layers] + ([self.aux_layer.conv.weight] if self.aux_layer is not None else [])
        slabs = {id(f): f for f in (getattr(w, '_pp_flat', None) for w in ws) if f is not None}      # FlatSlab back-references
        return (tuple((f.version, f.params._version) for f in slabs.values()), tuple(w._version for w in ws),
                tuple(w.data_ptr() for w in ws))

    def invalidate_packed(self) -> None:
        """Forget which weights the forward-only plans packed.  `_weights_key` sees optimizer steps (slab version), torch's
        in-place version counters and moved storage; writes that bypass all three -- ``p.data.copy_()`` / EMA updates through
        ``.data``, collectives on a view of the slab -- are the CALLER's to announce with this call.  Called by
        pacingpseudo_amd.parallel.attach and by ``load_state_dict`` of ConsistencyRegulr / UNet (a post-hook; so
        inference.load_backbone is covered too).  tests/test_gpu_round5.py: a ``.data`` write + this call re-packs."""
        for p in self.plans.values():
            p.packed_key = None
        if self.teacher_resync is not None:      # weights written in place behind the shadow's creation (--init_from, load_state_dict)
            self.teacher_resync()

    # ------------------------------------------------------------------ the EMA teacher of the consistency term
    def set_teacher(self, slabs, resync=None) -> None:
        """slabs: {id(FlatSlab): (FlatSlab, shadow slab of its parameters)} or None (off).  Existing teacher plans are dropped
        with their key (teacher_key), so a captured step is captured again."""
        self.teacher = dict(slabs) if slabs else None
        self.teacher_resync = resync if self.teacher is not None else None
        if self.teacher is None:
            self.unc = None              # the uncertainty mask is a mask on the teacher call
        for p in self.plans.values():
            p.teacher_plan = None

    def teacher_key(self):
        """What a teacher plan bakes in: which slabs, where their shadows live (part of GraphedStep's capture key)."""
        if self.teacher is None:
            return None
        return tuple((i, f.params.data_ptr(), e.data_ptr()) for i, (f, e) in sorted(self.teacher.items()))

    # ------------------------------------------------------------------ the uncertainty mask of the teacher call
    def set_uncertainty(self, passes=None, sigma=0.1, clip=0.2, start=0.75, seed=0) -> None:
        """``--cr_uncertainty``: from now on the teacher call of the consistency term acts where the entropy of the teacher's mean
        soft-max over `passes` noisy passes is below theta(epoch) (utils/uncertainty.py has the definition).  Needs an attached
        teacher.  ``set_uncertainty(None)`` (or 0) switches it off.  The (seed, step) state of the generator is one device buffer of
        the ENGINE, created at the first call and kept at its address ever after -- plans and captured graphs come and go around
        it; every call with settings rewrites it to (seed, 0), set_uncertainty_state restores a saved pair.  In a data-parallel
        run the seed is mixed with the rank (call parallel.attach first), so the ranks perturb their shards independently."""
        if not passes:
            self.unc = None
            return
        if self.teacher is None:
            raise ValueError('the uncertainty mask is a mask on the EMA teacher\'s call: attach_teacher(optimizer) first (--cr_teacher ema)')
        from .utils.uncertainty import check_uncertainty_params
        prm = check_uncertainty_params(passes, sigma, clip, start, seed, K=self.backbone.num_classes)
        self.unc = prm
        self.set_uncertainty_state((prm['seed'] + self.rank * 0x9E3779B97F4A7C15) & ((1 << 64) - 1), 0)

    def set_uncertainty_state(self, seed: int, step: int) -> None:
        """Write (seed, step) into the engine's state buffer, in place (``--resume``: before the first step)."""
        from .utils.uncertainty import state_tensor
        new = state_tensor(seed, step, self.device)
        if self.unc_state is None or self.unc_state.device != new.device:
            self.unc_state = new
        else:
            self.unc_state.copy_(new)

    def uncertainty_state(self):
        """(seed, step) as unsigned Python integers (synchronises), or None when the feature was never configured."""
        if self.unc_state is None:
            return None
        a, b = (int(v) & ((1 << 64) - 1) for v in self.unc_state.tolist())
        return a, b

    def uncertainty_stats(self) -> torch.Tensor:
        """double[3] on the device, written by the most recent training step: (sum of the mask, sum of the entropy over valid
        pixels, number of valid pixels).  A buffer of the teacher plan: read it before the next step."""
        tp = self.last_plan.teacher_plan if self.last_plan is not None else None
        if tp is None or getattr(tp, 'unc', None) is None:
            raise RuntimeError('uncertainty_stats: no training step with the uncertainty mask has run')
        return tp.unc['stats']

    def uncertainty_key(self):
        """What a captured step bakes in of the uncertainty mask: the settings and the ADDRESS of the state buffer (its content is
        read by the kernels, so a replay draws new noise).  theta changes per epoch, which the capture key contains already."""
        if self.unc is None:
            return None
        u = self.unc
        return (u['passes'], u['sigma'], u['clip'], u['start'], self.unc_state.data_ptr())

    def _uncertainty_buffers(self, tp: _Plan, B, K, Cin, H, W):
        """acc, mask, noisy image, the noisy passes' logits, stats and workspace: buffers of the TEACHER plan."""
        from ._unc import unc
        bufs = getattr(tp, 'unc', None)
        if bufs is None:
            dev = self.device
            f32 = dict(device=dev, dtype=torch.float32)
            nws = unc.punc_workspace_bytes(B, K, H * W)
            if nws == 0:
                raise RuntimeError(f'punc_workspace_bytes({B}, {K}, {H * W}) = 0: {unc.punc_last_error().decode()}')
            bufs = tp.unc = dict(acc=torch.empty((B, K, H, W), **f32), mask=torch.empty((B, 1, H, W), **f32),
                                 noisy=torch.empty((B, Cin, H, W), **f32), logits=torch.empty((B, K, H, W), **f32),
                                 stats=torch.zeros(3, device=dev, dtype=torch.float64),
                                 ws=torch.empty(nws // 8, device=dev, dtype=torch.float64), ws_bytes=nws)
        return bufs

    def _uncertainty_passes(self, tp: _Plan, image, logits_t, theta: float, valid_mask, st) -> None:
        """Behind the clean teacher pass, on the main stream, with the teacher's packs of this step: for every pass noise ->
        image pack -> the teacher plan's forward into ONE reused logits buffer -> punc_accumulate; then one punc_advance.  With
        sigma = 0 the only launch is punc_accumulate on the clean logits.  Leaves tp.unc['mask'] and tp.unc['stats']."""
        from ._unc import unc
        u = self.unc
        B, Cin, H, W = image.shape
        K = self.backbone.num_classes
        b = self._uncertainty_buffers(tp, B, K, Cin, H, W)
        vptr = valid_mask.data_ptr() if valid_mask is not None else None
        tail = (vptr, float(theta), b['acc'].data_ptr(), b['mask'].data_ptr(), None, b['stats'].data_ptr(), b['ws'].data_ptr(),
                b['ws_bytes'], st)
        if u['sigma'] == 0.0:
            unc.punc_accumulate(logits_t.data_ptr(), B, K, H * W, 0, 1, *tail)
            return
        T = u['passes']
        for t in range(T):
            unc.punc_noise_add(image.data_ptr(), image.numel(), u['sigma'], u['clip'], self.unc_state.data_ptr(), t,
                               b['noisy'].data_ptr(), st)
            tp.K.pp_pack_image_nchw_to_nhwc(b['noisy'].data_ptr(), B, Cin, H, W, tp.x0.ptr, tp.x0.ld, tp.x0.C, st)
            self._unet_forward(tp, False, st, b['logits'])
            unc.punc_accumulate(b['logits'].data_ptr(), B, K, H * W, t, T, *tail)
        unc.punc_advance(self.unc_state.data_ptr(), st)

    def _teacher_offset(self, p) -> int:
        """Bytes from parameter `p` to its averaged copy.  A parameter outside every slab the optimizer updates (a frozen encoder
        stage: released from the slab, never averaged) reads as its live value: offset 0."""
        flat = getattr(p, '_pp_flat', None)
        if flat is None:
            return 0
        ent = self.teacher.get(id(flat))
        if ent is None or not flat.owns(p):
            raise RuntimeError('the EMA teacher was attached to another parameter slab (the model was re-flattened: .cuda() / '
                               'freeze_encoder after attach_teacher); call attach_teacher(optimizer) again')
        return ent[1].data_ptr() - flat.params.data_ptr()

    def _teacher_plan_for(self, plan: _Plan) -> _Plan:
        """The teacher plan of training plan `plan`: B images, one statistics group, fp32, forward-only.  It is an attribute of
        the training plan -- not an entry of self.plans -- so it lives exactly as long as the plan whose captured graph holds its
        buffers, the LRU of validation plans cannot evict it and no forward-only plan of the same shape (live weights) is mistaken
        for it."""
        key = self.teacher_key()
        tp = plan.teacher_plan
        if tp is None or tp.teacher_key != key:
            tp = _Plan(self, plan.B, plan.H, plan.W, 1, False, 'fp32', teacher=self._teacher_offset)
            tp.teacher_key = key
            dev = self.device
            # what the training plan's loss calls need beside it: the gradient wrt the teacher logits (written, never read) and
            # the zero upstream gradient of the teacher call's partial-CE slot
            tp.dlogits_discard = torch.empty((plan.B, self.backbone.num_classes, plan.H, plan.W), device=dev, dtype=torch.float32)
            tp.zero = torch.zeros(1, device=dev, dtype=torch.float32)
            plan.teacher_plan = tp
        return tp

    def _teacher_forward(self, plan: _Plan, image, st, unc_args=None) -> torch.Tensor:
        """Logits (B,K,H,W) of the backbone under the averaged weights for the weak images, on the main stream: eval-mode
        BatchNorm from the model's live running statistics, nothing recorded for a backward pass, no parameter or buffer written.
        The packs are rebuilt in every step (no packed_key shortcut: a host decision a hipGraph replay would skip)."""
        tp = self._teacher_plan_for(plan)
        B, Cin, H, W = image.shape
        tp.begin_forward((False, False, self._frozen))
        rec, self._rec = self._rec, None
        try:
            self._pack_weights(tp, st, need_grad=True)
            tp.K.pp_pack_image_nchw_to_nhwc(image.data_ptr(), B, Cin, H, W, tp.x0.ptr, tp.x0.ld, tp.x0.C, st)
            logits = torch.empty((B, self.backbone.num_classes, H, W), device=image.device, dtype=torch.float32)
            self._unet_forward(tp, False, st, logits)
            if unc_args is not None:         # (theta, valid_mask): the noisy passes, with the same packs and nothing recorded either
                self._uncertainty_passes(tp, image, logits, unc_args[0], unc_args[1], st)
        finally:
            self._rec = rec
        return logits

    def _pack_weights(self, plan: _Plan, st, need_grad: bool = True):
        """Kernel-side weight layouts of every layer (split-fp16 operands, Winograd-domain U).  Forward operands on the main
        stream; the data-gradient operands (Ub / wb: first used much later, in the backward pass) on the second stream when
        there is one.  A forward without gradients whose weights are unchanged since the plan last packed them packs nothing
        (validation / inference: 23 launches per forward, 3 with the batched packs)."""
        key = None
        if not need_grad:
            key = self._weights_key()
            if plan.packed_key == key:
                return
        layers = self.layers + ([self.aux_layer] if (self.aux is not None and plan.aux is not None) else [])
        if PACK_BATCH:
            # one launch per family for all layers (the per-layer launches are 5 - 50 us each behind one another at the start of every
            # step); the item tables are rebuilt when a weight or a packed buffer moved
            bkey = tuple(L.conv.weight.data_ptr() + plan.conv[L.name].woff for L in layers)
            if getattr(plan, 'pack_batch_key', None) != bkey:
                direct, wino, single = [], [], []
                for L in layers:
                    item = plan.conv[L.name].pack_item()
                    if item is None:
                        single.append(L)
                    else:
                        (wino if isinstance(item, PpWinoPackItem) else direct).append(item)
                plan.pack_batch = ((PpPackItem * len(direct))(*direct) if direct else None, len(direct),
                                   (PpWinoPackItem * len(wino))(*wino) if wino else None, len(wino), single)
                plan.pack_batch_key = bkey
            d_arr, d_n, w_arr, w_n, layers = plan.pack_batch
            if d_n:
                lib.pp_pack_conv3x3_weights_f16x3_batch(d_arr, d_n, st)
            if w_n:
                lib.pp_wino_pack_weights_f16x3_batch(w_arr, w_n, st)
        for L in layers:
            plan.conv[L.name].pack(st)
        plan.packed_key = key

    def _frozen_stages(self) -> int:
        """N of ``freeze_encoder(N)``: encoder stages 1 .. N run eval-mode BatchNorm in every forward and have no backward.  The
        only supported set of non-trainable backbone parameters is exactly that prefix; anything else is refused here, before
        any launch, with the name of the first parameter that is on the wrong side."""
        n = int(getattr(self.backbone, 'frozen_stages', 0) or 0)
        prefixes = tuple(f'enc_block{k}.' for k in range(1, n + 1))
        for name, p in self.backbone.named_parameters():
            want = not name.startswith(prefixes) if prefixes else True
            if p.requires_grad != want:
                raise NotImplementedError(
                    f'backbone.{name}: requires_grad={p.requires_grad} with frozen_stages={n}; the engine trains everything or '
                    'everything but an encoder prefix -- use freeze_encoder(n) (--freeze_encoder N), which freezes '
                    'enc_block1 .. enc_block<n> as a whole')
        return n

    def _sync(self, training) -> bool:
        """Synchronised BatchNorm applies: train-mode statistics of a data-parallel run over the GLOBAL batch."""
        return bool(training and self.comm is not None and self.sync_bn)

    def _convbn_fwd(self, plan, L: _Layer, x: View, y: View, groups, training, st, pool_out: Optional[View] = None,
                    record: bool = True):
        """conv3x3 + BatchNorm + LeakyReLU of one layer.  pool_out: where the 2x2 max-pooled copy of the output goes when the
        caller wants it from the same pass; returns True when it was written (train-mode apply pass), else the caller pools.
        record=False: a layer of a frozen stage -- nothing is kept for a backward pass."""
        op, nop = plan.conv[L.name], plan.norm[L.name]
        assert x.C == L.cin_pad, (L.name, x.C, L.cin_pad)
        # LAZY output (train-mode BN): z goes straight into the buffer of y, the finalize writes the layer's (scale, shift,
        # slope) rows next to it and the separate normalise + activate pass (pp_bn_lrelu_fwd) does not run: the consumers
        # of the tensor evaluate y while they load it (plan.lazy_out guarantees that each of them can)
        lazy = bool(training and nop.lazy)
        zptr, zld = nop.z_dest(y, lazy)
        L.x, L.y, L.groups = x, y, groups
        if self._rec is not None and record:
            # what this step's backward reads (kept with the step, not the layer): input view (+ whether it was lazy),
            # output view, groups, whether the output is lazy (then the output buffer holds z)
            self._rec[L.name] = (x, y, groups, lazy, x.lazy)
        ws = plan.ws_args()
        stats = None        # (pointer, rows per group) of the statistics a fused convolution epilogue left
        if L.stride == 2:
            assert not lazy
            # stride-2 / padding-1 convolution = the stride-1 convolution sampled at the even pixels (NormOp.fwd gathers them)
            op.fwd(x, nop.zfull.data_ptr(), L.cout, ws, st)
        elif not FUSE_BN or L.gn:       # (PP_FUSE_BN=0 implies PP_LAZY_BN=0: no input is lazy here)
            op.fwd(x, zptr, zld, ws, st)
        elif training:
            # z + per-block (sum, sum of squares) from the conv epilogue -> finalize -> y = lrelu(z*scale + shift)
            rows = op.fwd_bn(x, zptr, zld, groups, 1, None, None, plan.stats_args(), ws, plan.rows_out, st)
            stats = (plan.stats_args()[0], rows)
        else:
            # running statistics are known before the convolution: the epilogue writes y, z never exists.  (The backbone's
            # coefficient rows were written by ONE launch at the start of the forward: _eval_coeffs_batch.)
            if L.name not in self._coefs_ready:
                nop.eval_coeffs(groups, st)
            op.fwd_bn(x, y.ptr, y.ld, groups, 2, *nop.rows[2:], plan.stats_args(), ws, plan.rows_out, st)
            return False
        # the max-pooled copy comes from the apply pass behind a fused epilogue or GroupNorm statistics
        pool_out = pool_out if (FUSE_POOL_FWD and (stats is not None or L.gn)) else None
        return nop.fwd(zptr, zld, y, groups, training, lazy, stats, self._sync(training), self.comm, self.world, pool_out, ws, st)

    def _convbn_bwd(self, plan, L: _Layer, dy: View, dx: Optional[View], dx_accumulate, training, grads, st, pool: Optional[View] = None):
        """dy: gradient wrt the layer output.  Writes parameter gradients, and dx (+)= data gradient.  pool: gradient of the
        2x2-max-pooled copy of the layer output (half the size of dy), added to each window's winner inside the BatchNorm backward."""
        # (y: the forward's output view; lazy_out: its buffer holds the pre-BatchNorm z instead)
        x, y, groups, lazy_out, x_lazy = self._bwd_rec[L.name]
        op, nop = plan.conv[L.name], plan.norm[L.name]
        kind = op.sel.kind
        xlz = x.lazy_arg() if (x_lazy and kind != 'wino') else None      # (Winograd: the kept V was made from y already)
        assert not x_lazy or kind == 'wino' or (xlz is not None and kind == 'f16x3'), f'{L.name}: lazy input without a lazy weight gradient'
        gw = grads[L.conv.weight]
        pg = (grads[L.bn.weight].data_ptr(), grads[L.bn.bias].data_ptr(), grads[L.conv.bias].data_ptr())
        sync = self._sync(training)
        eval_fused = FUSE_BN and not training       # eval-mode BN: the forward epilogue wrote y only
        ws = (plan.ws.data_ptr(), plan.ws_bytes)
        if (FUSE_WG1 and not L.gn and dx is None and pool is None and L.cin == 1 and L.stride == 1 and L.dil == 1 and not x_lazy
                and kind == 'fp32' and not sync):
            # the first layer: dz has one reader, the weight gradient
            nop.bwd_wgrad_c1(dy, y, lazy_out, x, groups, gw.data_ptr(), pg, training, eval_fused, ws, st)
            return
        side = self._side_stream(plan)
        slot = 0
        if side is not None:
            slot = plan.dz_slot
            plan.dz_slot ^= 1
            if plan.wg_pending[slot]:                   # the weight gradient that last read this dz buffer (two layers ago)
                torch.cuda.current_stream().wait_event(plan.wg_done[slot])
        # (stride 2: the gradients are those of the stride-1 convolution for dz scattered to the even pixels; dz is that buffer then)
        dz = nop.bwd(dy, y, lazy_out, groups, pg, (plan.s1b if slot else plan.s1).data_ptr(), pool, training, eval_fused, sync,
                     self.comm, self.world, ws, st)

        # Order on two streams: the weight gradient starts WITH the data gradient.  (Round 5 measured the alternative -- the weight
        # gradient enqueued behind the data gradient, so that it runs beside the HBM-bound BatchNorm backward of the next layer
        # instead of beside another matrix kernel: 31.9 -> 32.9 ms, the BatchNorm family 7.5 -> 9.7 ms.  The direct weight
        # gradients read 2 - 2.5 GB per launch themselves; profiles/r05_experiments/wgrad_behind_dgrad.log.)
        if side is None:
            op.bwd_weight(dz, x, gw.data_ptr(), ws, xlz, st)
        else:       # on the second stream, with its own workspace: it waits for everything the main stream has enqueued so far
            plan.dz_ready[slot].record(torch.cuda.current_stream())
            side.wait_event(plan.dz_ready[slot])
            op.bwd_weight(dz, x, gw.data_ptr(), (plan.ws_wg.data_ptr(), plan.wg_ws_bytes), xlz, side.cuda_stream)
            plan.wg_done[slot].record(side)
            plan.wg_pending[slot] = True
        if dx is not None:          # the critical chain, always on the main stream
            op.bwd_data(dz, x, dx, dx_accumulate, ws, st)

    def _side_stream(self, plan):
        """The second stream of the weight gradients, or None (switched off, or a plan without the second dz buffer)."""
        if not WGRAD_STREAM or getattr(plan, 's1b', None) is None:
            return None
        if self._wg_stream is None:
            self._wg_stream = torch.cuda.Stream(device=self.device)
        return self._wg_stream

    def _join_side_stream(self, plan):
        """The main stream waits for every weight gradient enqueued so far (before a gradient bucket is handed to the
        all-reduce, and at the end of the backward pass: the optimizer reads the gradients next)."""
        if self._wg_stream is None:
            return
        for slot, ev in enumerate(plan.wg_done):
            if plan.wg_pending[slot]:
                torch.cuda.current_stream().wait_event(ev)

    # ------------------------------------------------------------------ backbone forward / backward
    def _eval_coeffs_batch(self, plan: _Plan, st):
        """Eval-mode BatchNorm (the reference from epoch 1 on, train_chaos.py:370): scale / shift of every backbone layer depend on
        parameters and running statistics only, so ONE launch at the start of the forward writes all 22 coefficient rows
        (pp_bn_eval_coeffs_batch; bit-identical to the per-layer pp_bn_eval_coeffs it replaces, which sat between the convolutions
        of the critical chain).  The item table is rebuilt when a parameter or a buffer moved."""
        layers = [L for L in self.layers if L.stride == 1 and not L.gn]
        if not layers:                  # a GroupNorm backbone: no BatchNorm coefficient rows to write
            return frozenset()
        key = tuple((L.bn.weight.data_ptr() + plan.norm[L.name].goff, L.bn.running_mean.data_ptr(), plan.coef[L.name].data_ptr()) for L in layers)
        if getattr(plan, 'coef_batch_key', None) != key:
            items = [PpBnCoefItem(L.cout, plan.coef[L.name].shape[1], *plan.norm[L.name].params(), *plan.norm[L.name].rows) for L in layers]
            plan.coef_batch = ((PpBnCoefItem * len(items))(*items), len(items), frozenset(L.name for L in layers))
            plan.coef_batch_key = key
        arr, n, names = plan.coef_batch
        lib.pp_bn_eval_coeffs_batch(arr, n, BN_EPS, st)
        return names

    def _unet_forward(self, plan: _Plan, training, st, logits: torch.Tensor, after_encoder=None):
        """after_encoder: called once every encoder stage has been enqueued (the auxiliary path reads stages 5 / 6: the composite
        step forks it to the second stream there, beside the decoder)."""
        self._coefs_ready = self._eval_coeffs_batch(plan, st) if (FUSE_BN and COEF_BATCH and not training) else frozenset()
        net = self.backbone
        decs = net.dec_blocks()
        G = plan.G
        encs = net.enc_blocks()
        pooled_done = False
        frozen = self._frozen
        for k, e in enumerate(encs, start=1):
            if e.pooling is not None and not pooled_done:
                src = plan.enc_out[k - 1]
                assert not src.lazy
                plan.K.pp_maxpool2_fwd(src.ptr, src.ld, plan.pooled[k].ptr, plan.pooled[k].ld, src.C, src.N, src.H, src.W, st)
            L1, L2 = self.enc_layers[k]
            # a frozen stage (freeze_encoder): eval-mode BatchNorm from the running statistics whatever the backbone's mode -- no
            # statistics update, no SyncBN all-reduce, no lazy output, no backward record (in a train-mode forward its coefficient
            # rows come from the per-layer pp_bn_eval_coeffs: _eval_coeffs_batch has not run)
            live = k > frozen
            tr = training and live
            self._convbn_fwd(plan, L1, plan.enc_in[k], plan.mid[L1.name], G, tr, st, record=live)
            # the next stage's max-pooling from the same pass that normalises this stage's output (train mode)
            nxt = plan.pooled.get(k + 1) if (k < 6 and encs[k].pooling is not None) else None
            pooled_done = bool(self._convbn_fwd(plan, L2, plan.mid[L1.name], plan.enc_out[k], G, tr, st, pool_out=nxt, record=live))
        if after_encoder is not None:
            after_encoder()
        for k in (5, 4, 3, 2, 1):
            d = decs[k]
            cat = plan.cat[k]
            if not d.identity_up:
                src = plan.low_src[k]
                dst = _sub(cat, 0, d.up_ch)
                if d.trans:                   # nn.ConvTranspose2d(lower, skip, k, k, bias=False), unet.py:140,149
                    plan.K.pp_convtranspose_fwd(src.ptr, src.ld, src.C, d.up_samp.weight.data_ptr() + plan.up_off[k], dst.ptr, dst.ld, d.up_ch,
                                             d.scale, src.N, src.H, src.W, st)
                else:
                    assert not src.lazy
                    plan.K.pp_bilinear_fwd(src.ptr, src.ld, dst.ptr, dst.ld, src.C, src.N, src.H, src.W, cat.H, cat.W, st)
            L1, L2 = self.dec_layers[k]
            self._convbn_fwd(plan, L1, cat, plan.mid[L1.name], G, training, st)
            self._convbn_fwd(plan, L2, plan.mid[L1.name], plan.dec_out[k], G, training, st)
        d1 = plan.dec_out[1]
        fc = net.final_conv
        fcw, fcb = fc.weight.data_ptr() + plan.head_off[0], fc.bias.data_ptr() + plan.head_off[1]
        lz = d1.lazy_arg()
        if lz is not None:
            plan.K.pp_conv1x1_nhwc_to_nchw_fwd_lazy(d1.ptr, d1.ld, d1.C, fcw, fcb,
                                                 logits.data_ptr(), net.num_classes, d1.N, d1.H * d1.W, ctypes.byref(lz), st)
        else:
            plan.K.pp_conv1x1_nhwc_to_nchw_fwd(d1.ptr, d1.ld, d1.C, fcw, fcb,
                                            logits.data_ptr(), net.num_classes, d1.N, d1.H * d1.W, st)

    def _unet_backward_decoder(self, plan: _Plan, training, grads, st, need_g6: bool = True):
        """need_g6=False (the whole encoder is frozen): the up-sampling backward of decoder stage 5, whose only product is the
        gradient wrt encoder stage 6, does not run (a ConvTranspose2d's own weight gradient still does)."""
        net = self.backbone
        decs = net.dec_blocks()
        d1 = plan.dec_out[1]
        fc = net.final_conv
        # (the lazy flags still describe the forward being differentiated: any later forward through this plan would have
        # raised in backward_step / unet_backward)
        a = (plan.dlogits.data_ptr(), d1.ptr, d1.ld, d1.C, fc.weight.data_ptr(), plan.g_head.ptr, plan.g_head.ld,
             grads[fc.weight].data_ptr(), grads[fc.bias].data_ptr(), net.num_classes, d1.N, d1.H * d1.W, 0, 0,
             plan.ws.data_ptr(), plan.ws_bytes)
        lz = d1.lazy_arg()
        if lz is not None:
            plan.K.pp_conv1x1_nchw_to_nhwc_bwd_lazy(*a, ctypes.byref(lz), st)
        else:
            plan.K.pp_conv1x1_nchw_to_nhwc_bwd(*a, st)
        g_out = plan.g_head
        for k in (1, 2, 3, 4, 5):
            L1, L2 = self.dec_layers[k]
            m = plan.mid[L1.name]
            dmid = View(plan.s2.data_ptr(), m.C, m.C, m.N, m.H, m.W, plan.s2[:m.N * m.H * m.W * m.C].view(m.N, m.H, m.W, m.C), es=plan.es)
            self._convbn_bwd(plan, L2, g_out, dmid, False, training, grads, st)
            self._convbn_bwd(plan, L1, dmid, plan.dcat[k], False, training, grads, st)
            # gradient wrt the `lower` input of this stage = gradient wrt the previous stage's output
            d = decs[k]
            glow = _sub(plan.dcat[k], 0, d.up_ch)
            if not d.identity_up:
                dst = plan.g_low[k]
                if d.trans:               # ConvTranspose2d: weight gradient from (lower input, d up-sampled), then the data gradient
                    src = plan.low_src[k]
                    plan.K.pp_convtranspose_bwd_weight(glow.ptr, glow.ld, d.up_ch, src.ptr, src.ld, src.C, d.scale, src.N, src.H, src.W,
                                                    grads[d.up_samp.weight].data_ptr(), 0, plan.ws.data_ptr(), plan.ws_bytes, st)
                    if k < 5 or need_g6:
                        plan.K.pp_convtranspose_bwd_data(glow.ptr, glow.ld, d.up_ch, d.up_samp.weight.data_ptr(), dst.ptr, dst.ld, dst.C,
                                                      d.scale, dst.N, dst.H, dst.W, 0, st)
                elif k < 5 or need_g6:
                    plan.K.pp_bilinear_bwd(glow.ptr, glow.ld, dst.ptr, dst.ld, dst.C, dst.N, dst.H, dst.W, glow.H, glow.W, 0, st)
                glow = dst
            g_out = glow          # for k == 5 this is the gradient wrt encoder stage 6
            if k == 4:
                self._bucket('decoder_upper')
            elif k == 5:
                self._bucket('dec5')
        return g_out

    def _enc_grad_view(self, plan, k, g6):
        if k == 6:
            return g6
        d = self.backbone.dec_blocks()[k]
        return _sub(plan.dcat[k], d.up_ch, d.skip_ch)

    def _unet_backward_encoder(self, plan: _Plan, training, grads, g6: View, st, frozen: int = 0):
        """frozen = N (freeze_encoder): the walk 6 -> 1 stops behind stage N + 1, whose first layer gets no data gradient; for the
        stages k <= N nothing is launched -- no norm backward, no weight or data gradient, no pooling gradient into them."""
        encs = self.backbone.enc_blocks()
        # the pooled-tensor gradient of stage k + 1, when it is folded into this stage's BatchNorm backward instead of being
        # added to the skip-gradient buffer by pp_maxpool2_bwd (not under synchronised BatchNorm: its split calls have no such form)
        fuse_pool = FUSE_POOL_BWD and not self._sync(training)
        pool_grad = None
        for k in range(6, frozen, -1):
            e = encs[k - 1]
            L1, L2 = self.enc_layers[k]
            g_out = self._enc_grad_view(plan, k, g6)
            m = plan.mid[L1.name]
            dmid = View(plan.s2.data_ptr(), m.C, m.C, m.N, m.H, m.W, plan.s2[:m.N * m.H * m.W * m.C].view(m.N, m.H, m.W, m.C), es=plan.es)
            self._convbn_bwd(plan, L2, g_out, dmid, False, training, grads, st, pool=pool_grad)
            pool_grad = None
            if k == frozen + 1:              # (k == 1 without frozen stages: the first layer of the network)
                self._convbn_bwd(plan, L1, dmid, None, False, training, grads, st)
                self._bucket('enc_rest' if k <= 4 else f'enc{k}')
                break
            gprev = self._enc_grad_view(plan, k - 1, g6)
            if e.pooling is not None:
                dp = plan.dpooled[k]
                self._convbn_bwd(plan, L1, dmid, dp, False, training, grads, st)
                src = plan.enc_out[k - 1]
                if fuse_pool and self.enc_layers[k - 1][1].stride == 1:
                    pool_grad = dp               # consumed by the BatchNorm backward of stage k - 1's last layer (next iteration)
                else:
                    plan.K.pp_maxpool2_bwd(src.ptr, src.ld, dp.ptr, dp.ld, gprev.ptr, gprev.ld, src.C, src.N, src.H, src.W, 1, st)
            else:
                self._convbn_bwd(plan, L1, dmid, gprev, True, training, grads, st)
            if k in (6, 5):
                self._bucket(f'enc{k}')

    def _bucket(self, tag):
        """Tell the data-parallel reducer that every gradient of bucket `tag` has been enqueued.

        Round 6: with the weight gradients on the second stream the bucket's all-reduce is issued FROM that stream, which first
        waits for an event of the main stream -- so RCCL's stream orders itself behind both (the bucket's BatchNorm / bias / head
        gradients are main-stream work, its weight gradients second-stream work) and the MAIN stream is not blocked at the bucket
        boundary.  Round 5 made the main stream wait for every pending weight gradient at each of the six boundaries
        (`_join_side_stream`), forfeiting part of the two-stream overlap in data-parallel runs; the
        main stream now waits once, for the collectives themselves, at the end of the backward pass (GradReducer.reduce)."""
        if self.bucket_hook is None:
            return
        plan = self._bwd_plan
        side = self._side_stream(plan) if plan is not None else None
        if side is None or getattr(plan, 'bucket_ev', None) is None:
            if plan is not None:
                self._join_side_stream(plan)
            self.bucket_hook(tag)
            return
        plan.bucket_ev.record(torch.cuda.current_stream())
        side.wait_event(plan.bucket_ev)
        with torch.cuda.stream(side):
            self.bucket_hook(tag)

    # ------------------------------------------------------------------ public: inference of the bare backbone
    @torch.no_grad()
    def infer_end_points(self, x: torch.Tensor, training: bool):
        x = self._check_input(x, 'x')
        B, Cin, H, W = x.shape
        self._frozen = self._frozen_stages()
        plan = self.plan_for(B, H, W, 1, trainable=False)
        self.last_plan = plan
        plan.begin_forward((bool(training), False, self._frozen))
        self._rec = None
        st = stream_ptr()
        self._pack_weights(plan, st, need_grad=False)
        plan.K.pp_pack_image_nchw_to_nhwc(x.data_ptr(), B, Cin, H, W, plan.x0.ptr, plan.x0.ld, plan.x0.C, st)
        logits = torch.empty((B, self.backbone.num_classes, H, W), device=x.device, dtype=torch.float32)
        self._unet_forward(plan, training, st, logits)
        ep = {'segmentation/logits': logits}
        for k in range(1, 7):
            ep[f'encoder/stage{k}'] = self._as_nchw(plan.enc_out[k])
        for k in (5, 4, 3, 2, 1):
            ep[f'decoder/stage{k}'] = self._as_nchw(plan.dec_out[k])
        return ep

    # ------------------------------------------------------------------ public: the bare backbone, trainable
    def unet_forward_train(self, x: torch.Tensor):
        """UNet.forward with gradients (upper_bound_chaos.py:156): forward in the module's BN mode, state kept for
        unet_backward."""
        x = self._check_input(x, 'x')
        B, Cin, H, W = x.shape
        self._frozen = self._frozen_stages()
        plan = self.plan_for(B, H, W, 1)
        self.last_plan = plan
        training = self.backbone.training
        plan.begin_forward((bool(training), False, self._frozen))
        self._rec = {}
        st = stream_ptr()
        self._pack_weights(plan, st)
        plan.K.pp_pack_image_nchw_to_nhwc(x.data_ptr(), B, Cin, H, W, plan.x0.ptr, plan.x0.ld, plan.x0.C, st)
        logits = torch.empty((B, self.backbone.num_classes, H, W), device=x.device, dtype=torch.float32)
        self._unet_forward(plan, training, st, logits)
        ep = {'segmentation/logits': logits}
        if self.backbone.elab_end_points:
            for k in range(1, 7):
                ep[f'encoder/stage{k}'] = self._as_nchw(plan.enc_out[k])
            for k in (5, 4, 3, 2, 1):
                ep[f'decoder/stage{k}'] = self._as_nchw(plan.dec_out[k])
        self.last = dict(unet=True, rec=self._rec, gen=plan.generation, plan=plan, bn_training=training, frozen=self._frozen)
        return ep

    def unet_backward(self, dlogits: torch.Tensor, grads: Dict[torch.nn.Parameter, torch.Tensor],
                      state: Optional[dict] = None):
        """Backward of unet_forward_train: d loss / d logits (N,K,H,W) -> parameter gradients."""
        S = state if state is not None else self.last
        if S is None or not S.get('unet'):
            raise RuntimeError('unet_backward called without a recorded unet_forward_train')
        if S is self.last:
            self.last = None
        plan: _Plan = S['plan']
        if plan.generation != S['gen']:
            raise RuntimeError('unet_backward: another forward ran through the same buffers after the forward being '
                               'differentiated; call backward before the next forward')
        if tuple(dlogits.shape) != tuple(plan.dlogits.shape):
            raise ValueError(f'gradient of the logits has shape {tuple(dlogits.shape)}, expected {tuple(plan.dlogits.shape)}')
        self._bwd_rec, self._rec = S['rec'], None
        self._bwd_plan = plan
        if getattr(plan, 'wg_pending', None) is not None:
            plan.wg_pending[0] = plan.wg_pending[1] = False
            plan.dz_slot = 0
        st = stream_ptr()
        if plan.loss_scale != 1.0:
            torch.mul(dlogits.to(torch.float32), plan.loss_scale, out=plan.dlogits)
        else:
            plan.dlogits.copy_(dlogits.to(torch.float32))
        with self._wgrad_budget(plan):
            g6 = self._unet_backward_decoder(plan, S['bn_training'], grads, st, need_g6=S['frozen'] < 6)
            self._unet_backward_encoder(plan, S['bn_training'], grads, g6, st, S['frozen'])
        self._join_side_stream(plan)

    def _wgrad_budget(self, plan):
        """Context: the CU budget of the direct weight-gradient kernels for one backward pass (this thread's launches only --
        the library keeps it per thread), put back on exit so that direct ABI callers on the same thread see what they set."""
        eng = self

        class _Budget:
            def __enter__(self):
                self.prev = lib.pp_get_wgrad_cus()
                lib.pp_set_wgrad_cus(WGRAD_CUS_SIDE if eng._side_stream(plan) is not None else WGRAD_CUS_FULL)

            def __exit__(self, *exc):
                lib.pp_set_wgrad_cus(self.prev)
                return False
        return _Budget()

    def _as_nchw(self, v: View) -> torch.Tensor:
        """Fresh NCHW-shaped (channels-last strided) copy of an engine buffer (a lazy one is normalised + activated on the way)."""
        out = torch.empty((v.N, v.H, v.W, v.C), device=self.device, dtype=v.dtype)
        lz = v.lazy_arg()
        if lz is not None:
            lib_for(v.storage).pp_lazy_materialize(v.ptr, v.ld, ctypes.byref(lz), out.data_ptr(), v.C, v.C, v.N, v.H * v.W, stream_ptr())
        else:
            lib_for(v.storage).pp_copy_slab(v.ptr, v.ld, out.data_ptr(), v.C, v.C, v.N * v.H * v.W, 0, stream_ptr())
        return out.float().permute(0, 3, 1, 2)

    def branch_mask(self, L: _Layer) -> torch.Tensor:
        """(N,C,H,W) bool: the LeakyReLU branch (pre-activation > 0) the kernels took for every output element of layer L in
        the last forward -- read from y, or from z and the layer's coefficients where the output stayed lazy (tests align the
        oracle's non-differentiable choices with the device's through this)."""
        y = L.y
        if y.lazy:
            # through the DEVICE's own expression (pp_lazy_materialize -> pp_lazy_apply4: one fma, as in every consumer and in
            # the BatchNorm backward): a torch restatement rounds twice and disagrees on elements within an ulp of the kink
            tmp = torch.empty((y.N, y.H, y.W, y.C), device=self.device, dtype=y.dtype)
            lz = y.lazy_arg()
            lib_for(y.storage).pp_lazy_materialize(y.ptr, y.ld, ctypes.byref(lz), tmp.data_ptr(), y.C, y.C, y.N, y.H * y.W, stream_ptr())
            m = tmp > 0
        else:
            m = y.torch() > 0
        return m.permute(0, 3, 1, 2)

    # ------------------------------------------------------------------ public: the composite step
    def forward_step(self, batch, mode, step, need_grad: bool):
        """Forward of ConsistencyRegulr (consistency_reglur_memory.py:24-102).  Returns dict of tensors."""
        args = self.args
        image = self._check_input(batch['image'], 'image')
        scribble = self._check_input(batch['scribble'], 'scribble')
        B, Cin, H, W = image.shape
        K = self.backbone.num_classes
        if scribble.shape != (B, K + 1, H, W):
            raise ValueError(f'scribble must be (B,{K + 1},H,W) one-hot, got {tuple(scribble.shape)}')
        train = mode == 'train'
        do_ent = bool(train and args.do_loss_ent)
        do_cr = bool(train and args.do_decoder_consistency)
        do_aux = bool(train and args.do_aux_path)
        do_mem = bool(do_aux and args.do_memory)
        variant = 0
        if do_cr:
            if args.loss_cr_variants not in CR_VARIANTS:
                raise ValueError('The loss is not implemented.')
            variant = CR_VARIANTS[args.loss_cr_variants]
        G = 2 if do_cr else 1
        self._frozen = self._frozen_stages()
        plan = self.plan_for(B, H, W, G, trainable=need_grad)
        self.last_plan = plan
        if do_aux and plan.aux is None:
            raise RuntimeError(plan.aux_error or 'model was built without an auxiliary path')
        st = stream_ptr()
        bn_training = self.backbone.training
        dev = image.device

        # --cr_teacher ema: the weak view's side of the consistency term is the averaged weights' prediction.  Its pass runs in
        # FRONT of the student's, so the per-layer records the student's forward leaves (L.x / L.y, the coefficient rows in flight)
        # are those of the student, as without a teacher.
        do_teacher = bool(do_cr and self.teacher is not None)
        logits_t = None
        unc_mask = None                  # --cr_uncertainty: (B,1,H,W) mask of the teacher call, a buffer of the teacher plan
        if do_teacher:
            unc_args = None
            if self.unc is not None:
                from .utils.uncertainty import uncertainty_threshold
                vm = batch.get('valid_mask')
                unc_args = (uncertainty_threshold(step or 0, self.unc['start'], K, getattr(args, 'ramp_up_scale', 5.0)),
                            self._check_input(vm, 'valid_mask') if vm is not None else None)
            with prof_range('forward: teacher (EMA weights, weak view)'):
                logits_t = self._teacher_forward(plan, image, st, unc_args)
            if unc_args is not None:
                unc_mask = plan.teacher_plan.unc['mask']
        plan.begin_forward((bool(bn_training), bool(self.aux.training) if self.aux is not None else False, self._frozen))
        self._rec = {} if need_grad else None
        with prof_range('pack weights + images'):
            self._pack_weights(plan, st, need_grad=need_grad)
            plan.K.pp_pack_image_nchw_to_nhwc(image.data_ptr(), B, Cin, H, W, plan.x0.ptr, plan.x0.ld, plan.x0.C, st)
            if do_cr:
                strong = self._check_input(batch['image_strong'], 'image_strong')
                x1 = _batch(plan.x0, B, B)
                plan.K.pp_pack_image_nchw_to_nhwc(strong.data_ptr(), B, Cin, H, W, x1.ptr, x1.ld, x1.C, st)
        logits = torch.empty((plan.Bt, K, H, W), device=dev, dtype=torch.float32)
        # class map of the scribbles: the target of the weak and of the auxiliary partial CE (enqueued first: both streams read it)
        plan.K.pp_argmax_channels(scribble.data_ptr(), B, K + 1, H * W, plan.target.data_ptr(), st)
        aux_group = 1 if do_cr else 0      # the aliased end_points dict holds the LAST backbone pass
        A = {}                             # what the auxiliary forward leaves for the rest of this function

        def aux_forward(sa, main_stream=None):
            """The auxiliary head up to its loss sums (aux_path_memory.py:46-66) and the bank update (:68-120), on stream `sa`.  It
            runs before the loss sums are reduced over the ranks, so that ONE all-reduce carries the denominators of all four
            pixel losses (SURVEY.md 8(e) coupling B)."""
            ax, a, LA = self.aux, plan.aux, self.aux_layer
            ain = self._aux_input(plan, aux_group, sa)
            drop = None
            if ax.aux_drop_prob > 0 and ax.training:
                # nn.Dropout2d in front of the bottleneck conv, of the classifier and (through fc_cls) of the memory
                # bank: per-(sample, channel) keep masks scaled by 1/(1-p), drawn from torch's CUDA generator like
                # F.dropout2d does, and kept for the backward pass
                keep = 1.0 - ax.aux_drop_prob

                def mask(n, c):
                    m = torch.empty((n, c), device=dev, dtype=torch.float32).bernoulli_(keep).div_(keep)
                    if main_stream is not None:      # drawn on the second stream, read by the backward pass on the main one
                        m.record_stream(main_stream)
                    return m
                drop = {'input': mask(B, ain.C), 'features': mask(B, LA.cout)}
                if do_mem:
                    drop['bank'] = mask(K, ax.hid_ch)
                din = a['drop_in']
                plan.K.pp_channel_scale(ain.ptr, ain.ld, din.ptr, din.ld, drop['input'].data_ptr(), ain.C, B,
                                     a['h'] * a['w'], 0, sa)
                ain = din
            self.last_drop_masks = drop
            self._convbn_fwd(plan, LA, ain, a['feat'], 1, self.aux.training, sa)
            feat = a['feat']
            ffc = feat                       # what the classifier reads
            if drop is not None:
                ffc = a['drop_feat']
                plan.K.pp_channel_scale(feat.ptr, feat.ld, ffc.ptr, ffc.ld, drop['features'].data_ptr(), feat.C, B,
                                     a['h'] * a['w'], 0, sa)
            wfc = ax.fc_cls[1].weight
            plan.K.pp_conv1x1_nhwc_to_nchw_fwd(ffc.ptr, ffc.ld, ffc.C, wfc.data_ptr(), None, a['lo'].data_ptr(), K, B,
                                            a['h'] * a['w'], sa)
            plan.K.pp_aux_pce_fwd(a['lo'].data_ptr(), B, K, a['h'], a['w'], H, W, plan.target.data_ptr(),
                               args.ignored_index, A['logits_aux'].data_ptr(), a['sums'].data_ptr(), *plan.ws_args(), sa)
            if do_mem and self.rank == 0:
                # only batch sample 0 of the (global) batch updates the bank: aux_path_memory.py:116
                plan.K.pp_memory_update(feat.ptr, feat.ld, feat.C, a['h'], a['w'], scribble.data_ptr(), K, H, W,
                                     ax.memory_bank.data_ptr(), float(ax.current_momentum(step)),
                                     1 if ax.ensemble_mode == 'cosine_similarity' else 0, *plan.ws_args(), sa)
            A.update(drop=drop, feat=feat, wfc=wfc)

        # Round 5: the auxiliary forward on the SECOND stream, forked when the encoder is enqueued (it reads stages 5 / 6) and
        # joined behind the segmentation losses: ~0.4 ms of small, latency-bound launches beside the decoder's forward pass.
        # Own workspace and statistics rows (plan.res); same kernels on the same data: bit-identical to the in-line order.
        side = self._side_stream(plan) if (AUX_SIDE and do_aux and need_grad and plan.bn_stats_side is not None
                                           and not self._sync(True)) else None
        if do_aux:
            A['logits_aux'] = torch.empty((B, K, H, W), device=dev, dtype=torch.float32)

        def fork_aux():
            main = torch.cuda.current_stream()
            plan.aux_fork.record(main)
            side.wait_event(plan.aux_fork)
            plan.res = (plan.ws_wg, plan.wg_ws_bytes, plan.bn_stats_side, plan.bn_stats_side_bytes)
            try:
                with torch.cuda.stream(side):
                    aux_forward(side.cuda_stream, main)
            finally:
                plan.res = None
            plan.aux_join.record(side)
        with prof_range('forward: weak | strong pass' if do_cr else 'forward: weak pass'):
            self._unet_forward(plan, bn_training, st, logits, after_encoder=fork_aux if side is not None else None)

        valid_mask = batch.get('valid_mask')
        if valid_mask is not None:
            valid_mask = self._check_input(valid_mask, 'valid_mask')
        mask_ptr = valid_mask.data_ptr() if (valid_mask is not None and (do_ent or do_cr)) else None
        zs = logits[B:] if do_cr else None
        if do_teacher:
            # two calls of the same kernels, each sum with one writer: the student's weak logits give partial CE and entropy
            # (variant 0: the strong logits are not read), the teacher's logits against the student's strong logits give the
            # consistency sums (slots [4:6] of sums_teacher; its partial-CE slots are computed and ignored)
            plan.K.pp_seg_losses_fwd(logits.data_ptr(), None, plan.target.data_ptr(), mask_ptr,
                                  B, K, H * W, args.ignored_index, int(do_ent), 0, plan.sums.data_ptr(),
                                  plan.ws.data_ptr(), plan.ws_bytes, st)
            plan.K.pp_seg_losses_fwd(logits_t.data_ptr(), zs.data_ptr(), plan.target.data_ptr(),
                                  unc_mask.data_ptr() if unc_mask is not None else mask_ptr,      # (the mask holds valid_mask already)
                                  B, K, H * W, args.ignored_index, 0, variant, plan.sums_teacher.data_ptr(),
                                  plan.ws.data_ptr(), plan.ws_bytes, st)
        else:
            plan.K.pp_seg_losses_fwd(logits.data_ptr(), zs.data_ptr() if do_cr else None, plan.target.data_ptr(), mask_ptr,
                                  B, K, H * W, args.ignored_index, int(do_ent), variant, plan.sums.data_ptr(),
                                  plan.ws.data_ptr(), plan.ws_bytes, st)
        regs = plan.regs if train else {}
        reg_mptr = valid_mask.data_ptr() if valid_mask is not None else None      # whenever the batch has one, entropy / consistency on or off
        for op in regs.values():
            op.fwd(logits.data_ptr(), image.data_ptr(), reg_mptr, B, K, Cin, H, W, need_grad, st)
        if do_aux:
            if side is not None:
                torch.cuda.current_stream().wait_event(plan.aux_join)
            else:
                aux_forward(st)
            ax, a = self.aux, plan.aux
            drop, feat, wfc, logits_aux = A['drop'], A['feat'], A['wfc'], A['logits_aux']
        if self.comm is not None and do_teacher:
            self.comm.allreduce_sums(plan.sums_store)      # every pair of the step and the teacher call's six sums: one collective
        elif self.comm is not None:
            self.comm.allreduce_sums(plan.all_sums if do_aux else (plan.all_sums[:6 + 2 * len(regs)] if regs else plan.sums))
        out = {}
        loss_pce = torch.empty((), device=dev, dtype=torch.float32)
        loss_ent = torch.empty((), device=dev, dtype=torch.float32) if do_ent else None
        loss_cr = torch.empty((), device=dev, dtype=torch.float32) if do_cr else None
        plan.K.pp_losses_finalize(plan.sums.data_ptr(), 1 if mask_ptr else 0, loss_pce.data_ptr(),
                               loss_ent.data_ptr() if do_ent else None, loss_cr.data_ptr() if (do_cr and not do_teacher) else None, st)
        if do_teacher:
            plan.K.pp_losses_finalize(plan.sums_teacher.data_ptr(), 1 if (mask_ptr or unc_mask is not None) else 0, None, None,
                                   loss_cr.data_ptr(), st)
        out['segmentation/logits'] = logits[:B]
        out['loss_pce'] = loss_pce
        if do_ent:
            out['loss_ent'] = loss_ent
        if do_cr:
            out['loss_cr'] = loss_cr
            out['segmentation/logits_strong'] = logits[B:]
            if do_teacher:
                out['segmentation/logits_teacher'] = logits_t
                if unc_mask is not None:
                    out['segmentation/uncertainty_mask'] = unc_mask.view(B, 1, H, W)      # (a fresh tensor object per step over the plan's buffer)
        for op in regs.values():     # the ratio of each pair, summed over the ranks by now
            out[op.reg.key] = torch.empty((), device=dev, dtype=torch.float32)
            op.finalize(out[op.reg.key].data_ptr(), reg_mptr is not None, st)

        if do_aux:
            loss_aux = torch.empty((), device=dev, dtype=torch.float32)
            plan.K.pp_losses_finalize(a['sums'].data_ptr(), 0, loss_aux.data_ptr(), None, None, st)
            out['logits_aux_cls'] = logits_aux
            out['loss_aux_cls'] = loss_aux
            if do_mem:
                bank = ax.memory_bank          # (updated by rank 0 inside aux_forward)
                if self.comm is not None:
                    self.comm.broadcast_bank(bank)
                loss_mem = torch.empty((), device=dev, dtype=torch.float32)
                bank_fc = bank
                if drop is not None:             # fc_cls(memory_bank) passes through fc_cls's Dropout2d too (aux_path_memory.py:61)
                    bank_fc = a['drop_bank']
                    plan.K.pp_channel_scale(bank.data_ptr(), ax.hid_ch, bank_fc.data_ptr(), ax.hid_ch,
                                         drop['bank'].data_ptr(), ax.hid_ch, K, 1, 0, st)
                plan.K.pp_memory_ce_fwd(bank_fc.data_ptr(), wfc.data_ptr(), K, ax.hid_ch, loss_mem.data_ptr(), st)
                out['loss_memory'] = loss_mem
        if need_grad:
            self.last = dict(rec=self._rec, gen=plan.generation, plan=plan, B=B, H=H, W=W, K=K, logits=logits, mask=valid_mask if mask_ptr else None,
                             do_ent=do_ent, do_cr=do_cr, do_aux=do_aux, do_mem=do_mem, variant=variant,
                             bn_training=bn_training, aux_training=self.aux.training if self.aux is not None else False,
                             aux_group=aux_group, logits_aux=out.get('logits_aux_cls'), frozen=self._frozen,
                             drop=self.last_drop_masks if do_aux else None, regs=tuple(regs), reg_mask=reg_mptr is not None)
            if do_teacher:
                self.last.update(teacher=plan.teacher_plan, logits_teacher=logits_t, teacher_mask=unc_mask)
        return out

    def _aux_input(self, plan, aux_group, st) -> View:
        a = plan.aux
        B = plan.B
        if a['alias_cat5']:
            return _batch(plan.cat[5], aux_group * B, B)
        c0 = 0
        for s in a['stages']:
            src = _batch(plan.enc_out[s], aux_group * B, B)
            dst = _sub(a['in'], c0, src.C)
            plan.K.pp_copy_slab(src.ptr, src.ld, dst.ptr, dst.ld, src.C, B * src.H * src.W, 0, st)
            c0 += src.C
        return a['in']

    def backward_step(self, g: Dict[str, Optional[torch.Tensor]], grads: Dict[torch.nn.Parameter, torch.Tensor],
                      state: Optional[dict] = None):
        """Backward of the composite step.  g: upstream gradient (0-dim device tensor) per loss name;
        grads: destination tensor per parameter (views of the flat gradient slab); state: the record of the forward
        being differentiated (the autograd node keeps it; default: the most recent forward)."""
        S = state if state is not None else self.last
        if S is None or S.get('unet'):
            raise RuntimeError('backward_step called without a recorded forward_step')
        if S is self.last:
            self.last = None
        plan: _Plan = S['plan']
        if plan.generation != S['gen']:
            raise RuntimeError('backward_step: another forward ran through the same buffers after the forward being '
                               'differentiated (its activations are gone); call backward before the next forward')
        self._bwd_rec = S['rec']
        self._rec = None
        self._bwd_plan = plan
        if getattr(plan, 'wg_pending', None) is not None:
            plan.wg_pending[0] = plan.wg_pending[1] = False
            plan.dz_slot = 0
        st = stream_ptr()
        B = S['B']
        logits = S['logits']

        def gp(name):
            if name in gp_done:
                return gp_done[name]
            t = g.get(name)
            if t is None:
                gp_done[name] = None
                return None
            if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                t = t.to(device=logits.device, dtype=torch.float32).reshape(())
            keep.append(t)
            gp_done[name] = t.data_ptr()
            return gp_done[name]
        keep: List[torch.Tensor] = []
        gp_done: Dict[str, Optional[int]] = {}
        mask = S['mask']
        zs_ptr = logits[B:].data_ptr() if S['do_cr'] else None
        dzs_ptr = plan.dlogits[B:].data_ptr() if S['do_cr'] else None
        # Round 5: the head of the auxiliary backward (it needs the loss gradients only) on the second stream, beside the 1x1 head and
        # the first decoder stages of the main chain; the main stream waits for it in front of the auxiliary convolution's backward
        aux_side = None
        if S['do_aux']:
            aux_side = self._side_stream(plan) if (AUX_SIDE and getattr(plan, 'bn_stats_side', None) is not None) else None
            for nm in ('loss_aux_cls', 'loss_memory'):
                gp(nm)                                   # (upstream gradients on the device before the fork)
            if aux_side is not None:
                main = torch.cuda.current_stream()
                plan.aux_fork.record(main)
                aux_side.wait_event(plan.aux_fork)
                plan.res = (plan.ws_wg, plan.wg_ws_bytes, plan.bn_stats_side, plan.bn_stats_side_bytes)
                try:
                    with torch.cuda.stream(aux_side):
                        self._aux_backward_head(plan, S, gp, grads, aux_side.cuda_stream)
                finally:
                    plan.res = None
                plan.aux_join.record(aux_side)
        with self._wgrad_budget(plan):
            self._backward_step_body(plan, S, grads, gp, aux_side, mask, zs_ptr, dzs_ptr, st)
        self._join_side_stream(plan)
        del keep

    def _backward_step_body(self, plan, S, grads, gp, aux_side, mask, zs_ptr, dzs_ptr, st):
        args = self.args
        B, H, W, K = S['B'], S['H'], S['W'], S['K']
        logits = S['logits']
        with prof_range('backward: losses'):
            tp = S.get('teacher')
            mptr = mask.data_ptr() if mask is not None else None
            if tp is not None:
                # the student call (variant 0) writes dlogits[:B] and leaves the strong half alone: both kernels store dzs under
                # `if (variant)` only (pp_loss.hip, seg_losses_bwd_kernel / seg_losses_bwd_v4_kernel).  The teacher call -- upstream
                # partial-CE gradient a device zero, no entropy, weak side detached -- writes the strong half, and its gradient wrt
                # the teacher logits into a buffer nobody reads.
                plan.K.pp_seg_losses_bwd(logits.data_ptr(), None, plan.target.data_ptr(), mptr, B, K, H * W, args.ignored_index,
                                      int(S['do_ent']), 0, 1, plan.sums.data_ptr(), gp('loss_pce'), gp('loss_ent'), None,
                                      plan.loss_scale, plan.dlogits.data_ptr(), None, st)
                tm = S.get('teacher_mask')      # --cr_uncertainty: the buffer the forward's teacher call read
                plan.K.pp_seg_losses_bwd(S['logits_teacher'].data_ptr(), zs_ptr, plan.target.data_ptr(),
                                      tm.data_ptr() if tm is not None else mptr, B, K, H * W,
                                      args.ignored_index, 0, S['variant'], 1, plan.sums_teacher.data_ptr(), tp.zero.data_ptr(), None,
                                      gp('loss_cr'), plan.loss_scale, tp.dlogits_discard.data_ptr(), dzs_ptr, st)
            else:
                plan.K.pp_seg_losses_bwd(logits.data_ptr(), zs_ptr, plan.target.data_ptr(), mptr,
                                      B, K, H * W, args.ignored_index, int(S['do_ent']), S['variant'],
                                      1 if getattr(args, 'detach_weak_cr', False) else 0, plan.sums.data_ptr(),
                                      gp('loss_pce'), gp('loss_ent'), gp('loss_cr'), plan.loss_scale, plan.dlogits.data_ptr(), dzs_ptr, st)
            for name in S['regs']:       # streaming adds of the unit gradients the forward left, behind the kernel that WRITES dlogits[:B]
                op = plan.regs[name]
                if gp(op.reg.key) is not None:
                    op.bwd(gp(op.reg.key), S['reg_mask'], plan.loss_scale, plan.dlogits.data_ptr(), B * K * H * W, st)
        with prof_range('backward: decoder'):
            g6 = self._unet_backward_decoder(plan, S['bn_training'], grads, st, need_g6=S['frozen'] < 6)
        if S['do_aux']:
            with prof_range('backward: aux path'):
                if aux_side is not None:
                    torch.cuda.current_stream().wait_event(plan.aux_join)
                else:
                    self._aux_backward_head(plan, S, gp, grads, st)
                self._aux_backward_conv(plan, S, grads, st)
                self._bucket('aux')
        with prof_range('backward: encoder'):
            self._unet_backward_encoder(plan, S['bn_training'], grads, g6, st, S['frozen'])

    def _aux_backward_head(self, plan, S, gp, grads, st):
        """The part of the auxiliary backward that depends on the loss gradients only: partial CE -> classifier (its weight
        gradient, d features) and the bank CE.  `st` may be the second stream (plan.res then names its workspace)."""
        ax, a = self.aux, plan.aux
        B, H, W, K = S['B'], S['H'], S['W'], S['K']
        wfc = ax.fc_cls[1].weight
        gw = grads[wfc]
        plan.K.pp_aux_pce_bwd(S['logits_aux'].data_ptr(), plan.target.data_ptr(), self.args.ignored_index, gp('loss_aux_cls'), plan.loss_scale,
                           a['sums'].data_ptr(), a['dlo'].data_ptr(), B, K, a['h'], a['w'], H, W, st)
        feat, dfeat = a['feat'], a['dfeat']
        drop = S['drop']
        ffc, dffc = (a['drop_feat'], a['drop_dfeat']) if drop is not None else (feat, dfeat)
        plan.K.pp_conv1x1_nchw_to_nhwc_bwd(a['dlo'].data_ptr(), ffc.ptr, ffc.ld, ffc.C, wfc.data_ptr(), dffc.ptr,
                                        dffc.ld, gw.data_ptr(), None, K, B, a['h'] * a['w'], 0, 0, *plan.ws_args(), st)
        if drop is not None:
            plan.K.pp_channel_scale(dffc.ptr, dffc.ld, dfeat.ptr, dfeat.ld, drop['features'].data_ptr(), feat.C, B,
                                 a['h'] * a['w'], 0, st)
        if S['do_mem']:
            bank_fc = a['drop_bank'] if drop is not None else ax.memory_bank
            plan.K.pp_memory_ce_bwd(bank_fc.data_ptr(), wfc.data_ptr(), K, ax.hid_ch, gp('loss_memory'),
                                 plan.loss_scale / self.world, gw.data_ptr(), 1, st)

    def _aux_backward_conv(self, plan, S, grads, st):
        """Bottleneck convolution + BatchNorm of the auxiliary path backwards, its data gradient added to the stage-5 / 6 gradients
        (behind the decoder's backward pass, which writes them first)."""
        ax, a, LA = self.aux, plan.aux, self.aux_layer
        B = S['B']
        feat, dfeat = a['feat'], a['dfeat']
        drop = S['drop']
        grp = S['aux_group']

        # freeze_encoder: the data gradient into a frozen stage's feature has no reader.  With every gathered stage frozen the
        # bottleneck convolution gets no data gradient at all (its own parameters still train); else the launch writes all of its
        # input channels and only the live stages' slices are added to their gradients
        live = [s > S['frozen'] for s in a['stages']]

        def scatter(din: View):
            """din (B,h,w,Cin) += into the gradient slices of the stages the auxiliary input was gathered from."""
            c0 = 0
            for s, on in zip(a['stages'], live):
                dst = _batch(self._enc_grad_view(plan, s, None) if s != 6 else self._stage6_grad(plan), grp * B, B)
                src = _sub(din, c0, dst.C)
                if on:
                    plan.K.pp_copy_slab(src.ptr, src.ld, dst.ptr, dst.ld, dst.C, B * dst.H * dst.W, 1, st)
                c0 += dst.C
        if not any(live):
            self._convbn_bwd(plan, LA, dfeat, None, False, S['aux_training'], grads, st)
        elif drop is not None:
            ddin = a['drop_din']
            self._convbn_bwd(plan, LA, dfeat, ddin, False, S['aux_training'], grads, st)
            if a['alias_cat5']:
                dx = _batch(plan.dcat[5], grp * B, B)
                plan.K.pp_channel_scale(ddin.ptr, ddin.ld, dx.ptr, dx.ld, drop['input'].data_ptr(), ddin.C, B,
                                     a['h'] * a['w'], 1, st)
            else:
                plan.K.pp_channel_scale(ddin.ptr, ddin.ld, a['din'].ptr, a['din'].ld, drop['input'].data_ptr(), ddin.C, B,
                                     a['h'] * a['w'], 0, st)
                scatter(a['din'])
        elif a['alias_cat5']:
            dx = _batch(plan.dcat[5], grp * B, B)
            self._convbn_bwd(plan, LA, dfeat, dx, True, S['aux_training'], grads, st)
        else:
            self._convbn_bwd(plan, LA, dfeat, a['din'], False, S['aux_training'], grads, st)
            scatter(a['din'])

    def unscale_grads(self, state, segments, flat=None) -> None:
        """After the backward of `state` (and, data-parallel, after its all-reduce): divide the gradient-slab segments the step
        wrote by the plan's static loss scale (16-bit storage; a power of two, so exact).  A no-op for fp32 plans.  With the
        FlatSlab given, the same pass raises its overflow flag when a gradient is not finite (a static scale can overflow
        fp16 in a bad step) and the fused optimizers then skip the update, as torch.cuda.amp.GradScaler.step would."""
        plan = state['plan']
        if plan.loss_scale == 1.0:
            if flat is not None:
                flat.guard_on = False
            return
        if flat is not None:
            flat.guard[0:1].zero_()
            flat.guard_on = True
        for t in segments:
            if flat is not None:
                lib.pp_scale_guard(t.data_ptr(), t.numel(), 1.0 / plan.loss_scale, flat.guard.data_ptr(), stream_ptr())
            else:
                lib.pp_scale(t.data_ptr(), t.numel(), 1.0 / plan.loss_scale, stream_ptr())

    def set_loss_scale(self, scale: float) -> float:
        """Change the static loss scale of the 16-bit storage mode (train.py halves it when an epoch's updates were mostly
        skipped by the overflow guard): the engine's value for plans still to be built, and every existing 16-bit plan."""
        self.loss_scale = float(scale)
        for p in self.plans.values():
            if p.h16:
                p.loss_scale = self.loss_scale
        return self.loss_scale

    def _stage6_grad(self, plan):
        d = self.backbone.dec_blocks()[5]
        return plan.g_low[5] if not d.identity_up else _sub(plan.dcat[5], 0, d.up_ch)

