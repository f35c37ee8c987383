"""Census of the convolution launches of real steps, each replayed against a float64 reference.

The per-kernel parity tests use hand-picked case lists; which kernel a layer gets is a function of its shape (convop.select).
Here every convolution-family launch of real full-width steps is recorded -- the engine's entry-point table (plan.K) is wrapped in a
recording proxy -- and every distinct launch (entry point, storage kind, every non-pointer argument, which optional pointers were
null, the ld / groups of a lazy input) is replayed on seeded random operands with the recorded ld's and flags and canaries in the
padding columns:
  * fp32 storage: against conv2d / conv_transpose2d / their gradients in float64 (outputs, data and weight gradients 1e-4,
    BatchNorm partial sums 1e-5); lazy-input forms against the lazy tensor evaluated in float64 and, bit for bit, against the
    ordinary entry point fed the materialised tensor (the harness of test_direct_convolution_with_lazy_input); the first layer's
    folded weight gradient through the harness of test_first_layer_bn_backward_with_folded_weight_gradient.
  * 16-bit storage: the _h16 / _bf16 entry against its fp32 twin on operands representable in the 16-bit type (check_act's bound,
    with the output's own magnitude as the intermediate a kernel may store in 16 bits first; fp32 results such as weight gradients
    at 1e-4), and that fp32 twin against float64 at the same shape.
A recorded launch without a replay adapter fails the census by name.  Outside the census: the stand-alone AuxPath.forward (it calls
the library directly, not through a plan) and --precision fp16 (fp16-grade by design, tested on its own).
"""
import ctypes
import math
import zlib
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4            # outputs, data and weight gradients (max-norm relative to the reference)
TOL_SUMS = 1e-5       # BatchNorm partial sums (test_conv_bn_fused_epilogues)
ATOL_SUM = 4e-6       # check_act (tests/test_gpu_h16.py): fp32 summation-order noise, relative to the largest output
G_FP32, G_16 = 1e-7, 1e-2      # gradient operand scale: far below fp16's normal range (fp32 storage), inside it (16-bit storage)
MANT = {'fp16': (10, -14, torch.float16), 'bf16': (7, -126, torch.bfloat16)}


def _dev():
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------------------------ recording
def _is_conv_launch(name):
    from pacingpseudo_amd._lib import _PROTOS
    family = name.startswith(('pp_conv3x3_', 'pp_conv1x1_', 'pp_convtranspose_')) or (
        name.startswith('pp_bn_lrelu_bwd') and name.endswith('_wgrad_c1'))
    args = _PROTOS.get(name, (None, []))[1]
    return family and bool(args) and args[-1] is ctypes.c_void_p          # a launch takes a stream; shape queries do not


@pytest.fixture(scope='module')
def census():
    """{(storage, entry, launch shape): set of configuration labels}: the convolution family of the shared recording
    (tests/_launch_census.py runs the configurations once per process)."""
    from tests._launch_census import record
    return {key: cfgs for key, cfgs in record().items() if _is_conv_launch(key[1])}


# ------------------------------------------------------------------------------------------------------------------ operands
class _Ops:
    """Seeded operands of one replay; activation-type tensors are rounded to the key's storage type (identical for the 16-bit
    entry and its fp32 twin)."""

    def __init__(self, key):
        self.storage = key[0]
        self.g = torch.Generator().manual_seed(zlib.crc32(repr(key[1:]).encode()))
        self.gs = G_FP32 if self.storage == 'fp32' else G_16

    def r(self, t):
        return t if self.storage == 'fp32' else t.to(MANT[self.storage][2]).float()

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def act(self, B, H, W, ld, C, scale=1.0, fill=5.0):
        """NHWC operand of row length ld: C random channels, `fill` in the columns the call must not read."""
        t = torch.full((B, H, W, ld), fill)
        t[..., :C] = self.r(self.randn(B, H, W, C, scale=scale))
        return t

    def lazy(self, lz, C):
        """Coefficient rows (groups, 3, ld) of a lazy input: scale (some negative), shift, slope 0.01 (tests/test_gpu_round4.py)."""
        _, ld, groups = lz
        coef = torch.zeros(groups, 3, ld)
        coef[:, 0], coef[:, 2] = 1.0, 1.0
        coef[:, 0, :C] = self.randn(groups, C) * 0.7 + 0.3
        coef[:, 1, :C] = self.randn(groups, C) * 0.5
        coef[:, 2, :C] = 0.01
        return coef


def _lazy64(z, coef, groups, C):
    """y = lrelu(z * scale + shift) per statistics group (images split evenly), float64, NHWC -> NHWC (first C channels)."""
    z = z[..., :C].double()
    per = z.shape[0] // groups
    ys = []
    for gi in range(groups):
        pre = z[gi * per:(gi + 1) * per] * coef[gi, 0, :C].double() + coef[gi, 1, :C].double()
        ys.append(torch.where(pre > 0, pre, pre * coef[gi, 2, :C].double()))
    return torch.cat(ys)


def _n64(t, C):
    """NHWC (first C channels) -> NCHW float64 on the device (the references run in float64 on the GPU)."""
    return t[..., :C].permute(0, 3, 1, 2).double().to(_dev())


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


class _Run:
    """One execution of a launch: K = entry-point table, dt = activation dtype; collects (label, device result, fp64 reference,
    tolerance, is-activation) and canary verdicts."""

    def __init__(self, K, dt, want_ref):
        from pacingpseudo_amd._lib import stream_ptr
        self.K, self.dt, self.want_ref, self.st = K, dt, want_ref, stream_ptr()
        self.res, self.keep = [], []

    def d(self, t, act=True):
        x = t.to(_dev()).to(self.dt if act else torch.float32).contiguous()
        self.keep.append(x)
        return x

    def out(self, B, H, W, ld, C, prior=None, fill=7.0):
        t = torch.full((B, H, W, ld), fill)
        if prior is not None:
            t[..., :C] = prior
        return self.d(t)

    def check(self, label, got, ref, tol=TOL, act=True):
        self.res.append((label, got, ref if self.want_ref else None, tol, act and got.dtype != torch.float32))

    def canary(self, label, buf, C, fill=7.0):
        self.res.append((label + ' canary', None, bool((buf[..., C:] == fill).all()), None, False))


def _p(t):
    return None if t is None else t.data_ptr()


def _ws(n):
    return torch.empty(max(int(n), 1) + 64, dtype=torch.uint8, device=_dev())


def _amax(t):
    return t.float().abs().max().reshape(1).contiguous()


def _cudnn_off():
    return torch.backends.cudnn.flags(enabled=False)


# ---------------------------------------------------------------------------------------------------------------- adapters
def _pack_direct(w, O_, I, f16):
    from pacingpseudo_amd._lib import lib, stream_ptr
    wf, wb = torch.zeros(O_, 9, I, device=_dev()), torch.zeros(I, 9, O_, device=_dev())
    (lib.pp_pack_conv3x3_weights_f16x3 if f16 else lib.pp_pack_conv3x3_weights)(w.data_ptr(), O_, I, I, wf.data_ptr(), wb.data_ptr(),
                                                                                  stream_ptr())
    return wf, wb


def _pack_wino(w, O_, I, tile, f16):
    from pacingpseudo_amd._lib import lib, stream_ptr
    n = (tile + 2) ** 2
    uf, ub = torch.zeros(n, O_, I, device=_dev()), torch.zeros(n, I, O_, device=_dev())
    (lib.pp_wino_pack_weights_f16x3 if f16 else lib.pp_wino_pack_weights)(w.data_ptr(), O_, I, tile, uf.data_ptr(), ub.data_ptr(),
                                                                          stream_ptr())
    return uf, ub


def _conv_in(ops, lz, run, ld, C, B, H, W, scale=1.0):
    """The input of a launch: plain, or lazy (lz = ('lazy', ld, groups): raw z + coefficient rows): (device tensor, lazy struct or
    None, fp64 NCHW value the convolution sees, materialised-y tensor for the bit-identity check or None)."""
    x = ops.act(B, H, W, ld, C, scale)
    if lz is None:
        return run.d(x), None, _n64(x, C) if run.want_ref else None, None
    from pacingpseudo_amd._lib import PpLazyIn
    coef = ops.lazy(lz, C)
    cd = run.d(coef, act=False)
    st = PpLazyIn(cd.data_ptr(), lz[1], lz[2])
    run.keep.append(st)
    xd = run.d(x)
    y = torch.empty_like(xd)
    y.copy_(xd)
    run.K.pp_lazy_materialize(xd.data_ptr(), ld, ctypes.byref(st), y.data_ptr(), ld, C, B, H * W, run.st)
    run.keep.append(y)
    ref = _lazy64(x, coef, lz[2], C).permute(0, 3, 1, 2).to(_dev()) if run.want_ref else None
    return xd, st, ref, y


def _direct_fwd(key, run):
    """pp_conv3x3_fwd / pp_conv3x3_fwd_f16x3"""
    _, name, a = key
    f16 = name.endswith('_f16x3')
    _, ld_in, C, _, bias, _, ld_out, N, B, H, W, dil, acc = a[:13]
    ops = _Ops(key)
    x, _, x64, _ = _conv_in(ops, None, run, ld_in, C, B, H, W)
    w = ops.randn(N, C, 3, 3, scale=1 / math.sqrt(9 * C)).to(_dev())
    b = ops.randn(N).to(_dev())
    prior = ops.r(ops.randn(B, H, W, N)) if acc else None
    wf, _ = _pack_direct(w, N, C, f16)
    out = run.out(B, H, W, ld_out, N, prior)
    args = (x.data_ptr(), ld_in, C, wf.data_ptr(), _p(b) if bias else None, out.data_ptr(), ld_out, N, B, H, W, dil, acc)
    if f16:
        am = _amax(x[..., :C]) if a[13] else None
        run.K.pp_conv3x3_fwd_f16x3(*args, _p(am), run.st)
    else:
        run.K.pp_conv3x3_fwd(*args, run.st)
    ref = None
    if run.want_ref:
        with _cudnn_off():
            ref = F.conv2d(x64, w.double(), b.double() if bias else None, 1, dil, dil)
        if acc:
            ref = ref + _n64(prior, N)
    run.check('y', out[..., :N], _nhwc(ref) if ref is not None else None)
    run.canary('y', out, N)


def _wino_fwd(key, run):
    """pp_conv3x3_wino_fwd / pp_conv3x3_wino_fwd_f16x3 (unfused forward: GroupNorm blocks, forward-only plans)"""
    _, name, a = key
    f16 = name.endswith('_f16x3')
    _, ld_in, C, _, bias, _, ld_out, N, B, H, W, dil, acc, vkeep = a[:14]
    from pacingpseudo_amd._lib import lib
    ops = _Ops(key)
    x, _, x64, _ = _conv_in(ops, None, run, ld_in, C, B, H, W)
    w = ops.randn(N, C, 3, 3, scale=1 / math.sqrt(9 * C)).to(_dev())
    b = ops.randn(N).to(_dev())
    prior = ops.r(ops.randn(B, H, W, N)) if acc else None
    U, _ = _pack_wino(w, N, C, lib.pp_conv3x3_wino_tile(H, W, dil), f16)
    nws = lib.pp_conv3x3_wino_workspace(C, N, B, H, W, dil)
    ws = _ws(nws)
    vk = torch.empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil), device=_dev()) if vkeep else None
    out = run.out(B, H, W, ld_out, N, prior)
    (run.K.pp_conv3x3_wino_fwd_f16x3 if f16 else run.K.pp_conv3x3_wino_fwd)(
        x.data_ptr(), ld_in, C, U.data_ptr(), _p(b) if bias else None, out.data_ptr(), ld_out, N, B, H, W, dil, acc, _p(vk),
        ws.data_ptr(), nws, run.st)
    ref = None
    if run.want_ref:
        with _cudnn_off():
            ref = F.conv2d(x64, w.double(), b.double() if bias else None, 1, dil, dil)
        ref = _nhwc(ref + (_n64(prior, N) if acc else 0))
    run.check('y', out[..., :N], ref)
    run.canary('y', out, N)


def _bn_fwd(key, run):
    """pp_conv3x3_fwd_bn[_lazy] / pp_conv3x3_wino_fwd_bn: z + partial statistics (mode 1), y into a wider tensor (mode 2)."""
    _, name, a = key
    wino = 'wino' in name
    if wino:
        (_, ld_in, C, _, bias, _, ld_out, N, B, H, W, dil, f16, vkeep, _, _, mode, scale, shift, slope, groups) = a[:21]
    else:
        (_, ld_in, C, _, bias, _, ld_out, N, B, H, W, dil, f16, in_amax, mode, scale, shift, slope, groups) = a[:19]
    ops = _Ops(key)
    x, lz, x64, ymat = _conv_in(ops, a[-2] if name.endswith('_lazy') else None, run, ld_in, C, B, H, W)
    stats_ptr = a[21] if wino else a[19]
    w = ops.randn(N, C, 3, 3, scale=1 / math.sqrt(9 * C)).to(_dev())
    b = ops.randn(N).to(_dev())
    sc = (torch.rand(N, generator=ops.g) + 0.5).to(_dev())
    sh = ops.randn(N).to(_dev())
    from pacingpseudo_amd._lib import lib
    if wino:
        tile = lib.pp_conv3x3_wino_tile(H, W, dil)
        U, _ = _pack_wino(w, N, C, tile, f16)
        nws = lib.pp_conv3x3_wino_workspace(C, N, B, H, W, dil)
        ws = _ws(nws)
        vk = torch.empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil), device=_dev()) if vkeep else None
    else:
        U, _ = _pack_direct(w, N, C, f16)
        am = _amax(x[..., :C]) if in_amax else None
    nst = lib.pp_conv3x3_bn_stats_bytes(N, B, H, W, groups)
    rows = ctypes.c_int(0)
    results = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        out = run.out(B, H, W, ld_out, N)
        stats = torch.full((nst // 8 + 2,), float('nan'), dtype=torch.float64, device=_dev())
        sp = stats.data_ptr() if stats_ptr else None
        if wino:
            run.K.pp_conv3x3_wino_fwd_bn(src.data_ptr(), ld_in, C, U.data_ptr(), _p(b) if bias else None, out.data_ptr(), ld_out, N,
                                         B, H, W, dil, f16, _p(vk), ws.data_ptr(), nws, mode, _p(sc) if scale else None,
                                         _p(sh) if shift else None, slope, groups, sp, nst, ctypes.byref(rows), run.st)
        else:
            args = (src.data_ptr(), ld_in, C, U.data_ptr(), _p(b) if bias else None, out.data_ptr(), ld_out, N, B, H, W, dil, f16,
                    _p(am), mode, _p(sc) if scale else None, _p(sh) if shift else None, slope, groups, sp, nst,
                    ctypes.byref(rows))
            if lzs is not None:
                run.K.pp_conv3x3_fwd_bn_lazy(*args, ctypes.byref(lzs), run.st)
            else:
                run.K.pp_conv3x3_fwd_bn(*args, run.st)
        torch.cuda.synchronize()
        results.append((out, stats[:groups * rows.value * 2 * N].clone() if mode == 1 else None))
    out, stats = results[0]
    if lz is not None:      # lazy form == ordinary entry on the materialised tensor, element for element
        run.res.append(('lazy form bit-identical', None, torch.equal(out, results[1][0]) and (
            mode != 1 or torch.equal(stats, results[1][1])), None, False))
    ref = None
    if run.want_ref:
        with _cudnn_off():
            ref = F.conv2d(x64, w.double(), b.double() if bias else None, 1, dil, dil)
        if mode == 2:
            pre = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
            ref = torch.where(pre > 0, pre, pre * slope)
        ref = _nhwc(ref)
    run.check('z' if mode == 1 else 'y', out[..., :N], ref)
    run.canary('z' if mode == 1 else 'y', out, N)
    if mode == 1:
        r = rows.value
        part = stats.view(groups, r, 2, N)
        zc = out[..., :N].double().reshape(groups, -1, N)
        run.stats_mag = {'stats sum': zc.abs().sum(1), 'stats sum of squares': 2 * zc.pow(2).sum(1)}
        run.res.append(('stats sum', part[:, :, 0].sum(1), zc.sum(1), TOL_SUMS, False))
        run.res.append(('stats sum of squares', part[:, :, 1].sum(1), zc.pow(2).sum(1), TOL_SUMS, False))


def _bwd_data(key, run):
    """pp_conv3x3_bwd_data[_f16x3] / pp_conv3x3_wino_bwd_data[_f16x3]"""
    _, name, a = key
    wino, f16 = 'wino' in name, name.endswith('_f16x3')
    _, ld_dz, O_, _, _, ld_dx, I, B, H, W, dil, acc = a[:12]
    ops = _Ops(key)
    dz = run.d(ops.act(B, H, W, ld_dz, O_, ops.gs))
    w = ops.randn(O_, I, 3, 3, scale=1 / math.sqrt(9 * I)).to(_dev())
    prior = ops.r(ops.randn(B, H, W, I, scale=ops.gs)) if acc else None
    dx = run.out(B, H, W, ld_dx, I, prior)
    am = _amax(dz[..., :O_]) if (f16 and a[-2]) else None
    from pacingpseudo_amd._lib import lib
    if wino:
        _, Ub = _pack_wino(w, O_, I, lib.pp_conv3x3_wino_tile(H, W, dil), f16)
        nws = lib.pp_conv3x3_wino_workspace(O_, I, B, H, W, dil)
        ws = _ws(nws)
        args = (dz.data_ptr(), ld_dz, O_, Ub.data_ptr(), dx.data_ptr(), ld_dx, I, B, H, W, dil, acc, ws.data_ptr(), nws)
        if f16:
            run.K.pp_conv3x3_wino_bwd_data_f16x3(*args, _p(am), run.st)
        else:
            run.K.pp_conv3x3_wino_bwd_data(*args, run.st)
    else:
        _, wb = _pack_direct(w, O_, I, f16)
        args = (dz.data_ptr(), ld_dz, O_, wb.data_ptr(), dx.data_ptr(), ld_dx, I, B, H, W, dil, acc)
        if f16:
            run.K.pp_conv3x3_bwd_data_f16x3(*args, _p(am), run.st)
        else:
            run.K.pp_conv3x3_bwd_data(*args, run.st)
    ref = None
    if run.want_ref:
        with _cudnn_off():
            ref = torch.nn.grad.conv2d_input((B, I, H, W), w.double(), _n64(dz, O_), 1, dil, dil)
        if acc:
            ref = ref + _n64(prior, I)
        ref = _nhwc(ref)
    run.check('dx', dx[..., :I], ref)
    run.canary('dx', dx, I)


def _bwd_weight(key, run):
    """pp_conv3x3_bwd_weight[_f16x3[_lazy]] / pp_conv3x3_wino_bwd_weight[_f16x3] (kept V: made by the matching forward first)"""
    _, name, a = key
    wino, f16 = 'wino' in name, '_f16x3' in name
    from pacingpseudo_amd._lib import lib
    if wino:
        _, ld_dz, O_, _, ld_x, C, B, H, W, dil, _, acc, vcached = a[:13]
        Cpad, I = C, C
    else:
        _, ld_dz, O_, _, ld_x, Cpad, I, B, H, W, dil, _, acc = a[:13]
        vcached = None
    ops = _Ops(key)
    dz = run.d(ops.act(B, H, W, ld_dz, O_, ops.gs))
    x, lz, x64, ymat = _conv_in(ops, a[-2] if name.endswith('_lazy') else None, run, ld_x, Cpad, B, H, W)
    if Cpad > I:            # the padded input channels of the first layer hold zeros
        x[..., I:Cpad] = 0
        if x64 is not None:
            x64[:, I:] = 0
    prior = ops.randn(O_, I, 3, 3) * ops.gs if acc else None
    am = _amax(dz[..., :O_]) if (f16 and a[-3 if name.endswith('_lazy') else -2]) else None
    outs = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        dw = (prior.clone() if acc else torch.full((O_, I, 3, 3), 5.0)).to(_dev())
        if wino:
            nws = max(lib.pp_conv3x3_wino_bwd_weight_workspace(O_, C, B, H, W, dil), lib.pp_conv3x3_wino_workspace(C, O_, B, H, W, dil))
            ws = _ws(nws)
            vk = None
            if vcached:
                tile = lib.pp_conv3x3_wino_tile(H, W, dil)
                vk = torch.empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil), device=_dev())
                uf, _ = _pack_wino(ops.randn(O_, C, 3, 3).to(_dev()), O_, C, tile, f16)
                tmp = run.out(B, H, W, O_, O_)
                fwd = run.K.pp_conv3x3_wino_fwd_f16x3 if f16 else run.K.pp_conv3x3_wino_fwd
                fwd(src.data_ptr(), ld_x, C, uf.data_ptr(), None, tmp.data_ptr(), O_, O_, B, H, W, dil, 0, vk.data_ptr(), ws.data_ptr(),
                    nws, run.st)
            args = (dz.data_ptr(), ld_dz, O_, src.data_ptr(), ld_x, C, B, H, W, dil, dw.data_ptr(), acc, _p(vk), ws.data_ptr(), nws)
            if f16:
                run.K.pp_conv3x3_wino_bwd_weight_f16x3(*args, _p(am), run.st)
            else:
                run.K.pp_conv3x3_wino_bwd_weight(*args, run.st)
        else:
            nws = lib.pp_conv3x3_bwd_weight_workspace(O_, Cpad, B, H, W)
            ws = _ws(nws)
            args = (dz.data_ptr(), ld_dz, O_, src.data_ptr(), ld_x, Cpad, I, B, H, W, dil, dw.data_ptr(), acc, ws.data_ptr(), nws)
            if lzs is not None:
                run.K.pp_conv3x3_bwd_weight_f16x3_lazy(*args, _p(am), ctypes.byref(lzs), run.st)
            elif f16:
                run.K.pp_conv3x3_bwd_weight_f16x3(*args, _p(am), run.st)
            else:
                run.K.pp_conv3x3_bwd_weight(*args, run.st)
        torch.cuda.synchronize()
        outs.append(dw)
    if lz is not None:
        run.res.append(('lazy form bit-identical', None, torch.equal(outs[0], outs[1]), None, False))
    ref = None
    if run.want_ref:
        with _cudnn_off():
            ref = torch.nn.grad.conv2d_weight(x64[:, :I], (O_, I, 3, 3), _n64(dz, O_), 1, dil, dil)
        if acc:
            ref = ref + prior.double().to(_dev())
    run.check('dw', outs[0], ref, act=False)


def _conv1x1(key, run):
    """pp_conv1x1_nhwc_to_nchw_fwd[_lazy] / pp_conv1x1_nchw_to_nhwc_bwd[_lazy] (the 1x1 heads, NCHW fp32 logits).  With 16-bit
    storage the heads evaluate a lazy input in fp32 (no 16-bit rounding of y, unlike the 3x3 kernels, which stage y in 16 bits):
    there the lazy form is held to the fp32 twin's float64 reference instead of to the entry fed the stored y."""
    _, name, a = key
    ops = _Ops(key)
    from pacingpseudo_amd._lib import lib
    if 'fwd' in name:
        _, ld_x, C, _, bias, _, K_, N, HW = a[:9]
    else:
        _, _, ld_x, C, _, dxp, ld_dx, _, dbp, K_, N, HW, acc_dx, acc_p = a[:14]
    x, lz, x64, ymat = _conv_in(ops, a[-2] if name.endswith('_lazy') else None, run, ld_x, C, N, HW, 1)
    w = ops.randn(K_, C, scale=1 / math.sqrt(C)).to(_dev())
    y64 = x64.reshape(N, C, HW) if x64 is not None else None
    if 'fwd' in name:
        b = ops.randn(K_).to(_dev())
        outs = []
        for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
            lo = torch.full((N, K_, HW), 7.0, device=_dev())
            args = (src.data_ptr(), ld_x, C, w.data_ptr(), _p(b) if bias else None, lo.data_ptr(), K_, N, HW)
            if lzs is not None:
                run.K.pp_conv1x1_nhwc_to_nchw_fwd_lazy(*args, ctypes.byref(lzs), run.st)
            else:
                run.K.pp_conv1x1_nhwc_to_nchw_fwd(*args, run.st)
            torch.cuda.synchronize()
            outs.append(lo)
        if lz is not None and run.dt == torch.float32:
            run.res.append(('lazy form bit-identical', None, torch.equal(outs[0], outs[1]), None, False))
        ref = None
        if run.want_ref:
            ref = torch.einsum('kc,ncp->nkp', w.double(), y64) + (b.double().view(1, -1, 1) if bias else 0)
        run.check('logits', outs[0], ref, act=False)
        return
    dl = (ops.randn(N, K_, HW) * ops.gs).to(_dev())
    pdx = ops.r(ops.randn(N, 1, HW, C, scale=ops.gs)) if acc_dx else None
    pdw, pdb = ops.randn(K_, C) * ops.gs, ops.randn(K_) * ops.gs
    nws = lib.pp_conv1x1_bwd_workspace(K_, C, N, HW)
    ws = _ws(nws)
    outs = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        dx = run.out(N, 1, HW, ld_dx, C, pdx) if dxp else None
        dw = (pdw if acc_p else torch.full((K_, C), 5.0)).to(_dev())
        db = (pdb if acc_p else torch.full((K_,), 5.0)).to(_dev())
        args = (dl.data_ptr(), src.data_ptr(), ld_x, C, w.data_ptr(), _p(dx), ld_dx, dw.data_ptr(), _p(db) if dbp else None, K_, N,
                HW, acc_dx, acc_p, ws.data_ptr(), nws)
        if lzs is not None:
            run.K.pp_conv1x1_nchw_to_nhwc_bwd_lazy(*args, ctypes.byref(lzs), run.st)
        else:
            run.K.pp_conv1x1_nchw_to_nhwc_bwd(*args, run.st)
        torch.cuda.synchronize()
        outs.append((dx, dw, db))
    if lz is not None and run.dt == torch.float32:
        same = all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]) if p is not None)
        run.res.append(('lazy form bit-identical', None, same, None, False))
    dx, dw, db = outs[0]
    refs = [None, None, None]
    if run.want_ref:
        dl64 = dl.double()
        refs[0] = torch.einsum('kc,nkp->npc', w.double(), dl64).unsqueeze(1) + (_n64(pdx, C).permute(0, 2, 3, 1) if acc_dx else 0)
        refs[1] = torch.einsum('nkp,ncp->kc', dl64, y64) + (pdw.double().to(_dev()) if acc_p else 0)
        refs[2] = dl64.sum((0, 2)) + (pdb.double().to(_dev()) if acc_p else 0)
    if dx is not None:
        run.check('dx', dx[..., :C], refs[0])
        run.canary('dx', dx, C)
    run.check('dw', dw, refs[1], act=False)
    if dbp:
        run.check('dbias', db, refs[2], act=False)


def _convtranspose(key, run):
    """pp_convtranspose_fwd / _bwd_data / _bwd_weight (--is_trans_conv, fp32 storage only)"""
    _, name, a = key
    ops = _Ops(key)
    from pacingpseudo_amd._lib import lib
    if name == 'pp_convtranspose_fwd':
        _, ld_x, Cin, _, _, ld_out, Cout, k, N, H, W = a[:11]
    elif name == 'pp_convtranspose_bwd_data':
        _, ld_out, Cout, _, _, ld_x, Cin, k, N, H, W, acc = a[:12]
    else:
        _, ld_out, Cout, _, ld_x, Cin, k, N, H, W, _, acc = a[:12]
    w = ops.randn(Cin, Cout, k, k, scale=1 / math.sqrt(Cin)).to(_dev())
    if name == 'pp_convtranspose_fwd':
        x = run.d(ops.act(N, H, W, ld_x, Cin))
        out = run.out(N, k * H, k * W, ld_out, Cout)
        run.K.pp_convtranspose_fwd(x.data_ptr(), ld_x, Cin, w.data_ptr(), out.data_ptr(), ld_out, Cout, k, N, H, W, run.st)
        ref = None
        if run.want_ref:
            with _cudnn_off():
                ref = _nhwc(F.conv_transpose2d(_n64(x, Cin), w.double(), None, k))
        run.check('y', out[..., :Cout], ref)
        run.canary('y', out, Cout)
        return
    dout = run.d(ops.act(N, k * H, k * W, ld_out, Cout, ops.gs))
    if name == 'pp_convtranspose_bwd_data':
        prior = ops.randn(N, H, W, Cin, scale=ops.gs) if acc else None
        dx = run.out(N, H, W, ld_x, Cin, prior)
        run.K.pp_convtranspose_bwd_data(dout.data_ptr(), ld_out, Cout, w.data_ptr(), dx.data_ptr(), ld_x, Cin, k, N, H, W, acc, run.st)
        ref = None
        if run.want_ref:
            with _cudnn_off():
                ref = F.conv2d(_n64(dout, Cout), w.double(), None, k)
            ref = _nhwc(ref + (_n64(prior, Cin) if acc else 0))
        run.check('dx', dx[..., :Cin], ref)
        run.canary('dx', dx, Cin)
        return
    x = run.d(ops.act(N, H, W, ld_x, Cin))
    prior = ops.randn(Cin, Cout, k, k, scale=ops.gs) if acc else None
    dw = (prior.clone() if acc else torch.full((Cin, Cout, k, k), 5.0)).to(_dev())
    nws = lib.pp_convtranspose_bwd_weight_workspace(Cin, Cout, k, N, H, W)
    ws = _ws(nws)
    run.K.pp_convtranspose_bwd_weight(dout.data_ptr(), ld_out, Cout, x.data_ptr(), ld_x, Cin, k, N, H, W, dw.data_ptr(), acc,
                                      ws.data_ptr(), nws, run.st)
    ref = None
    if run.want_ref:
        with _cudnn_off():
            xr = _n64(x, Cin)
            wr = w.double().requires_grad_(True)
            F.conv_transpose2d(xr, wr, None, k).backward(_n64(dout, Cout))
        ref = wr.grad + (prior.double().to(_dev()) if acc else 0)
    run.check('dw', dw, ref, act=False)


def _wgrad_c1(key, run):
    """pp_bn_lrelu_bwd[_eval]_wgrad_c1 (first layer: BatchNorm + LeakyReLU backward with the weight gradient folded in).
    fp32 twin: the harness of test_first_layer_bn_backward_with_folded_weight_gradient at the recorded geometry.  16-bit entry:
    against that twin on identical representable operands and coefficient rows (its results are fp32)."""
    storage, name, a = key
    ev = 'eval' in name
    if ev:
        _, ld_dy, _, ld_z, _, _, _, _, ld_x, H, W, _, acc_dw, _, _, _, acc_p, C, P = a[:19]
        groups, training = 1, False
    else:
        _, ld_dy, _, ld_z, _, _, _, _, _, training, _, ld_x, H, W, _, acc_dw, _, _, _, acc_p, C, ppg, groups = a[:23]
        P = ppg * groups
    B = P // (groups * H * W)
    if run.dt == torch.float32:
        if run.want_ref:
            from tests.test_gpu_round5 import test_first_layer_bn_backward_with_folded_weight_gradient as harness
            harness(C, B, H, W, groups, bool(training), 'fp32')
            run.res.append(('fp32 harness (test_first_layer_bn_backward_with_folded_weight_gradient)', None, True, None, False))
        return
    from pacingpseudo_amd._lib import lib
    ops = _Ops(key)
    N = B * groups
    x = ops.act(N, H, W, ld_x, 1)
    w = ops.randn(C, 1, 3, 3) / 3
    z = ops.act(N, H, W, ld_z, 0)
    z[..., :C] = ops.r(_nhwc(F.conv2d(x[..., :1].permute(0, 3, 1, 2), w, None, 1, 1, 1)).float())
    dy = ops.act(N, H, W, ld_dy, C, ops.gs)
    gamma, beta = torch.rand(C, generator=ops.g) + 0.5, ops.randn(C)
    gamma[0] = -0.7
    rm, rv = ops.randn(C) * 0.1, torch.rand(C, generator=ops.g) + 0.5
    coef = torch.empty(4, groups, C, device=_dev())
    mean, invstd, scale, shift = (coef[i].data_ptr() for i in range(4))
    gd, bd, rmd, rvd = (t.to(_dev()) for t in (gamma, beta, rm, rv))
    nbt = torch.zeros((), dtype=torch.int64, device=_dev())
    nws = max(lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(C, P // groups, groups), lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(C, P, 1),
              lib.pp_bn_workspace(C, P // groups, groups))
    ws = _ws(nws)
    z32 = z.to(_dev())
    if training:
        lib.pp_bn_train_stats(z32.data_ptr(), ld_z, C, P // groups, groups, 1e-5, 0.1, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(),
                              rvd.data_ptr(), nbt.data_ptr(), mean, invstd, scale, shift, ws.data_ptr(), nws, run.st)
    else:
        lib.pp_bn_eval_coeffs(C, groups, 1e-5, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), mean, invstd, scale,
                              shift, run.st)
    if ev:          # the one-pass eval form reads the stored output y = lrelu(z * scale + shift)
        pre = z32[..., :C] * coef[2] + coef[3]
        zsrc = z32.clone()
        zsrc[..., :C] = ops.r(torch.where(pre > 0, pre, pre * 0.01).cpu()).to(_dev())
    else:
        zsrc = z32
    res = []
    pdw, pp = ops.randn(C, 1, 3, 3) * ops.gs, ops.randn(3, C) * ops.gs
    for K, dt in ((lib, torch.float32), (run.K, run.dt)):
        xd, zd, dyd = (t.to(_dev()).to(dt).contiguous() for t in (x, zsrc, dy))
        dw = (pdw if acc_dw else torch.full((C, 1, 3, 3), 5.0)).to(_dev())
        dg, db, dbc = ((pp[i] if acc_p else torch.full((C,), 9.0)).to(_dev()) for i in range(3))
        if ev:
            K.pp_bn_lrelu_bwd_eval_wgrad_c1(dyd.data_ptr(), ld_dy, zd.data_ptr(), ld_z, scale, gd.data_ptr(), bd.data_ptr(), xd.data_ptr(),
                                            ld_x, H, W, dw.data_ptr(), acc_dw, dg.data_ptr(), db.data_ptr(), dbc.data_ptr(), acc_p, C,
                                            P, 0.01, ws.data_ptr(), nws, run.st)
        else:
            K.pp_bn_lrelu_bwd_wgrad_c1(dyd.data_ptr(), ld_dy, zd.data_ptr(), ld_z, scale, shift, mean, invstd, gd.data_ptr(), training,
                                       xd.data_ptr(), ld_x, H, W, dw.data_ptr(), acc_dw, dg.data_ptr(), db.data_ptr(), dbc.data_ptr(),
                                       acc_p, C, ppg, groups, 0.01, ws.data_ptr(), nws, run.st)
        torch.cuda.synchronize()
        res.append((dw, dg, db, dbc))
    for label, h, f in zip(('dw', 'dgamma', 'dbeta', 'dbias'), res[1], res[0]):
        run.res.append((label + ' vs fp32 twin', h, f.double(), TOL, False))


ADAPTERS = {
    'pp_conv3x3_fwd': _direct_fwd, 'pp_conv3x3_fwd_f16x3': _direct_fwd,
    'pp_conv3x3_wino_fwd': _wino_fwd, 'pp_conv3x3_wino_fwd_f16x3': _wino_fwd,
    'pp_conv3x3_fwd_bn': _bn_fwd, 'pp_conv3x3_fwd_bn_lazy': _bn_fwd, 'pp_conv3x3_wino_fwd_bn': _bn_fwd,
    'pp_conv3x3_bwd_data': _bwd_data, 'pp_conv3x3_bwd_data_f16x3': _bwd_data,
    'pp_conv3x3_wino_bwd_data': _bwd_data, 'pp_conv3x3_wino_bwd_data_f16x3': _bwd_data,
    'pp_conv3x3_bwd_weight': _bwd_weight, 'pp_conv3x3_bwd_weight_f16x3': _bwd_weight, 'pp_conv3x3_bwd_weight_f16x3_lazy': _bwd_weight,
    'pp_conv3x3_wino_bwd_weight': _bwd_weight, 'pp_conv3x3_wino_bwd_weight_f16x3': _bwd_weight,
    'pp_conv1x1_nhwc_to_nchw_fwd': _conv1x1, 'pp_conv1x1_nhwc_to_nchw_fwd_lazy': _conv1x1,
    'pp_conv1x1_nchw_to_nhwc_bwd': _conv1x1, 'pp_conv1x1_nchw_to_nhwc_bwd_lazy': _conv1x1,
    'pp_convtranspose_fwd': _convtranspose, 'pp_convtranspose_bwd_data': _convtranspose, 'pp_convtranspose_bwd_weight': _convtranspose,
    'pp_bn_lrelu_bwd_wgrad_c1': _wgrad_c1, 'pp_bn_lrelu_bwd_eval_wgrad_c1': _wgrad_c1,
}


def _rel(got, ref):
    got, ref = got.double().to(ref.device), ref.double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _act_ratio(h, f, storage):
    """check_act (tests/test_gpu_h16.py) for 16-bit result h against the fp32 twin's f, as max(err / bound); the output's own
    magnitude is the intermediate (a kernel may store a partial sum or z in 16 bits before the output is formed)."""
    mant, emin, _ = MANT[storage]
    f64, h64 = f.double(), h.double()
    if not bool(torch.isfinite(h64).all()):
        return float('inf')
    m = max(float(f64.abs().max()), 1e-30)
    ulp = torch.pow(2.0, torch.floor(torch.log2(f64.abs().clamp_min(2.0 ** emin))) - mant)
    bound = 0.75 * ulp + ATOL_SUM * m + 2.0 ** -(mant + 1) * m
    return float(((h64 - f64).abs() / bound).max())


def replay(key, adapters=None, table=None):
    """[(label, error / tolerance)] of one recorded launch; raises KeyError naming an entry without an adapter.  adapters: another
    family's table of adapters (tests/test_gpu_stream_census.py); table: a stand-in for the fp32 entry-point table."""
    storage, name, a = key
    adapters = ADAPTERS if adapters is None else adapters
    if name not in adapters:
        raise KeyError(name)
    from pacingpseudo_amd._lib import lib, lib_for
    if table is not None:
        lib = table
    out = []
    r32 = _Run(lib, torch.float32, True)
    adapters[name]((storage, name, a), r32)
    torch.cuda.synchronize()
    for label, got, ref, tol, _ in r32.res:
        tag = 'fp32 twin ' if storage != 'fp32' else ''
        if got is None:
            out.append((tag + label, 0.0 if ref else float('inf')))
        else:
            out.append((tag + label, _rel(got, ref) / tol))
    if storage != 'fp32':
        r16 = _Run(lib_for(storage), MANT[storage][2], False)
        adapters[name]((storage, name, a), r16)
        torch.cuda.synchronize()
        twin = {lab: got for lab, got, _, _, _ in r32.res}
        twin_ref = {lab: ref for lab, _, ref, _, _ in r32.res if ref is not None}
        for label, got, ref, tol, act in r16.res:
            if got is None:
                out.append((label, 0.0 if ref else float('inf')))
            elif act:
                out.append((label + ' vs fp32 twin', _act_ratio(got, twin[label], storage)))
            elif label.startswith('stats'):
                # BatchNorm partial sums of a 16-bit entry: of z before its 16-bit store (the sums of the twin's fp32 z) or after
                # it (the sums of the z this call stored), as the kernel takes them; check_act's intermediate allowance (half a
                # 16-bit ulp of every summed magnitude) covers a split-K partial stored in 16 bits before the sum is formed
                mag = r16.stats_mag[label]
                allow = 2.0 ** -(MANT[storage][0] + 1) * float(mag.max()) / (float(ref.abs().max()) + 1e-30)
                out.append((label, min(_rel(got, twin_ref[label]), _rel(got, ref)) / (tol + allow)))
            else:           # fp32 result of the 16-bit entry: the twin's float64 reference
                out.append((label, _rel(got, twin_ref.get(label, ref)) / tol))
    return out


def _geom(name, a):
    """(B, H, W, dil) of a 3x3 launch."""
    if name.startswith('pp_conv3x3_wino_bwd_weight'):
        return a[6:10]
    if 'bwd' in name:
        return a[7:11]
    return a[8:12]


# ------------------------------------------------------------------------------------------------------------------ tests
def test_census_holds_what_the_dispatch_promises(census):
    """Not vacuous: the recording contains the kernel families the shape rules send these configurations to."""
    from pacingpseudo_amd._lib import lib

    def has(cfg_prefix, storage, names, pred=lambda n, a: True):
        return any(s == storage and n in names and pred(n, a) and any(c.startswith(cfg_prefix) for c in cfgs)
                   for (s, n, a), cfgs in census.items())

    def at(H, W, dil, tile=None):
        def pred(n, a):
            B, h, w, d = _geom(n, a)
            return (h, w, d) == (H, W, dil) and (tile is None or lib.pp_conv3x3_wino_tile(h, w, d) == tile)
        return pred
    fp32_fwd = lambda n, a: n == 'pp_conv3x3_wino_fwd' or a[12] == 0          # noqa: E731  (fwd_bn: f16x3 flag off)
    for cfg in ('224/os8/4cls', '224/os8/2cls'):
        assert has(cfg, 'fp32', ('pp_conv3x3_wino_fwd', 'pp_conv3x3_wino_fwd_bn'), lambda n, a: fp32_fwd(n, a) and at(28, 28, 2, 2)(n, a)), cfg
        assert has(cfg, 'fp32', ('pp_conv3x3_wino_bwd_data',), at(28, 28, 2, 2)), cfg
        assert has(cfg, 'fp32', ('pp_conv3x3_wino_bwd_weight',), at(28, 28, 2, 2)), cfg
    assert has('256/os8', 'fp32', ('pp_conv3x3_wino_bwd_data_f16x3',)) and has('256/os8', 'fp32', ('pp_conv3x3_wino_bwd_weight_f16x3',))
    assert has('256/os8', 'fp32', ('pp_conv3x3_wino_fwd_bn',), lambda n, a: a[12] == 1)
    for kind in ('fp16', 'bf16'):
        assert has(f'224/{kind}', kind, ('pp_conv3x3_fwd_bn', 'pp_conv3x3_fwd_f16x3', 'pp_conv3x3_bwd_data_f16x3'),
                   lambda n, a: (n != 'pp_conv3x3_fwd_bn' or a[12] == 1) and at(28, 28, 2)(n, a)), kind
    assert has('256/strided', 'fp32', ('pp_convtranspose_fwd', 'pp_convtranspose_bwd_data', 'pp_convtranspose_bwd_weight'))
    assert has('256x272/inference', 'fp32', ('pp_conv3x3_wino_fwd', 'pp_conv3x3_wino_fwd_bn'), at(32, 34, 1, 2))


def test_every_recorded_convolution_launch_matches_float64(census):
    """Replay every distinct launch; list every failing one, worst first, with the configurations that produced it."""
    per_cfg = defaultdict(int)
    for cfgs in census.values():
        for c in cfgs:
            per_cfg[c] += 1
    worst = defaultdict(float)
    failures, missing = [], set()
    for key in sorted(census, key=repr):
        try:
            res = replay(key)
        except KeyError as e:
            missing.add(str(e.args[0]))
            continue
        suffix = '' if key[0] == 'fp32' else ('_h16' if key[0] == 'fp16' else '_bf16')
        entry = key[1] + suffix
        for label, ratio in res:
            worst[entry] = max(worst[entry], ratio)
            if not ratio <= 1.0:
                failures.append((ratio, entry, label, key[2], sorted(census[key])))
    print(f'\nconvolution census: {len(census)} distinct launches')
    for c in sorted(per_cfg):
        print(f'  {c:28s} {per_cfg[c]:4d} distinct launches')
    for e in sorted(worst):
        print(f'  worst error / tolerance  {e:42s} {worst[e]:.3g}')
    assert not missing, f'recorded launches of entry points without a replay adapter: {sorted(missing)}'
    failures.sort(key=lambda f: -f[0] if f[0] == f[0] else -math.inf)
    assert not failures, '\n'.join(f'{r:.3g} x tol  {e}  {lab}  args={a}  from {cfgs}' for r, e, lab, a, cfgs in failures)
