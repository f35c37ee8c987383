"""Census of the convolution launches of real steps, each replayed against a float64 reference.

The per-kernel parity tests use hand-picked case lists; which kernel a layer gets is a function of its shape (convop.select).
Here every convolution-family launch of real full-width steps is recorded -- the engine's entry-point table (plan.K) is wrapped in a
recording proxy -- and every distinct launch (entry point, storage kind, every non-pointer argument, which optional pointers were
null, the ld / groups of a lazy input) is replayed on seeded random operands with the recorded ld's and flags and canaries in the
padding columns:
  * fp32 storage: against conv2d / conv_transpose2d / their gradients in float64 (outputs, data and weight gradients 1e-4,
    BatchNorm partial sums 1e-5); lazy-input forms against the lazy tensor evaluated in float64 and, bit for bit, against the
    ordinary entry point fed the materialised tensor (the harness of test_direct_convolution_with_lazy_input); the first layer's
    folded weight gradient against float64 autograd at the tolerances of test_first_layer_bn_backward_with_folded_weight_gradient,
    on operands moved off the LeakyReLU kink (_wgrad_c1).
  * 16-bit storage: the _h16 / _bf16 entry against its fp32 twin on operands representable in the 16-bit type (check_act's bound,
    with the output's own magnitude as the intermediate a kernel may store in 16 bits first; fp32 results such as weight gradients
    at 1e-4), and that fp32 twin against float64 at the same shape.
A second recording (tests/_launch_census.py::record_batches) runs batch 3 and 12, 16-bit storage at batch 3 and the Control plan on
128-pixel images, one test case per configuration; an edge table feeds hand-made launches to the same adapters at the states of
the launch plans (asserted through the library's plan queries), and a planted-mistake test shows the gate fails when an entry
point is called wrongly.
Every operand of a replay -- inputs, outputs, kept transforms, statistics rows, workspaces -- lies between sentinel bands of 0xFF
bytes (tests/_guard.py; _Run.d / _Run.out / _ws / _full / _empty / _zeros / _b): a read outside an input's extent that reaches a
result turns it into NaN and fails the float64 comparison, a write outside an output or a workspace adds a failing result line
'<buffer> band'.  A workspace is EXACTLY as large as the query include/pacingpseudo_hip.h names for that launch returns (what the
engine allocates for it) and starts as 0xFF, so a query that is too small, a kernel that writes a few bytes past it and a kernel
that relies on what an earlier layer left in the workspace all show.  The run's entry-point table (_Checked) holds every device
pointer of a launch to this: one that points into no banded buffer of the run is a failing result line.
The operands have one magnitude per kind (Profile: the default, CENSUS); tests/test_gpu_operand_range.py runs the same adapters at
others.  The pre-normalisation operand likewise (NormProfile: the default, NORM_CENSUS, leaves every draw as it is);
tests/test_gpu_norm_range.py moves its mean-to-spread ratio and scale (docs/norm_range.md).
A recorded launch without a replay adapter fails the census by name.  Outside the census: the stand-alone AuxPath.forward (it calls
the library directly, not through a plan) and --precision fp16 (fp16-grade by design, tested on its own).
"""
import contextlib
import ctypes
import math
import zlib
from collections import defaultdict
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn.functional as F

from tests._guard import BandSet

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
class Profile(NamedTuple):
    """Magnitudes of the operands of a replay.  The default is the point the censuses run at; tests/test_gpu_operand_range.py
    moves it (`with operands(profile):` around a replay)."""
    act: float = 1.0                # activations (forward input, the weight gradient's x) times this
    weight: float = 1.0             # weights times this
    grad: Optional[float] = None    # scale of the gradient operand dz; None: G_FP32 / G_16 by storage
    unit: bool = False              # |dz| = 2^-4u, u uniform in [0, 1), random sign, instead of randn: no element far below the largest
    peak: Optional[float] = None    # dz rescaled (in float64, rounded once) so that max |dz| is this
    spread: int = 0                 # output channel c of dz times 2^(-spread * c / (O - 1))
    balance: bool = False           # ... and output channel c of the weights times the inverse, so every channel contributes alike
    pow2: int = 0                   # dz times 2^pow2 AFTER it was rounded to the storage type (exact while nothing leaves the normal range)
    zero: bool = False              # dz == 0
    amax: Optional[float] = None    # the max |dz| cell the launch is handed; None: the true maximum of dz


CENSUS = Profile()
_PROFILE = [CENSUS]


@contextlib.contextmanager
def operands(profile):
    prev, _PROFILE[0] = _PROFILE[0], profile
    try:
        yield
    finally:
        _PROFILE[0] = prev


class NormProfile(NamedTuple):
    """Where the pre-normalisation operand z of a replay lies.  The default is the point the censuses run at (|mean| <= 4 sigma);
    tests/test_gpu_norm_range.py moves it (`with norm_operands(profile):` around a replay, docs/norm_range.md)."""
    offset: Optional[float] = None  # r: the channel mean is +-r * sigma_c, sign alternating by channel; None: mu in [-2, 2] as drawn.
    #                                 Fused epilogues (mode 1 / 2): the conv bias is +-r * (float64 deviation of the bias-free output)
    scale: int = 0                  # z times 2^scale


NORM_CENSUS = NormProfile()
_NORM_PROFILE = [NORM_CENSUS]


@contextlib.contextmanager
def norm_operands(profile):
    prev, _NORM_PROFILE[0] = _NORM_PROFILE[0], profile
    try:
        yield
    finally:
        _NORM_PROFILE[0] = prev


def _signs(C, device=None):
    """+1, -1, +1, ... per channel"""
    return 1.0 - 2.0 * (torch.arange(C, device=device) % 2).float()


class _Ops:
    """Seeded operands of one replay; activation-type tensors are rounded to the key's storage type (identical for the 16-bit
    entry and its fp32 twin).  Their magnitudes are the current Profile's."""

    def __init__(self, key):
        self.storage = key[0]
        self.g = torch.Generator().manual_seed(zlib.crc32(repr(key[1:]).encode()))
        self.prof = _PROFILE[0]
        self.nprof = _NORM_PROFILE[0]
        self.gs = (G_FP32 if self.storage == 'fp32' else G_16) if self.prof.grad is None else self.prof.grad

    def _chan(self, O_):
        """per-output-channel factors 2^(-spread * c / (O - 1))"""
        return torch.pow(2.0, -self.prof.spread * torch.arange(O_, dtype=torch.float64) / max(O_ - 1, 1))

    def grad(self, B, H, W, ld, O_):
        """The gradient operand dz of a 3x3 launch (NHWC, row length ld, O_ channels); the census profile: act(..., self.gs)."""
        p = self.prof
        if p.unit:
            v = torch.pow(2.0, -4.0 * torch.rand(B, H, W, O_, generator=self.g)) * self.gs
            v = torch.where(torch.rand(B, H, W, O_, generator=self.g) < 0.5, -v, v)
        else:
            v = self.randn(B, H, W, O_, scale=self.gs)
        if p.spread:
            v = (v.double() * self._chan(O_)).float()
        if p.peak is not None:
            v = (v.double() * (p.peak / float(v.abs().max()))).float()
        v = self.r(v)
        if p.zero:
            v = torch.zeros_like(v)
        if p.pow2:
            v = v * 2.0 ** p.pow2
        t = torch.full((B, H, W, ld), 5.0)
        t[..., :O_] = v
        return t

    def weights(self, O_, I):
        """(O_, I, 3, 3) weights of a 3x3 launch"""
        w = self.randn(O_, I, 3, 3, scale=1 / math.sqrt(9 * I))
        if self.prof.weight != 1.0:
            w = w * self.prof.weight
        if self.prof.balance and self.prof.spread:
            w = (w.double() / self._chan(O_).view(-1, 1, 1, 1)).float()
        return w

    def cell(self, dz):
        """the max |dz| cell of a split-fp16 gradient launch: the true maximum of the operand, or the profile's value"""
        return _amax(dz) if self.prof.amax is None else _b(torch.tensor([self.prof.amax], dtype=torch.float32))

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


class _Checked:
    """The entry-point table of a run: before a launch goes out, every device pointer it is handed (a void* argument; the
    stream, null pointers, host item tables and the pointers inside a lazy-input struct are not looked at) must point into the
    payload of a banded buffer of this run.  One that does not adds a failing result line naming the argument, so an operand that
    slipped past the bands cannot go unnoticed.  Adapters reach the library through run.K (the entry under test) or _L() (helper
    launches: packs, statistics, loss finalisation); both are wrapped."""

    def __init__(self, inner, run):
        self._inner, self._run = inner, run

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        from tests._launch_census import is_launch
        if not is_launch(name):
            return fn

        def call(*a):
            from pacingpseudo_amd._lib import _PROTOS
            spans = [(b.data_ptr(), b.data_ptr() + b.nbytes) for _, b in self._run.bands.items]
            for i, (t, v) in enumerate(zip(_PROTOS[name][1][:-1], a)):
                if t is ctypes.c_void_p and isinstance(v, int) and v and not any(lo <= v < hi or v == lo == hi for lo, hi in spans):
                    self._run.res.append((f'{name} argument {i} points into no banded buffer', None, False, None, False))
            return fn(*a)
        return call


class _Run:
    """One execution of a launch: K = entry-point table, dt = activation dtype; collects (label, device result, fp64 reference,
    tolerance, is-activation) and canary verdicts."""

    def __init__(self, K, dt, want_ref):
        from pacingpseudo_amd._lib import stream_ptr
        self.K, self.dt, self.want_ref, self.st = _Checked(K, self), dt, want_ref, stream_ptr()
        self.res, self.keep = [], []
        from pacingpseudo_amd._lib import lib
        self.L = _Checked(lib, self)          # the fp32 table for helper launches beside the one under test: checked alike
        self.bands = BandSet(0xFF, _dev())        # every operand of the launch made through d / out / _ws / _full / _empty / _zeros / _b

    def d(self, t, act=True):
        """t on the device in the run's activation type (act) or fp32, between sentinel bands -- inputs too: a read outside an
        input's extent that reaches a result makes it NaN."""
        x = self.bands.tensor(t, self.dt if act else torch.float32)
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


_CUR = [None]       # the _Run whose adapter is executing (replay sets it): where the helpers below register their buffers


def _L():
    """The library for an adapter's helper launches and size queries: inside a replay the run's checked fp32 table."""
    from pacingpseudo_amd._lib import lib
    return _CUR[0].L if _CUR[0] is not None else lib


def _bands():
    if _CUR[0] is None:
        raise RuntimeError('an operand helper of the census was called outside a replay: its bands would never be read')
    return _CUR[0].bands


def _shape(shape):
    return tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)


def _ws(n):
    """A workspace of EXACTLY n bytes (the size the header's query returns for the launch, which is what the engine allocates
    for it), stale (0xFF) and with a sentinel band behind it (tests/_guard.py)."""
    return _bands().ws(int(n))


def _full(shape, value, dtype=torch.float32):
    return _bands().tensor(_shape((shape,)), dtype, fill=value)


def _zeros(*shape, dtype=torch.float32):
    return _bands().tensor(_shape(shape), dtype, fill=0)


def _empty(*shape, dtype=torch.float32):
    """an uninitialised buffer between bands: the payload starts as 0xFF (NaN / -1), so reading an element nobody wrote shows."""
    return _bands().tensor(_shape(shape), dtype)


def _b(t):
    """t (any device) as a banded device tensor of the same type"""
    return _bands().tensor(t)


def _amax(t):
    return _b(t.float().abs().max().reshape(1))


def _cudnn_off():
    return torch.backends.cudnn.flags(enabled=False)


# ---------------------------------------------------------------------------------------------------------------- adapters
def _pack_direct(w, O_, I, f16):
    from pacingpseudo_amd._lib import stream_ptr
    lib = _L()
    wf, wb = _zeros(O_, 9, I), _zeros(I, 9, O_)
    (lib.pp_pack_conv3x3_weights_f16x3 if f16 else lib.pp_pack_conv3x3_weights)(w.data_ptr(), O_, I, I, wf.data_ptr(), wb.data_ptr(),
                                                                                  stream_ptr())
    return wf, wb


def _pack_wino(w, O_, I, tile, f16, K=None):
    """U of the geometry's tile, packed through the entry-point table K of the run (a stand-in table can pack wrongly)."""
    from pacingpseudo_amd._lib import stream_ptr
    lib = _L()
    K = lib if K is None else K
    n = (tile + 2) ** 2
    uf, ub = _zeros(n, O_, I), _zeros(n, I, O_)
    (K.pp_wino_pack_weights_f16x3 if f16 else K.pp_wino_pack_weights)(w.data_ptr(), O_, I, tile, uf.data_ptr(), ub.data_ptr(),
                                                                      stream_ptr())
    return uf, ub


def _conv_in(ops, lz, run, ld, C, B, H, W, scale=1.0):
    """The input of a launch: plain, or lazy (lz = ('lazy', ld, groups): raw z + coefficient rows): (device tensor, lazy struct or
    None, fp64 NCHW value the convolution sees, materialised-y tensor for the bit-identity check or None)."""
    x = ops.act(B, H, W, ld, C, scale * ops.prof.act)
    if lz is None:
        return run.d(x), None, _n64(x, C) if run.want_ref else None, None
    from pacingpseudo_amd._lib import PpLazyIn
    coef = ops.lazy(lz, C)
    cd = run.d(coef, act=False)
    st = PpLazyIn(cd.data_ptr(), lz[1], lz[2])
    run.keep.append(st)
    xd = run.d(x)
    y = _empty(xd.shape, dtype=xd.dtype)
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
    w = _b(ops.weights(N, C))
    b = _b(ops.randn(N))
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
    lib = _L()
    ops = _Ops(key)
    x, _, x64, _ = _conv_in(ops, None, run, ld_in, C, B, H, W)
    w = _b(ops.weights(N, C))
    b = _b(ops.randn(N))
    prior = ops.r(ops.randn(B, H, W, N)) if acc else None
    U, _ = _pack_wino(w, N, C, lib.pp_conv3x3_wino_tile(H, W, dil), f16, run.K)
    nws = lib.pp_conv3x3_wino_workspace(C, N, B, H, W, dil)
    ws = _ws(nws)
    vk = _empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil)) if vkeep else None
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
    w = _b(ops.weights(N, C))
    b = _b(ops.randn(N))
    sc = _b((torch.rand(N, generator=ops.g) + 0.5))
    sh = _b(ops.randn(N))
    lib = _L()
    off = ops.nprof.offset
    if off is not None:
        # the bias puts channel c of z = conv + bias at +-off deviations of its bias-free output from zero; the eval epilogue
        # then normalises with that running mean: shift = beta - bias * scale, and y = z * scale + shift cancels
        with _cudnn_off():
            free = F.conv2d(x64 if x64 is not None else _n64(x if ymat is None else ymat, C), w.double(), None, 1, dil, dil)
        b = _b((free.std((0, 2, 3), unbiased=False) * off * _signs(N, _dev())).float())
        if mode == 2:
            sh = _b((sh.double() - b.double() * sc.double()).float())
    if wino:
        tile = lib.pp_conv3x3_wino_tile(H, W, dil)
        U, _ = _pack_wino(w, N, C, tile, f16, run.K)
        nws = lib.pp_conv3x3_wino_workspace(C, N, B, H, W, dil)
        ws = _ws(nws)
        vk = _empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil)) if vkeep else None
    else:
        U, _ = _pack_direct(w, N, C, f16)
        am = _amax(x[..., :C]) if in_amax else None
    nst = lib.pp_conv3x3_bn_stats_bytes(N, B, H, W, groups)
    rows = ctypes.c_int(0)
    results = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        out = run.out(B, H, W, ld_out, N)
        stats = _full((nst // 8,), float('nan'), dtype=torch.float64)
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
        if off is not None:
            # the sums alone do not show the cancellation of var = q / n - mean^2: the partial rows go through pp_bn_train_finalize
            # as in a step, and its rows are held to the float64 statistics of the z this launch produced
            n, eps, mom = zc.shape[1], 1e-5, 0.1
            rows_d, rm, rv, nbt = _b(stats), _zeros(N), _full((N,), 1.0), _full((), 0, dtype=torch.int64)
            coef = _full((4, groups, N), 7.0)
            lib.pp_bn_train_finalize(rows_d.data_ptr(), r, N, n, groups, eps, mom, sc.data_ptr(), sh.data_ptr(), rm.data_ptr(),
                                     rv.data_ptr(), nbt.data_ptr(), *(coef[i].data_ptr() for i in range(4)), run.st)
            mean, var = zc.mean(1), zc.var(1, unbiased=False)
            invstd = 1.0 / torch.sqrt(var + eps)
            scale64 = sc.double() * invstd
            rv64 = torch.ones(N, dtype=torch.float64, device=_dev())
            for g in range(groups):
                rv64 = (1 - mom) * rv64 + mom * var[g] * (n / max(n - 1, 1))
            for i, (lab, ref64) in enumerate((('save_mean', mean), ('save_invstd', invstd), ('scale', scale64),
                                              ('shift', sh.double() - mean * scale64))):
                run.check('finalized ' + lab, coef[i], ref64, TOL_SUMS, act=False)
            run.check('finalized running_var', rv, rv64, TOL_SUMS, act=False)


def _bwd_data(key, run):
    """pp_conv3x3_bwd_data[_f16x3] / pp_conv3x3_wino_bwd_data[_f16x3]"""
    _, name, a = key
    wino, f16 = 'wino' in name, name.endswith('_f16x3')
    _, ld_dz, O_, _, _, ld_dx, I, B, H, W, dil, acc = a[:12]
    ops = _Ops(key)
    dz = run.d(ops.grad(B, H, W, ld_dz, O_))
    w = _b(ops.weights(O_, I))
    prior = ops.r(ops.randn(B, H, W, I, scale=ops.gs)) if acc else None
    dx = run.out(B, H, W, ld_dx, I, prior)
    am = ops.cell(dz[..., :O_]) if (f16 and a[-2]) else None
    lib = _L()
    if wino:
        _, Ub = _pack_wino(w, O_, I, lib.pp_conv3x3_wino_tile(H, W, dil), f16, run.K)
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
    lib = _L()
    if wino:
        _, ld_dz, O_, _, ld_x, C, B, H, W, dil, _, acc, vcached = a[:13]
        Cpad, I = C, C
    else:
        _, ld_dz, O_, _, ld_x, Cpad, I, B, H, W, dil, _, acc = a[:13]
        vcached = None
    ops = _Ops(key)
    dz = run.d(ops.grad(B, H, W, ld_dz, O_))
    x, lz, x64, ymat = _conv_in(ops, a[-2] if name.endswith('_lazy') else None, run, ld_x, Cpad, B, H, W)
    if Cpad > I:            # the padded input channels of the first layer hold zeros
        x[..., I:Cpad] = 0
        if x64 is not None:
            x64[:, I:] = 0
    prior = ops.randn(O_, I, 3, 3) * ops.gs if acc else None
    am = ops.cell(dz[..., :O_]) if (f16 and a[-3 if name.endswith('_lazy') else -2]) else None
    outs = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        dw = _b(prior.clone() if acc else torch.full((O_, I, 3, 3), 5.0))
        if wino:
            nws = lib.pp_conv3x3_wino_bwd_weight_workspace(O_, C, B, H, W, dil)
            ws = _ws(nws)
            vk = None
            if vcached:
                tile = lib.pp_conv3x3_wino_tile(H, W, dil)
                vk = _empty(lib.pp_conv3x3_wino_vkeep_elems(C, B, H, W, dil))
                uf, _ = _pack_wino(_b(ops.randn(O_, C, 3, 3)), O_, C, tile, f16, run.K)
                tmp = run.out(B, H, W, O_, O_)
                fwd = run.K.pp_conv3x3_wino_fwd_f16x3 if f16 else run.K.pp_conv3x3_wino_fwd
                nwf = lib.pp_conv3x3_wino_workspace(C, O_, B, H, W, dil)             # the forward that keeps V: its own workspace
                fwd(src.data_ptr(), ld_x, C, uf.data_ptr(), None, tmp.data_ptr(), O_, O_, B, H, W, dil, 0, vk.data_ptr(),
                    _ws(nwf).data_ptr(), nwf, run.st)
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
    lib = _L()
    if 'fwd' in name:
        _, ld_x, C, _, bias, _, K_, N, HW = a[:9]
    else:
        _, _, ld_x, C, _, dxp, ld_dx, _, dbp, K_, N, HW, acc_dx, acc_p = a[:14]
    x, lz, x64, ymat = _conv_in(ops, a[-2] if name.endswith('_lazy') else None, run, ld_x, C, N, HW, 1)
    w = _b(ops.randn(K_, C, scale=1 / math.sqrt(C)))
    y64 = x64.reshape(N, C, HW) if x64 is not None else None
    if 'fwd' in name:
        b = _b(ops.randn(K_))
        outs = []
        for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
            lo = _full((N, K_, HW), 7.0)
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
    dl = _b((ops.randn(N, K_, HW) * ops.gs))
    pdx = ops.r(ops.randn(N, 1, HW, C, scale=ops.gs)) if acc_dx else None
    pdw, pdb = ops.randn(K_, C) * ops.gs, ops.randn(K_) * ops.gs
    nws = lib.pp_conv1x1_bwd_workspace(K_, C, N, HW)
    ws = _ws(nws)
    outs = []
    for src, lzs in ((x, lz),) + (((ymat, None),) if lz is not None else ()):
        dx = run.out(N, 1, HW, ld_dx, C, pdx) if dxp else None
        dw = _b(pdw if acc_p else torch.full((K_, C), 5.0))
        db = _b(pdb if acc_p else torch.full((K_,), 5.0))
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
    lib = _L()
    if name == 'pp_convtranspose_fwd':
        _, ld_x, Cin, _, _, ld_out, Cout, k, N, H, W = a[:11]
    elif name == 'pp_convtranspose_bwd_data':
        _, ld_out, Cout, _, _, ld_x, Cin, k, N, H, W, acc = a[:12]
    else:
        _, ld_out, Cout, _, ld_x, Cin, k, N, H, W, _, acc = a[:12]
    w = _b(ops.randn(Cin, Cout, k, k, scale=1 / math.sqrt(Cin)))
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
    dw = _b(prior.clone() if acc else torch.full((Cin, Cout, k, k), 5.0))
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
    fp32 twin: dW, dgamma, dbeta (and, where it is not 0 by construction, the conv-bias gradient) against float64 autograd of
    batch_norm + leaky_relu per statistics group and conv2d_weight of its dz, at the tolerances of
    test_first_layer_bn_backward_with_folded_weight_gradient; the one-pass eval form reads (dy, y) and recovers xhat from y: with
    fp32 storage it is held to the same autograd from z (dgamma at 5 x TOL, that test's figure), only the fp32 twin of a 16-bit
    launch, which is handed a y rounded to 16 bits, to the float64 value of that recovery on the y of the call.
    That test's own operands serve its small shapes only: over 10^7 elements one pre-activation lies within fp32 rounding of the
    LeakyReLU kink, float64 takes the other branch there and a single such element moves dW by 2e-4 of its largest entry (seen at
    24 x 128 x 128); so, as in the stream census, the few z whose pre-activation is within 1e-4 of the kink are moved off it.
    16-bit entry: against the twin on identical representable operands and coefficient rows (its results are fp32)."""
    storage, name, a = key
    ev = 'eval' in name
    if ev:
        _, ld_dy, _, ld_z, _, _, _, _, ld_x, H, W, _, acc_dw, _, _, _, acc_p, C, P = a[:19]
        groups, training = 1, False
    else:
        _, ld_dy, _, ld_z, _, _, _, _, _, training, _, ld_x, H, W, _, acc_dw, _, _, _, acc_p, C, ppg, groups = a[:23]
        P = ppg * groups
    B = P // (groups * H * W)
    lib = _L()
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
    coef = _empty(4, groups, C)
    mean, invstd, scale, shift = (coef[i].data_ptr() for i in range(4))
    gd, bd = (_b(t) for t in (gamma, beta))
    nbt = _zeros((), dtype=torch.int64)
    # the launch under test: exactly what its own query returns (the eval form: all pixels as one group); the statistics call
    # that only prepares the coefficient rows has a workspace of its own
    nws = lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(C, P, 1) if ev else lib.pp_bn_lrelu_bwd_wgrad_c1_workspace(C, P // groups, groups)
    ws = _ws(nws)
    nws_stats = lib.pp_bn_workspace(C, P // groups, groups)
    ws_stats = _ws(nws_stats)

    def rows(zt):           # the coefficient rows the kernels are handed, from the library itself
        rmd, rvd = _b(rm), _b(rv)
        if training:
            lib.pp_bn_train_stats(zt.data_ptr(), ld_z, C, P // groups, groups, 1e-5, 0.1, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(),
                                  rvd.data_ptr(), nbt.data_ptr(), mean, invstd, scale, shift, ws_stats.data_ptr(), nws_stats, run.st)
        else:
            lib.pp_bn_eval_coeffs(C, groups, 1e-5, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), mean, invstd, scale,
                                  shift, run.st)
        torch.cuda.synchronize()
    z32 = _b(z)
    rows(z32)
    v = z32[..., :C].double().reshape(groups, -1, C)
    near = ((v * coef[2].double()[:, None] + coef[3].double()[:, None]).abs() < 1e-4).reshape(N, H, W, C)
    z32[..., :C] = torch.where(near, ops.r((z32[..., :C] + 0.125).cpu()).to(_dev()), z32[..., :C])
    rows(z32)               # (train mode: the rows move by ~1e-6, the margin stays)
    if ev:          # the one-pass eval form reads the stored output y = lrelu(z * scale + shift)
        pre = z32[..., :C] * coef[2] + coef[3]
        zsrc = z32.clone()
        zsrc[..., :C] = ops.r(torch.where(pre > 0, pre, pre * 0.01).cpu()).to(_dev())
    else:
        zsrc = z32
    res = []
    pdw, pp = ops.randn(C, 1, 3, 3) * ops.gs, ops.randn(3, C) * ops.gs
    for K, dt in ((run.K, run.dt),) if run.dt == torch.float32 else ((lib, torch.float32), (run.K, run.dt)):
        xd, zd, dyd = (_b(t.to(_dev()).to(dt)) for t in (x, zsrc, dy))
        dw = _b(pdw if acc_dw else torch.full((C, 1, 3, 3), 5.0))
        dg, db, dbc = (_b(pp[i] if acc_p else torch.full((C,), 9.0)) for i in range(3))
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
    labels = ('dw', 'dgamma', 'dbeta', 'dbias')
    if run.dt != torch.float32:
        for label, h, f in zip(labels, res[1], res[0]):
            run.res.append((label + ' vs fp32 twin', h, f.double(), TOL, False))
        return
    refs = [None] * 4
    if run.want_ref and ev and storage != 'fp32':         # the twin of a 16-bit launch is handed a ROUNDED y: the same operation on (dy, y)
        y64, dy64 = zsrc[..., :C].double(), dy[..., :C].double().to(_dev())
        gg = torch.where(y64 > 0, dy64, dy64 * 0.01)
        xhat = (torch.where(y64 > 0, y64, y64 / 0.01) - bd.double()) / gd.double()
        dz = (gg * coef[2, 0].double()).permute(0, 3, 1, 2)
        with _cudnn_off():
            refs[0] = torch.nn.grad.conv2d_weight(_n64(x, 1), (C, 1, 3, 3), dz, 1, 1, 1) + (pdw.double().to(_dev()) if acc_dw else 0)
        prior = pp.double().to(_dev()) if acc_p else torch.zeros(3, C, dtype=torch.float64, device=_dev())
        refs[1], refs[2], refs[3] = (gg * xhat).sum((0, 1, 2)) + prior[0], gg.sum((0, 1, 2)) + prior[1], dz.sum((0, 2, 3)) + prior[2]
    elif run.want_ref:
        zr = _n64(z32, C).requires_grad_(True)
        g64, b64 = gd.double().requires_grad_(True), bd.double().requires_grad_(True)
        rm64, rv64 = rm.double().to(_dev()), rv.double().to(_dev())
        ys = [F.leaky_relu(F.batch_norm(zr[gi * B:(gi + 1) * B], rm64.clone(), rv64.clone(), g64, b64, bool(training), 0.1, 1e-5), 0.01)
              for gi in range(groups)]
        torch.cat(ys).backward(_n64(dy, C))
        with _cudnn_off():
            refs[0] = torch.nn.grad.conv2d_weight(_n64(x, 1), (C, 1, 3, 3), zr.grad, 1, 1, 1) + (pdw.double().to(_dev()) if acc_dw else 0)
        prior = pp.double().to(_dev()) if acc_p else torch.zeros(3, C, dtype=torch.float64, device=_dev())
        refs[1], refs[2], refs[3] = g64.grad + prior[0], b64.grad + prior[1], zr.grad.sum((0, 2, 3)) + prior[2]
    for label, got, ref in zip(labels, res[0], refs):
        if label == 'dbias' and training:         # the sum of a train-mode dz is 0: nothing to be relative to
            continue
        run.check(label, got, ref, tol=5 * TOL if (ev and label == 'dgamma') else TOL, act=False)


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


def _execute(adapter, key, run):
    """Run one adapter with `run` as the home of its buffers, then add one result line per buffer, '<label> band': intact or not
    (all bands of the launch compared on the device, one read)."""
    _CUR[0] = run
    try:
        adapter(key, run)
    finally:
        _CUR[0] = None
    torch.cuda.synchronize()
    for label, ok in run.bands.verdicts():
        run.res.append((label + ' band', None, ok, None, False))


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
    _execute(adapters[name], (storage, name, a), r32)
    for label, got, ref, tol, _ in r32.res:
        tag = 'fp32 twin ' if storage != 'fp32' else ''
        if got is None:
            out.append((tag + label, 0.0 if ref else float('inf')))
        else:
            out.append((tag + label, _rel(got, ref) / tol))
    if storage != 'fp32':
        r16 = _Run(lib_for(storage), MANT[storage][2], False)
        _execute(adapters[name], (storage, name, a), r16)
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


def _report(keys, cfgs_of):
    """Replay `keys`; print the worst error / tolerance per entry point; return (failures, entry points without an adapter)."""
    worst = defaultdict(float)
    failures, missing = [], set()
    for key in keys:
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
                failures.append((ratio, entry, label, key[2], cfgs_of(key)))
    for e in sorted(worst):
        print(f'  worst error / tolerance  {e:42s} {worst[e]:.3g}')
    failures.sort(key=lambda f: -f[0] if f[0] == f[0] else -math.inf)
    return failures, missing


def test_every_recorded_convolution_launch_matches_float64(census):
    """Replay every distinct launch; list every failing one, worst first, with the configurations that produced it."""
    per_cfg = defaultdict(int)
    for cfgs in census.values():
        for c in cfgs:
            per_cfg[c] += 1
    print(f'\nconvolution census: {len(census)} distinct launches')
    for c in sorted(per_cfg):
        print(f'  {c:28s} {per_cfg[c]:4d} distinct launches')
    failures, missing = _report(sorted(census, key=repr), lambda key: sorted(census[key]))
    assert not missing, f'recorded launches of entry points without a replay adapter: {sorted(missing)}'
    assert not failures, '\n'.join(f'{r:.3g} x tol  {e}  {lab}  args={a}  from {cfgs}' for r, e, lab, a, cfgs in failures)


# ---------------------------------------------------------------------------------- other batch sizes and the Control plan
def _of_config(rec, cfg):
    """The launches of one configuration of record_batches() (labels are '<configuration>/<train|eval>-BN')."""
    return {key: cfgs for key, cfgs in rec.items() if any(c.rsplit('/', 1)[0] == cfg for c in cfgs)}


def _batch_config_names():
    from tests._launch_census import batch_configs
    return sorted(batch_configs())


@pytest.mark.parametrize('cfg', _batch_config_names())
def test_batch_recording_matches_float64(cfg):
    """The launch plans of the family are functions of B * H * W and of tile counts, and the census above records every
    configuration at batch 2: here batch 3 and 12 (6 and 24 images through the two-view pass), 16-bit storage at batch 3 and the
    Control plan (one backbone pass, one statistics group) at batch 8, every launch through the same replay and tolerances."""
    from tests._launch_census import batch_configs, record_batches
    storage, size, _, _, variant, batch = batch_configs()[cfg]
    every = _of_config(record_batches(), cfg)
    mine = {key: cfgs for key, cfgs in every.items() if _is_conv_launch(key[1])}
    conv3 = [(n, a) for (_, n, a) in mine if n.startswith('pp_conv3x3_')]
    images = {_geom(n, a)[0] for n, a in conv3}
    groups = {a[20] if 'wino' in n else a[18] for n, a in conv3 if n.startswith(('pp_conv3x3_fwd_bn', 'pp_conv3x3_wino_fwd_bn'))}
    print(f'\n{cfg}: {len(mine)} distinct convolution launches, images {sorted(images)}, statistics groups {sorted(groups)}')
    # not vacuous: the image counts this batch size gives, the weight-gradient families, the BatchNorm backward beside them
    if variant == 'control':
        assert batch in images and 2 * batch not in images and groups == {1}, (images, groups)
    else:
        assert 2 * batch in images and 2 in groups, (images, groups)
    for prefix in ('pp_conv3x3_bwd_weight', 'pp_conv3x3_wino_bwd_weight'):
        assert any(n.startswith(prefix) for n, _ in conv3), prefix
    assert any(key[1].startswith('pp_bn_lrelu_bwd') for key in every)
    assert all(key[0] == storage for key in mine if key[1].startswith('pp_conv3x3_')), cfg
    failures, missing = _report(sorted(mine, key=repr), lambda key: sorted(mine[key]))
    assert not missing, f'recorded launches of entry points without a replay adapter: {sorted(missing)}'
    assert not failures, '\n'.join(f'{r:.3g} x tol  {e}  {lab}  args={a}  from {cfgs}' for r, e, lab, a, cfgs in failures)


# ------------------------------------------------------------------------------------------------- launch plans at their edges
# Hand-made launch shapes through the same adapters, at the sizes where the launch plans of the family change state: the number
# of reduction splits, an uneven last split, a partial last chunk / segment / wave, tile walkers that get no tile.  Every
# weight-gradient row names the state it is there for and asserts it through the library's plan queries first
# (pp_conv3x3_bwd_weight_plan, pp_conv3x3_wino_bwd_weight_plan, pp_convtranspose_bwd_weight_splits: the launchers' own plan
# functions), so that a row whose plan drifted fails instead of testing something else.  Forward, BatchNorm-epilogue and data-gradient
# rows are generated from the geometries of ALL 3x3 weight-gradient rows, in the family convop.select picks, and assert that it
# does.  Operands are a few thousand pixels (the largest tensor of a row stays below 64 MB; the workspace is whatever the library's
# own query asks for).
SLOPE = 0.01
C4, W9, T32, T64, T128, HALO, HALO21, HALO12 = 1, 2, 3, 4, 5, 6, 7, 8          # PP_WGRAD_PATH_* of include/pacingpseudo_hip.h
SLABS, PER, LAST, UNITS, LIVE, LAST_PX = range(6)                              # out[] of pp_conv3x3_bwd_weight_plan
W_BM, W_PER, W_LAST, W_CHUNKS, W_LAST_TILES, W_TILES = range(6)                # out[] of pp_conv3x3_wino_bwd_weight_plan
MIN_CUS = 8             # the smallest budget pp_set_wgrad_cus accepts


def _k_wgrad(name, O_, C, I, B, H, W, dil, acc, lazy_groups=1):
    a = ('p', O_ + 8, O_, 'p', C + 16, C, I, B, H, W, dil, 'p', acc, 'p', 'sz')
    if 'f16x3' in name:
        a += ('p',)
    if name.endswith('_lazy'):
        a += (('lazy', C + 8, lazy_groups),)
    return (name, a + ('p',))


def _k_wino_wgrad(name, O_, C, B, H, W, dil, acc, vcached):
    a = ('p', O_ + 8, O_, 'p', C + 16, C, B, H, W, dil, 'p', acc, 'p' if vcached else None, 'p', 'sz')
    return (name, a + (('p', 'p') if name.endswith('_f16x3') else ('p',)))


def _k_fwd(family, O_, C, B, H, W, dil, acc=0, bias=1):
    head = ('p', C + 16, C, 'p', 'p' if bias else None, 'p', O_ + 8, O_, B, H, W, dil, acc)
    if family == 'fp32':
        return ('pp_conv3x3_fwd', head + ('p',))
    if family == 'f16x3':
        return ('pp_conv3x3_fwd_f16x3', head + (None, 'p'))             # (ConvOp.fwd passes no in_amax)
    return ('pp_conv3x3_wino_fwd_f16x3' if family == 'wino-split' else 'pp_conv3x3_wino_fwd', head + ('p', 'p', 'sz', 'p'))


def _k_fwd_bn(family, O_, C, B, H, W, dil, mode, groups=1):
    head = ('p', C + 16, C, 'p', 'p', 'p', O_ + 8, O_, B, H, W, dil)
    bn = (mode, None if mode == 1 else 'p', None if mode == 1 else 'p', SLOPE, groups, 'p' if mode == 1 else None, 'sz', 'p')
    if family in ('fp32', 'f16x3'):
        return ('pp_conv3x3_fwd_bn', head + (int(family == 'f16x3'), None) + bn + ('p',))
    return ('pp_conv3x3_wino_fwd_bn', head + (int(family == 'wino-split'), 'p', 'p', 'sz') + bn + ('p',))


def _k_bwd_data(family, O_, C, B, H, W, dil, acc):
    head = ('p', O_ + 8, O_, 'p', 'p', C + 16, C, B, H, W, dil, acc)
    if family == 'fp32':
        return ('pp_conv3x3_bwd_data', head + ('p',))
    if family == 'f16x3':
        return ('pp_conv3x3_bwd_data_f16x3', head + ('p', 'p'))
    if family == 'wino':
        return ('pp_conv3x3_wino_bwd_data', head + ('p', 'sz', 'p'))
    return ('pp_conv3x3_wino_bwd_data_f16x3', head + ('p', 'sz', 'p', 'p'))


def _k_ct(name, Cin, Cout, k, N, H, W, acc=0):
    ld_x, ld_o = Cin + 4, Cout + 4
    if name == 'pp_convtranspose_fwd':
        return (name, ('p', ld_x, Cin, 'p', 'p', ld_o, Cout, k, N, H, W, 'p'))
    if name == 'pp_convtranspose_bwd_data':
        return (name, ('p', ld_o, Cout, 'p', 'p', ld_x, Cin, k, N, H, W, acc, 'p'))
    return (name, ('p', ld_o, Cout, 'p', ld_x, Cin, k, N, H, W, 'p', acc, 'p', 'sz', 'p'))


def _family(O_, C, I, H, W, dil):
    """convop.select's kernel family of a layer (O, C, I = true input channels) at (H, W, dil) with fp32 storage."""
    if I == C and C >= 256 and O_ >= 64 and H % (2 * dil) == 0 and W % (2 * dil) == 0:
        return 'wino-split' if (H % (4 * dil) == 0 and W % (4 * dil) == 0 and C % 8 == 0 and O_ % 8 == 0) else 'wino'
    return 'f16x3' if (I == C and C % 4 == 0 and O_ % 4 == 0 and O_ >= 32) else 'fp32'


# Winograd geometries (O, C, B, H, W, dil) -> (tile, splits, {plan field: value}); 256 input channels: where convop.select
# takes the Winograd family
WINO_EDGES = {
    'tile4-bm64-one-split-one-partial-chunk-B1': ((64, 256, 1, 16, 16, 1), 4, 1, {W_BM: 64, W_CHUNKS: 1, W_LAST_TILES: 16}),
    'tile2-dil2-odd-7x7-tiles-bm64-O192-uneven-split-B3': ((192, 256, 3, 28, 28, 2), 2, 2,
                                                             {W_BM: 64, W_PER: 10, W_LAST: 9, W_CHUNKS: 19, W_LAST_TILES: 12}),
    'tile2-dil2-sub-image-6x10-bm128-one-split-B5': ((128, 256, 5, 12, 20, 2), 2, 1, {W_BM: 128, W_CHUNKS: 10, W_LAST_TILES: 12}),
    'tile4-bm128-uneven-split-partial-chunk-B5': ((128, 256, 5, 44, 44, 1), 4, 2,
                                                    {W_BM: 128, W_PER: 10, W_LAST: 9, W_CHUNKS: 19, W_LAST_TILES: 29, W_TILES: 605}),
    'tile4-bm128-two-row-tiles-C264-partial-channel-tile': ((256, 264, 1, 16, 16, 1), 4, 1, {W_BM: 128, W_CHUNKS: 1}),
    'tile4-dil2-odd-7x7-tiles-bm64-uneven-split-B3': ((64, 256, 3, 56, 56, 2), 4, 2, {W_BM: 64, W_PER: 10, W_LAST: 9, W_LAST_TILES: 12}),
    'tile4-bm64-O192-uneven-split-half-chunk-B5': ((192, 256, 5, 48, 48, 1), 4, 2,
                                                     {W_BM: 64, W_PER: 12, W_LAST: 11, W_CHUNKS: 23, W_LAST_TILES: 16}),
}
G0 = (3, 20, 28)        # P = 1680: no multiple of any chunk length, W % 32 != 0 (neither wgrad9 nor the halo kernels)
# ConvTranspose input geometries (N, H, W) -> (splits, pixels per split, pixels in the last split)
CT_EDGES = {'P4096-one-split': ((1, 64, 64), (1, 4096, 4096)), 'P4097-two-uneven-splits': ((1, 17, 241), (2, 2049, 2048)),
            'P258064-at-the-64-split-cap-uneven': ((1, 508, 508), (64, 4033, 3985))}


def _edge_cases():
    """[(tag, launch)], {tag: expectation}: ('direct', f16x3, path, {field: value}) / ('wino', geometry, tile, splits, {field:
    value}) / ('ct', geometry, (splits, per, last)) for weight-gradient rows, ('family', kind, O, C, I, H, W, dil) or ('tile', (H, W, dil),
    tile) for the rest."""
    cases, expect, geos = [], {}, {}

    def add(tag, launch, exp):
        assert tag not in expect, tag
        cases.append((tag, launch))
        expect[tag] = exp
        name, a = launch
        if name.startswith('pp_conv3x3_wino_bwd_weight'):          # (O, C, I, B, H, W, dil) of every 3x3 weight-gradient row
            geos[(a[2], a[5], a[5]) + tuple(a[6:10])] = None
        elif name.startswith('pp_conv3x3_bwd_weight'):
            geos[(a[2], a[5], a[6]) + tuple(a[7:11])] = None
    # -- generic direct weight gradient (wgrad_plan)
    generic = [(32, 32, T32, {PER: 4, LAST: 2, UNITS: 14}), (64, 64, T64, {PER: 7, LAST: 6, UNITS: 27}),
               (128, 128, T128, {PER: 14, LAST: 11, UNITS: 53}), (64, 96, T32, {PER: 4, LAST: 2, UNITS: 14}),
               (192, 64, T64, {PER: 7, LAST: 6, UNITS: 27})]
    for O_, C, path, st in generic:
        for dil in (1, 2):
            for acc in ((0, 1) if O_ == C == 32 else (dil - 1,)):
                add(f'wgrad/tile{(32, 64, 128)[path - T32]}/O{O_}-C{C}/4-splits-uneven-last-16px-chunk/dil{dil}/acc{acc}',
                    _k_wgrad('pp_conv3x3_bwd_weight', O_, C, C, *G0, dil, acc), ('direct', 0, path, {**st, SLABS: 4, LAST_PX: 16}))
    add('wgrad/tile32/one-split-partial-last-chunk', _k_wgrad('pp_conv3x3_bwd_weight', 32, 32, 32, 3, 6, 10, 1, 0),
        ('direct', 0, T32, {SLABS: 1, UNITS: 2, LAST_PX: 52}))
    add('wgrad/tile32/I_true5-of-Cpad8', _k_wgrad('pp_conv3x3_bwd_weight', 32, 8, 5, *G0, 1, 0), ('direct', 0, T32, {SLABS: 4, LAST_PX: 16}))
    # -- wgrad9: 64-pixel row segments
    for (B, H, W), st, what in (((1, 2, 64), {SLABS: 1, UNITS: 2}, 'one-split'),
                                ((5, 7, 64), {SLABS: 3, PER: 12, LAST: 11, UNITS: 35}, '3-splits-last-11-boundaries-inside-images'),
                                ((3, 5, 128), {SLABS: 2, PER: 15, LAST: 15, UNITS: 30}, 'two-segments-per-row')):
        for i, (O_, C) in enumerate(((4, 40), (36, 4), (36, 40), (64, 192))):
            add(f'wgrad9/{B}x{H}x{W}-{what}/O{O_}-C{C}/acc{i & 1}', _k_wgrad('pp_conv3x3_bwd_weight', O_, C, C, B, H, W, 1, i & 1),
                ('direct', 0, W9, st))
    # -- the first layer's four instantiations (Cpad == 4, one input channel)
    for (B, H, W), st, what in (((1, 4, 4), {SLABS: 1, UNITS: 1, LAST_PX: 16}, 'one-wave-three-idle'),
                                ((1, 2, 12), {SLABS: 1, UNITS: 2, LAST_PX: 8}, 'two-waves-last-partial'),
                                ((3, 10, 12), {SLABS: 1, UNITS: 4, LAST_PX: 72}, 'four-waves-last-partial'),
                                ((3, 6, 16), {SLABS: 1, UNITS: 4, LAST_PX: 48}, 'four-waves-W16-the-16-bit-forward-takes'),
                                ((5, 18, 20), {SLABS: 2, UNITS: 8, LAST: 4, LAST_PX: 120}, 'two-blocks-eight-waves-last-partial')):
        for i, O_ in enumerate((16, 32, 48, 64)):
            add(f'wgrad_c4/{B}x{H}x{W}-{what}/O{O_}/acc{i & 1}', _k_wgrad('pp_conv3x3_bwd_weight', O_, 4, 1, B, H, W, 1, i & 1),
                ('direct', 0, C4, st))
    # -- split-fp16 halo walkers, under the default CU budget and the smallest
    halo = [(32, 32, HALO, 'one-pair'), (64, 32, HALO21, 'two-pair-2x1'), (32, 64, HALO12, 'two-pair-1x2'),
            (32, 96, HALO12, 'two-pair-1x2-half-empty-C96'), (32, 160, HALO12, 'two-pair-1x2-half-empty-C160')]
    for (B, H, W), units in (((1, 4, 32), 1), ((3, 12, 96), 27)):
        for O_, C, path, what in halo:
            for cus in ('default', 'min'):
                if cus == 'default':       # every tile its own walker, the other walkers write zeros
                    st = {UNITS: units, LIVE: units, PER: 1, LAST: 1}
                else:                       # eight walkers: one tile for walker 0 alone, or 27 tiles as 4, 4, 4, 3 ...
                    st = {UNITS: units, LIVE: min(units, 8), PER: (units + 7) // 8, LAST: 1 if units == 1 else 3, SLABS: 32 if path == HALO else 8}
                for name in ('pp_conv3x3_bwd_weight_f16x3', 'pp_conv3x3_bwd_weight_f16x3_lazy'):
                    acc = int(cus == 'min')
                    add(f'{name[11:]}/{what}/{B}x{H}x{W}-{units}-tiles/cus-{cus}/acc{acc}', _k_wgrad(name, O_, C, C, B, H, W, 1, acc),
                        ('direct', 1, path, st))
    add('bwd_weight_f16x3/H-not-a-multiple-of-4-falls-back-to-fp32-kernels', _k_wgrad('pp_conv3x3_bwd_weight_f16x3', 32, 32, 32, 3, 10, 96, 1, 0),
        ('direct', 1, T32, {SLABS: 6, PER: 4, LAST: 3, UNITS: 23}))
    # -- Winograd weight gradient: fp32 on every geometry, the split-fp16 twin on the F(4x4) ones; kept V and own V
    for what, (g, tile, splits, st) in WINO_EDGES.items():
        for name in ('pp_conv3x3_wino_bwd_weight',) + (('pp_conv3x3_wino_bwd_weight_f16x3',) if tile == 4 else ()):
            for vc in (0, 1):
                add(f'{name[11:]}/{what}/{"kept" if vc else "own"}-V/acc{1 - vc}', _k_wino_wgrad(name, *g, 1 - vc, vc), ('wino', g, tile, splits, st))
    # -- ConvTranspose weight gradient (ct_splits), with the forward and data gradient of the same geometry
    for what, (g, plan) in CT_EDGES.items():
        ch = (4, 4) if plan[0] == 64 else (36, 20)           # the cap row: the narrowest channels that keep the rows aligned
        for acc in ((0,) if plan[0] == 64 else (0, 1)):
            add(f'convtranspose_bwd_weight/{what}/acc{acc}', _k_ct('pp_convtranspose_bwd_weight', *ch, 2, *g, acc), ('ct', g, plan))
        if plan[0] != 64:
            add(f'convtranspose_fwd/{what}', _k_ct('pp_convtranspose_fwd', *ch, 2, *g), None)
            add(f'convtranspose_bwd_data/{what}', _k_ct('pp_convtranspose_bwd_data', *ch, 2, *g, 1), None)
    # -- forward, BatchNorm epilogues and data gradient at EVERY geometry of the weight-gradient rows above, in the family
    # convop.select picks for it (restated in _family so that the table needs no library while it is collected; every row
    # asserts that convop.select agrees).  What an entry's argument check refuses is listed in REJECTED, nothing is left out.
    same = [(_family(*g[:3], *g[4:]),) + g for g in geos]
    for fam, O_, C, I, B, H, W, dil in same:
        geo = f'{fam}/O{O_}-C{C}/{B}x{H}x{W}/dil{dil}'
        exp = ('family', fam, O_, C, I, H, W, dil)
        add(f'fwd/{geo}', _k_fwd(fam, O_, C, B, H, W, dil), exp)
        add(f'fwd_bn/{geo}/train-statistics', _k_fwd_bn(fam, O_, C, B, H, W, dil, 1), exp)
        add(f'fwd_bn/{geo}/eval-epilogue', _k_fwd_bn(fam, O_, C, B, H, W, dil, 2), exp)
        if I == C:          # (the first layer has no data gradient)
            for acc in (0, 1):
                add(f'bwd_data/{geo}/acc{acc}', _k_bwd_data(fam, O_, C, B, H, W, dil, acc), exp)
    # -- the fp32 Winograd GEMM at an F(4x4) geometry (what convop.select takes there with the split-fp16 GEMMs switched off)
    for what, g in (('1x16x16/dil1', (64, 256, 1, 16, 16, 1)), ('5x44x44/dil1', (128, 256, 5, 44, 44, 1))):
        add(f'fwd/wino-fp32-gemm-tile4/O{g[0]}-C{g[1]}/{what}', _k_fwd('wino', *g), ('tile', g[3:], 4))
        add(f'bwd_data/wino-fp32-gemm-tile4/O{g[0]}-C{g[1]}/{what}/acc1', _k_bwd_data('wino', *g, 1), ('tile', g[3:], 4))
    # -- shapes an entry's argument check refuses (REJECTED): a dilation-2 image whose half is odd has no Winograd form
    add('fwd/wino/O64-C256/3x6x10/dil2-rejected', _k_fwd('wino', 64, 256, 3, 6, 10, 2), None)
    add('bwd_data/wino/O64-C256/3x6x10/dil2-rejected', _k_bwd_data('wino', 64, 256, 3, 6, 10, 2, 0), None)
    return cases, expect


EDGES, EDGE_EXPECT = _edge_cases()
# (tag, storage) -> error code of the entry's argument check (PP_ERR_ARG = -1, PP_ERR_UNSUPPORTED = -2); no weight-gradient row
# may be here.  The 16-bit builds of pp_conv3x3_fwd[_bn] have the first-layer kernel only, which wants W % 16 == 0.
REJECTED = {('fwd/wino/O64-C256/3x6x10/dil2-rejected', 'fp32'): -1, ('bwd_data/wino/O64-C256/3x6x10/dil2-rejected', 'fp32'): -1}
REJECTED.update({(t, s): -2 for s in ('fp16', 'bf16')
                 for t in ('fwd/fp32/O16-C4/5x18x20/dil1', 'fwd_bn/fp32/O16-C4/5x18x20/dil1/train-statistics')})
# one row per path in fp16 and bf16 storage as well (the twin logic of replay()); 16-bit storage has neither the fp32 Winograd
# forms nor ConvTranspose, and runs the generic plan where fp32 storage runs wgrad9.  The lazy weight-gradient rows stay fp32:
# 16-bit plans do not take that form (engine.LAZY_HALO_H16), and the twin logic has no reference for it -- the kernel stages
# y = lrelu(z * scale + shift) as fp16 without ever storing it, the twin's float64 reference sees y unrounded (measured on the
# 3x12x96 two-pair row: dw 1.7e-4 / 2.3e-4 of the largest gradient in fp16 / bf16 storage, the size of that rounding).
H16_ROWS = (
    'wgrad/tile32/O32-C32/4-splits-uneven-last-16px-chunk/dil2/acc1', 'wgrad/tile64/O64-C64/4-splits-uneven-last-16px-chunk/dil1/acc0',
    'wgrad/tile128/O128-C128/4-splits-uneven-last-16px-chunk/dil2/acc1', 'wgrad9/5x7x64-3-splits-last-11-boundaries-inside-images/O36-C40/acc0',
    'wgrad_c4/5x18x20-two-blocks-eight-waves-last-partial/O48/acc0', 'bwd_weight_f16x3/one-pair/3x12x96-27-tiles/cus-min/acc1',
    'bwd_weight_f16x3/two-pair-2x1/3x12x96-27-tiles/cus-default/acc0', 'bwd_weight_f16x3/two-pair-1x2-half-empty-C96/3x12x96-27-tiles/cus-min/acc1',
    'bwd_weight_f16x3/H-not-a-multiple-of-4-falls-back-to-fp32-kernels',
    'wino_bwd_weight_f16x3/tile4-bm128-uneven-split-partial-chunk-B5/kept-V/acc0', 'wino_bwd_weight_f16x3/tile4-dil2-odd-7x7-tiles-bm64-uneven-split-B3/own-V/acc1',
    'fwd/f16x3/O64-C96/3x20x28/dil2', 'fwd_bn/f16x3/O32-C160/3x12x96/dil1/train-statistics', 'fwd_bn/f16x3/O32-C160/3x12x96/dil1/eval-epilogue',
    'bwd_data/f16x3/O192-C64/3x20x28/dil2/acc1', 'fwd/fp32/O16-C4/5x18x20/dil1', 'fwd_bn/fp32/O16-C4/5x18x20/dil1/train-statistics',
    'fwd/fp32/O48-C4/3x6x16/dil1', 'fwd_bn/fp32/O48-C4/3x6x16/dil1/train-statistics', 'fwd_bn/fp32/O48-C4/3x6x16/dil1/eval-epilogue',
    'fwd/wino-split/O128-C256/5x44x44/dil1', 'fwd_bn/wino-split/O64-C256/3x56x56/dil2/train-statistics', 'bwd_data/wino-split/O128-C256/5x44x44/dil1/acc1',
)
_EDGE_OF = dict(EDGES)
EDGE_PARAMS = [(t, l, 'fp32') for t, l in EDGES] + [(t, _EDGE_OF[t], s) for t in H16_ROWS for s in ('fp16', 'bf16')]


def _assert_plan(tag, launch, storage):
    """The state the row's tag names, through the library's plan queries (host-only)."""
    from types import SimpleNamespace
    from pacingpseudo_amd import convop
    from pacingpseudo_amd._lib import lib
    exp = EDGE_EXPECT[tag]
    name, a = launch
    if exp is None:
        return
    if exp[0] == 'direct':
        _, f16x3, path, st = exp
        O_, C, B, H, W, dil = a[2], a[5], a[7], a[8], a[9], a[10]
        out = (ctypes.c_int * 6)()
        got = lib.pp_conv3x3_bwd_weight_plan(O_, C, B, H, W, dil, f16x3, out)
        assert got == path, f'{tag}: path {got}, expected {path} (plan {list(out)})'
        assert all(out[i] == v for i, v in st.items()), f'{tag}: plan {list(out)}, expected {st}'
        if path in (HALO, HALO21, HALO12) and 'cus-default' in tag:
            walkers = out[SLABS] // 4 if path == HALO else out[SLABS]         # a one-pair walker leaves four slabs
            assert walkers > out[LIVE], f'{tag}: every one of {walkers} walkers has a tile ({list(out)})'      # idle walkers exist
    elif exp[0] == 'wino':
        _, g, tile, splits, st = exp
        assert (a[2], a[5]) + tuple(a[6:10]) == g
        out = (ctypes.c_int * 6)()
        assert lib.pp_conv3x3_wino_tile(*g[3:]) == tile, tag
        assert lib.pp_conv3x3_wino_bwd_weight_plan(*g, out) == splits == lib.pp_conv3x3_wino_bwd_weight_splits(*g), f'{tag}: {list(out)}'
        assert all(out[i] == v for i, v in st.items()), f'{tag}: plan {list(out)}, expected {st}'
    elif exp[0] == 'ct':
        _, g, plan = exp
        assert tuple(a[7:10]) == g
        out = (ctypes.c_int * 2)()
        assert (lib.pp_convtranspose_bwd_weight_splits(*g, out), out[0], out[1]) == plan, f'{tag}: {list(out)}'
    elif exp[0] == 'tile':
        assert lib.pp_conv3x3_wino_tile(*exp[1]) == exp[2], tag
    else:
        _, fam, O_, C, I, H, W, dil = exp
        L = SimpleNamespace(name=tag, cin=I, cin_pad=C, cout=O_, dil=dil, stride=1)
        sel = convop.select(L, H, W, storage != 'fp32')
        kind = {'wino': 'wino-split' if sel.split else 'wino'}.get(sel.kind, sel.kind)
        assert kind == fam, f'{tag}: convop.select takes {sel}, the row is written for {fam}'


def test_edge_table_is_well_formed():
    """REJECTED is explicit and holds no weight-gradient row; every other row has its expectation; every 16-bit row exists."""
    for tag, storage in REJECTED:
        assert (tag, _EDGE_OF[tag], storage) in EDGE_PARAMS and 'bwd_weight' not in _EDGE_OF[tag][0] and 'wgrad' not in tag, tag
    for tag, (name, _) in EDGES:
        assert name in ADAPTERS, name
        assert (EDGE_EXPECT[tag] is not None) or (tag, 'fp32') in REJECTED or name in ('pp_convtranspose_fwd', 'pp_convtranspose_bwd_data'), tag
        if 'bwd_weight' in name:
            assert EDGE_EXPECT[tag][0] in ('direct', 'wino', 'ct'), tag


@pytest.mark.parametrize('tag,launch,storage', EDGE_PARAMS, ids=[f'{t}-{s}' for t, _, s in EDGE_PARAMS])
def test_edge_launch_matches_float64(tag, launch, storage):
    """One hand-made launch at a state of its plan, asserted through the plan queries, then replayed against float64 (fp32
    storage) or the fp32 twin (16-bit storage) at the tolerances of the census."""
    from pacingpseudo_amd._lib import HipLibraryError, lib
    prev = lib.pp_get_wgrad_cus()
    try:
        if 'cus-min' in tag:
            lib.pp_set_wgrad_cus(MIN_CUS)
        _assert_plan(tag, launch, storage)
        if (tag, storage) in REJECTED:
            with pytest.raises(HipLibraryError) as e:
                replay((storage,) + launch)
            assert f'rc={REJECTED[(tag, storage)]})' in str(e.value), str(e.value)
            return
        res = replay((storage,) + launch)
    finally:
        lib.pp_set_wgrad_cus(prev)
    bad = [(lab, r) for lab, r in res if not r <= 1.0]
    print(f'{tag} [{storage}] {launch[0]}: worst error / tolerance {max(r for _, r in res):.3g}')
    assert not bad, f'{tag} [{storage}] args={launch[1]}: ' + ', '.join(f'{lab} {r:.3g} x tol' for lab, r in bad)


# ------------------------------------------------------------------------------------------------------ the gate bites
class _Planted:
    """An entry-point table that calls ONE entry point wrongly (`wrong(fn, args)` makes the call), everything else unchanged."""

    def __init__(self, inner, name, wrong):
        self._inner, self._name, self._wrong = inner, name, wrong

    def __getattr__(self, n):
        fn = getattr(self._inner, n)
        if n != self._name:
            return fn
        return lambda *a: self._wrong(fn, list(a))


def _set(i, value):
    def wrong(fn, a):
        a[i] = value
        return fn(*a)
    return wrong


def _i_true_is_cpad(fn, a):
    """pp_conv3x3_bwd_weight with I_true = Cpad: the gradient in the (O, Cpad, 3, 3) layout.  It goes to a buffer of that size;
    the caller's (O, I, 3, 3) buffer receives what it would have held (the leading O * I * 9 floats): nothing is written outside."""
    lib = _L()
    O_, Cpad, I = a[2], a[5], a[6]
    big = _zeros(O_ * Cpad * 9)
    dw, a[6], a[11] = a[11], Cpad, big.data_ptr()
    rc = fn(*a)
    n = O_ * I * 9
    lib.pp_copy_slab(big.data_ptr(), n, dw, n, n, 1, 0, a[-1])
    torch.cuda.synchronize()
    return rc


def _other_x(fn, a):
    """the Winograd forward that fills the kept V, run on another tensor of the same extent"""
    B, H, W = a[8], a[9], a[10]
    other = _b(torch.randn(B * H * W * a[1], generator=torch.Generator().manual_seed(5)))
    a[0] = other.data_ptr()
    rc = fn(*a)
    torch.cuda.synchronize()
    return rc


def _stale_amax(fn, a):
    """max |dz| of an earlier, 2^8 times smaller dz: the split-fp16 operands leave the fp16 range"""
    lib = _L()
    lib.pp_scale(a[-2], 1, 2.0 ** -8, a[-1])
    rc = fn(*a)
    lib.pp_scale(a[-2], 1, 2.0 ** 8, a[-1])
    return rc


PLANTS = {
    # tag of an edge row, entry point called wrongly, how, labels that must leave the tolerance; every planted call stays inside
    # the buffers the adapter allocated
    'accumulate-flipped': ('wgrad/tile32/O32-C32/4-splits-uneven-last-16px-chunk/dil1/acc1', 'pp_conv3x3_bwd_weight', _set(12, 0), ('dw',)),
    'dilation-2-run-as-1': ('fwd/f16x3/O32-C32/3x20x28/dil2', 'pp_conv3x3_fwd_f16x3', _set(11, 1), ('y',)),
    'I_true-passed-as-Cpad': ('wgrad_c4/5x18x20-two-blocks-eight-waves-last-partial/O16/acc0', 'pp_conv3x3_bwd_weight', _i_true_is_cpad, ('dw',)),
    'kept-V-of-another-x': ('wino_bwd_weight/tile4-bm64-one-split-one-partial-chunk-B1/kept-V/acc0', 'pp_conv3x3_wino_fwd', _other_x, ('dw',)),
    'dz_amax-stale-by-2^8': ('bwd_weight_f16x3/one-pair/3x12x96-27-tiles/cus-default/acc0', 'pp_conv3x3_bwd_weight_f16x3', _stale_amax, ('dw',)),
    'weight-pack-of-the-other-tile': ('fwd/wino-fp32-gemm-tile4/O64-C256/1x16x16/dil1', 'pp_wino_pack_weights', _set(3, 2), ('y',)),
}


@pytest.mark.parametrize('plant', sorted(PLANTS))
def test_planted_mistake_fails_the_replay(plant):
    """The same replay with an entry-point table that makes one mistake must leave the tolerance on the named label (NaN counts,
    as it does in the gate); with the honest table the same launch passes."""
    from pacingpseudo_amd._lib import lib
    tag, entry, wrong, must_fail = PLANTS[plant]
    key = ('fp32',) + _EDGE_OF[tag]
    honest = dict(replay(key))
    assert all(r <= 1.0 for r in honest.values()), honest
    assert sum(label.endswith(' band') for label in honest) >= 2, 'no sentinel-band verdicts in the replay (an input and an output at least)'
    planted = dict(replay(key, table=_Planted(lib, entry, wrong)))
    for label in must_fail:
        assert not planted[label] <= 1.0, (plant, label, planted)
