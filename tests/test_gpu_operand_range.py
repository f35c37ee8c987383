"""The operand-magnitude envelope of the split-fp16 convolutions (docs/operand_range.md).

The censuses replay every convolution launch against float64 at ONE magnitude per operand kind (activations randn, weights
randn / sqrt(9 C), gradients 1e-7 in fp32 storage and 1e-2 in 16-bit storage).  Here the magnitudes move, on one smallest shape per
kernel family, through the same adapters (tests/test_gpu_conv_census.py: _Ops / Profile, _Run, the adapters, TOL, _rel, _act_ratio):
  A  gradient operands are scale-equivariant: dz * 2^k with the cell * 2^k gives 2^k times the result, bit for bit;
  B  an all-zero dz gives exact zeros, a vanishing one (max |dz| = 2^-120, 2^-130, 2^-145) finite results within
     TOL * max |ref| + 2^-126 of float64;
  C  dz whose output channels span 2^0 ... 2^-12: the weight gradient holds TOL PER OUTPUT CHANNEL;
  D  the fixed-scale forward operands hold TOL for activations of scale 2^-10 ... 2^10 and weights of 2^-6 ... 2^6; the Winograd
     input transform saturates (finite results at 2^20);
  E  in a real step, the max |dz| cell every split-fp16 gradient launch is handed equals the maximum of the dz it is handed.
The tolerances of C and D follow from the number formats (tests/test_operand_range.py holds the emulation); what lies outside the
declared envelope is measured by `python -m tests.test_gpu_operand_range` and written down in docs/operand_range.md, not asserted.

Which kernel a row reaches: the weight-gradient rows assert it through the library's plan queries; the forward / data-gradient
kernels of conv_dispatch_f16x3 (pp_conv.hip) have no query, so each row cites the dispatch condition; every row asserts the family
through convop.select.
"""
import ctypes
import sys
from types import SimpleNamespace

import pytest
import torch

from tests import test_gpu_conv_census as C
from tests.test_gpu_conv_census import CENSUS, HALO, HALO21, TOL, Profile, operands

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ rows
HALO_G = (3, 12, 96)            # the 27-tile halo geometry of EDGES
G0 = C.G0                       # (3, 20, 28): W % 32 != 0, so no halo kernel: the implicit GEMM by N % 128 / N % 64 / else
WINO_FULL = (256, 256, 8, 64, 64, 1)      # (O, C, B, H, W, dil): 2048 tiles; neither table has a shape the persistent GEMM takes
WINO_RAGGED = C.WINO_EDGES['tile4-bm64-one-split-one-partial-chunk-B1'][0]         # (64, 256, 1, 16, 16, 1): 16 tiles

# Direct kernels: (output channels O, input channels Cin, (B, H, W)), dilation 1.  conv_dispatch_f16x3 sees C = Cin, N = O in
# the forward and C = O (the channels of dz), N = Cin in the data gradient; with fp32 storage it takes
#   the two-half halo kernel   dil 1, W % 32 == 0, H % 4 == 0, C % 32 == 0, C <= 64, N % 32 == 0, N <= 192 (halo2_ok: weights +
#                              two patches within 160 KB), one row per wave (two rows exist in the 16-bit build only: H16_ROWS)
#   the one-half halo kernel   the same with C == 96
#   split-K halo launches      128 < C <= 192, C % 64 == 0: C / 64 accumulating launches of the two-half kernel
#   the implicit GEMM          otherwise: 128 x 128 for N % 128 == 0, 128 x 64 for N % 64 == 0, else 128 x 32
FWD_ROWS = {
    'halo2-one-row-per-wave': (32, 32, HALO_G),
    'halo-one-half-C96': (32, 96, HALO_G),
    'halo2-split-k-C192-to-64': (64, 192, (2, 32, 64)),           # F16X3_CASES (2, 32, 64, 192, 64, 1)
    'igemm-128x128': (128, 128, G0),
    'igemm-128x64': (64, 64, G0),
    'igemm-128x32': (32, 32, G0),
}
BWD_DATA_ROWS = {
    'halo2-one-row-per-wave': (32, 32, HALO_G),
    'halo-one-half-O96': (96, 64, (3, 20, 96)),                   # F16X3_CASES (3, 20, 96, 64, 96, 1)
    'halo2-split-k-O192-to-64': (192, 64, (2, 8, 64)),            # F16X3_CASES (2, 8, 64, 64, 192, 1)
    'igemm-128x128': (128, 128, G0),
    'igemm-128x64': (64, 64, G0),
    'igemm-128x32': (32, 32, G0),
}
# Direct weight gradient: (O, C, (B, H, W), PP_WGRAD_PATH_* the plan query must return)
WGRAD_ROWS = {
    'halo-one-pair': (32, 32, HALO_G, HALO),
    'halo-two-pair': (64, 32, HALO_G, HALO21),
}
WINO_ROWS = {'persistent-gemm-full-tiles': WINO_FULL, 'round-3-gemm-ragged-tiles': WINO_RAGGED}


def _select(O_, Cin, H, W, dil, h16=False):
    from pacingpseudo_amd import convop
    return convop.select(SimpleNamespace(name='row', cin=Cin, cin_pad=Cin, cout=O_, dil=dil, stride=1), H, W, h16)


def _assert_direct(O_, Cin, g, dil=1, h16=False):
    sel = _select(O_, Cin, g[1], g[2], dil, h16)
    assert sel.kind == 'f16x3', sel


def _assert_wino(g, h16=False):
    """The split-fp16 F(4x4) family, and which GEMM launch_gemm_ps takes: the persistent kernel needs M % 128 == 0 (M = tiles),
    N % 256 == 0, K >= 128 and 36 * (M / 128) * (N / 256) >= 512 blocks' worth of tiles."""
    O_, Cin, B, H, W, dil = g
    sel = _select(O_, Cin, H, W, dil, h16)
    assert sel.kind == 'wino' and sel.tile == 4 and sel.split, sel
    tiles = B * (H // (4 * dil)) * (W // (4 * dil)) * dil * dil
    full = [tiles % 128 == 0 and n % 256 == 0 and k >= 128 and 36 * (tiles // 128) * (n // 256) >= 512 for n, k in ((O_, Cin), (Cin, O_))]
    assert all(full) == (g == WINO_FULL) and any(full) == (g == WINO_FULL), (g, tiles, full)


def _assert_wgrad(O_, Cin, g, path):
    from pacingpseudo_amd._lib import lib
    _assert_direct(O_, Cin, g)
    out = (ctypes.c_int * 6)()
    got = lib.pp_conv3x3_bwd_weight_plan(O_, Cin, *g, 1, 1, out)
    assert got == path, f'path {got}, expected {path} (plan {list(out)})'


def _grad_rows():
    """[(id, launch, plan assertion)] of every gradient entry at accumulate = 0, fp32 storage."""
    rows = []
    for tag, (O_, Cin, g) in BWD_DATA_ROWS.items():
        rows.append((f'bwd_data/{tag}', C._k_bwd_data('f16x3', O_, Cin, *g, 1, 0), lambda O_=O_, Cin=Cin, g=g: _assert_direct(O_, Cin, g)))
    for tag, (O_, Cin, g, path) in WGRAD_ROWS.items():
        for name in ('pp_conv3x3_bwd_weight_f16x3', 'pp_conv3x3_bwd_weight_f16x3_lazy'):
            rows.append((f'{name[11:]}/{tag}', C._k_wgrad(name, O_, Cin, Cin, *g, 1, 0),
                         lambda O_=O_, Cin=Cin, g=g, path=path: _assert_wgrad(O_, Cin, g, path)))
    for tag, g in WINO_ROWS.items():
        rows.append((f'wino_bwd_data/{tag}', C._k_bwd_data('wino-split', *g, 0), lambda g=g: _assert_wino(g)))
        for vc in (1, 0):
            rows.append((f'wino_bwd_weight/{tag}/{"kept" if vc else "own"}-V',
                         C._k_wino_wgrad('pp_conv3x3_wino_bwd_weight_f16x3', *g, 0, vc), lambda g=g: _assert_wino(g)))
    return rows


def _fwd_rows():
    """[(id, launch, plan assertion)] of the forward and fwd_bn entries (fp32 storage)."""
    rows = []
    for tag, (O_, Cin, g) in FWD_ROWS.items():
        check = lambda O_=O_, Cin=Cin, g=g: _assert_direct(O_, Cin, g)       # noqa: E731
        rows.append((f'fwd/{tag}', C._k_fwd('f16x3', O_, Cin, *g, 1), check))
        rows.append((f'fwd_bn/{tag}/train-statistics', C._k_fwd_bn('f16x3', O_, Cin, *g, 1, 1), check))
        rows.append((f'fwd_bn/{tag}/eval-epilogue', C._k_fwd_bn('f16x3', O_, Cin, *g, 1, 2), check))
    for tag, g in WINO_ROWS.items():
        check = lambda g=g: _assert_wino(g)       # noqa: E731
        rows.append((f'wino_fwd/{tag}', C._k_fwd('wino-split', *g), check))
        rows.append((f'wino_fwd_bn/{tag}/train-statistics', C._k_fwd_bn('wino-split', *g, 1), check))
        rows.append((f'wino_fwd_bn/{tag}/eval-epilogue', C._k_fwd_bn('wino-split', *g, 2), check))
    return rows


# 16-bit storage: the split-fp16 gradient rows of H16_ROWS at accumulate = 0 (the fp32-kernel fall-back row is no split-fp16 launch),
# and the two-rows-per-wave form of the two-half halo kernel, which only the 16-bit build has (halo2_ok: H % 8 == 0, C <= 64):
# the data gradient of F16X3_CASES (2, 8, 64, 96, 32, 1), dz of 32 channels.
def _h16_rows():
    rows = [('bwd_data/igemm-128x64-O192-C64-dil2', C._k_bwd_data('f16x3', 192, 64, *G0, 2, 0), lambda h: _assert_direct(192, 64, G0, 2, h)),
            ('bwd_data/halo2-two-rows-per-wave', C._k_bwd_data('f16x3', 32, 96, 2, 8, 64, 1, 0), lambda h: _assert_direct(32, 96, (2, 8, 64), 1, h)),
            ('wino_bwd_data/O128-C256-5x44x44', C._k_bwd_data('wino-split', 128, 256, 5, 44, 44, 1, 0),
             lambda h: _assert_wino((128, 256, 5, 44, 44, 1), h))]
    for tag, O_, Cin, path in (('one-pair', 32, 32, HALO), ('two-pair-2x1', 64, 32, HALO21), ('two-pair-1x2-half-empty-C96', 32, 96, C.HALO12)):
        rows.append((f'bwd_weight_f16x3/{tag}', C._k_wgrad('pp_conv3x3_bwd_weight_f16x3', O_, Cin, Cin, *HALO_G, 1, 0),
                     lambda h, O_=O_, Cin=Cin, path=path: _assert_wgrad(O_, Cin, HALO_G, path)))
    rows.append(('wino_bwd_weight/bm128-uneven-split-B5/kept-V', C._k_wino_wgrad('pp_conv3x3_wino_bwd_weight_f16x3', 128, 256, 5, 44, 44, 1, 0, 1),
                 lambda h: _assert_wino((128, 256, 5, 44, 44, 1), h)))
    rows.append(('wino_bwd_weight/dil2-odd-7x7-tiles-B3/own-V', C._k_wino_wgrad('pp_conv3x3_wino_bwd_weight_f16x3', 64, 256, 3, 56, 56, 2, 0, 0),
                 lambda h: _assert_wino((64, 256, 3, 56, 56, 2), h)))
    return rows


GRAD_ROWS, FWD, H16 = _grad_rows(), _fwd_rows(), _h16_rows()
_ids = lambda rows: [r[0] for r in rows]          # noqa: E731


# ------------------------------------------------------------------------------------------------------------------ running
def _launch(storage, launch, profile, want_ref=True):
    """One execution of a launch on operands of `profile`: {label: (device result, float64 reference or None)}; the canaries and
    sentinel bands of the run are asserted here."""
    from pacingpseudo_amd._lib import lib, lib_for
    key = (storage,) + launch
    K, dt = (lib, torch.float32) if storage == 'fp32' else (lib_for(storage), C.MANT[storage][2])
    run = C._Run(K, dt, want_ref)
    with operands(profile):
        C._execute(C.ADAPTERS[launch[0]], key, run)
    broken = [label for label, got, ok, _, _ in run.res if got is None and not ok]
    assert not broken, f'{launch[0]} {profile}: {broken}'
    return {label: (got, ref) for label, got, ref, _, _ in run.res if got is not None}


def _ratios(storage, launch, profile):
    """replay() of the census under a profile: {label: error / tolerance}"""
    with operands(profile):
        return dict(C.replay((storage,) + launch))


def _bad(ratios):
    return {label: f'{r:.3g}' for label, r in ratios.items() if not r <= 1.0}


def _worst(ratios):
    """the largest error / tolerance of a replay; NaN counts as inf"""
    return max(float('inf') if r != r else r for r in ratios.values())


# ------------------------------------------------------------------------- A: gradient operands are scale-equivariant
K_FP32 = (-60, -20, -1, 1, 20, 60)           # around G_FP32 = 1e-7 ~ 2^-23: max |dz| from 2^-81 to 2^39, inside [2^-100, 2^100]
K_16 = (-9, -4, -1, 1, 7, 14)                # |dz| in [2^-4, 1] at k = 0: a normal fp16 number from 2^-13 to 2^14


@pytest.mark.parametrize('tag,launch,plan', GRAD_ROWS, ids=_ids(GRAD_ROWS))
def test_gradient_scale_equivariance(tag, launch, plan):
    """result(dz * 2^k, cell * 2^k) == 2^k * result(dz, cell), bit for bit: the operand scale is a power of two, the accumulators
    are fp32 and the epilogue multiplies by a power of two.  No row of this table is exempt.  The two extreme k also against
    float64 at TOL."""
    plan()
    base = _launch('fp32', launch, CENSUS, want_ref=False)
    (label, (r0, _)), = base.items()
    r0 = r0.cpu()
    for k in K_FP32:
        extreme = k in (K_FP32[0], K_FP32[-1])
        got, ref = _launch('fp32', launch, Profile(pow2=k), want_ref=extreme)[label]
        want = r0 * 2.0 ** k                # on the host, in fp32: exact
        assert torch.equal(got.cpu(), want), (f'{tag} {label} at k = {k}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ, '
                                              f'largest difference {float((got.cpu().double() - want.double()).abs().max() / want.abs().max()):.3g} of the maximum')
        if extreme:
            rel = C._rel(got, ref)
            print(f'{tag} {label} k = {k}: error / tolerance {rel / TOL:.3g}')
            assert rel <= TOL, (tag, label, k, rel)


def _equal_16(got, base, k, storage):
    """2^k * base == got for results of a 16-bit storage launch.  fp32 results (weight gradients) and bf16 results: bit for bit.
    An fp16 result is the fp32 value v rounded to fp16: rne(v * 2^k) == 2^k * rne(v) wherever both lie in fp16's normal range;
    an element that is subnormal (below 2^-14) in either run was rounded to a multiple of 2^-24 there, which the other run
    does not reproduce: those may differ by 2^-24 * max(1, 2^k); beyond 65504 both must have overflowed."""
    g, w = got.float().cpu(), base.float().cpu() * 2.0 ** k
    if got.dtype != torch.float16:
        return torch.equal(g, w)
    tiny = (w.abs() < 2.0 ** -14) | (base.float().cpu().abs() < 2.0 ** -14)
    over = w.abs() > 65504
    normal = ~tiny & ~over
    return (torch.equal(g[normal], w[normal]) and bool(((g[tiny] - w[tiny]).abs() <= 2.0 ** -24 * max(1.0, 2.0 ** k)).all())
            and bool((g[over].abs() >= 65504).all()))


@pytest.mark.parametrize('storage', ('fp16', 'bf16'))
@pytest.mark.parametrize('tag,launch,plan', H16, ids=_ids(H16))
def test_gradient_scale_equivariance_16bit(tag, launch, plan, storage):
    """The same in 16-bit storage, on a dz of magnitudes in [2^-4, 1] (normal in fp16 at every k of the sweep).  The weights of
    the data-gradient rows are scaled by 2^-2, which keeps dx of the largest k inside fp16.  Exempt from bit-equality: the
    subnormal elements of an fp16 dx (_equal_16).  The extreme k against the fp32 twin / float64 as the census does."""
    plan(True)
    prof = Profile(unit=True, grad=1.0, weight=0.25 if 'bwd_data' in tag else 1.0)
    base = _launch(storage, launch, prof, want_ref=False)
    (label, (r0, _)), = base.items()
    for k in K_16:
        got, _ = _launch(storage, launch, prof._replace(pow2=k), want_ref=False)[label]
        assert _equal_16(got, r0, k, storage), f'{tag} [{storage}] {label} at k = {k}'
    for k in (K_16[0], K_16[-1]):
        res = _ratios(storage, launch, prof._replace(pow2=k))
        print(f'{tag} [{storage}] k = {k}: worst error / tolerance {_worst(res):.3g}')
        assert not _bad(res), (tag, storage, k, _bad(res))


# ------------------------------------------------------------------------------------- B: vanishing and zero gradients
@pytest.mark.parametrize('tag,launch,plan', GRAD_ROWS, ids=_ids(GRAD_ROWS))
def test_zero_gradient_gives_exact_zeros(tag, launch, plan):
    plan()
    (label, (got, _)), = _launch('fp32', launch, Profile(zero=True), want_ref=False).items()
    assert int((got != 0).sum()) == 0, (tag, label)


@pytest.mark.parametrize('e', (-120, -130, -145))
@pytest.mark.parametrize('tag,launch,plan', GRAD_ROWS, ids=_ids(GRAD_ROWS))
def test_vanishing_gradient_stays_finite(tag, launch, plan, e):
    """max |dz| = 2^e, a finite fp32 number: finite results within TOL * max |ref| + 2^-126 of float64 (results in the
    subnormal range carry absolute precision).  Before f16_scales clamped its exponent the direct kernels' operand scale
    2^(10 - e) was inf here and every result NaN."""
    plan()
    (label, (got, ref)), = _launch('fp32', launch, Profile(peak=2.0 ** e)).items()
    assert bool(torch.isfinite(got).all()), f'{tag} {label}: {int((~torch.isfinite(got)).sum())} of {got.numel()} results are not finite'
    err, bound = float((got.double() - ref).abs().max()), TOL * float(ref.abs().max()) + 2.0 ** -126
    print(f'{tag} {label} max |dz| = 2^{e}: error {err:.3g}, bound {bound:.3g}, max |ref| {float(ref.abs().max()):.3g}')
    assert err <= bound, (tag, label, e, err, bound)


# ----------------------------------------------------------------------------------- C: channels of unequal magnitude
def _channel_errors(got, ref):
    """relative error per output channel of a weight gradient (O, I, 3, 3): max norm over the channel's slice"""
    d = (got.double() - ref).abs().flatten(1).max(1).values
    return d / ref.abs().flatten(1).max(1).values


WGRADS = [r for r in GRAD_ROWS if 'bwd_weight' in r[0]]
DGRADS = [r for r in GRAD_ROWS if 'bwd_data' in r[0]]


@pytest.mark.parametrize('tag,launch,plan', WGRADS, ids=_ids(WGRADS))
def test_weight_gradient_per_channel_with_spread_2_12(tag, launch, plan):
    """Output channel c of dz is scaled by 2^(-12 c / (O - 1)), the cell holds the true maximum.  The direct kernels stage the low
    part of dz unscaled: a channel 2^j below the maximum keeps 22 significant bits down to j = 12 (tests/test_operand_range.py),
    so every channel's own gradient holds TOL -- a whole-tensor max norm would not see the small channels at all."""
    plan()
    (label, (got, ref)), = _launch('fp32', launch, Profile(spread=12)).items()
    err = _channel_errors(got, ref)
    print(f'{tag}: worst per-channel error / tolerance {float(err.max()) / TOL:.3g} (channel {int(err.argmax())} of {err.numel()})')
    assert float(err.max()) <= TOL, (tag, [f'{float(e):.3g}' for e in err])


@pytest.mark.parametrize('tag,launch,plan', DGRADS, ids=_ids(DGRADS))
def test_data_gradient_with_spread_2_12(tag, launch, plan):
    """The same dz against weights scaled by the inverse spread per output channel: every channel contributes alike to dx."""
    plan()
    (label, (got, ref)), = _launch('fp32', launch, Profile(spread=12, balance=True)).items()
    rel = C._rel(got, ref)
    print(f'{tag}: error / tolerance {rel / TOL:.3g}')
    assert rel <= TOL, (tag, rel)


# ------------------------------------------------------------------------- D: fixed-scale operands, the declared envelope
ACT_K = (-10, -5, 0, 5, 10)       # activations are post-normalisation values: O(1); the split is flat from 2^-14 to 2^13
WEIGHT_K = (-6, 6)


@pytest.mark.parametrize('tag,launch,plan', FWD, ids=_ids(FWD))
def test_forward_inside_the_declared_envelope(tag, launch, plan):
    """Activations scaled by 2^-10 ... 2^10 and weights by 2^-6 ... 2^6 hold the census tolerances (TOL, TOL_SUMS for the
    statistics rows) against float64."""
    plan()
    for prof in [Profile(act=2.0 ** k) for k in ACT_K] + [Profile(weight=2.0 ** k) for k in WEIGHT_K]:
        res = _ratios('fp32', launch, prof)
        print(f'{tag} act {prof.act:g} weight {prof.weight:g}: worst error / tolerance {_worst(res):.3g}')
        assert not _bad(res), (tag, prof, _bad(res))


WINO_FWD = [r for r in FWD if r[0].startswith('wino_fwd/')]


@pytest.mark.parametrize('tag,launch,plan', WINO_FWD, ids=_ids(WINO_FWD))
def test_winograd_forward_saturates(tag, launch, plan):
    """Activations of scale 2^20 leave the fp16 range of the fixed-scale transform-domain operands: the CLAMP form of ps_store
    saturates them, the output is wrong but finite.  (The direct kernels have no clamp: docs/operand_range.md.)"""
    plan()
    (label, (got, _)), = _launch('fp32', launch, Profile(act=2.0 ** 20), want_ref=False).items()
    assert bool(torch.isfinite(got).all()), f'{tag}: {int((~torch.isfinite(got)).sum())} of {got.numel()} outputs are not finite'


# ------------------------------------------------------------------------------ E: the cell each launch reads, in a real step
WATCHED = ('pp_conv3x3_bwd_data_f16x3', 'pp_conv3x3_bwd_weight_f16x3', 'pp_conv3x3_bwd_weight_f16x3_lazy',
           'pp_conv3x3_wino_bwd_data_f16x3', 'pp_conv3x3_wino_bwd_weight_f16x3')


class _CellProbe:
    """Stands in for a plan's entry-point table (as tests/_launch_census.py::_Recorder).  At every split-fp16 gradient launch:
    wait for the device, copy the dz view out with the table's own pp_copy_slab, read the cell the launch is handed and log
    (step, entry, layer owning the cell, cell, cell rounded to the storage type, max |dz|); the launch then goes out unchanged.
    The backward of the normalisation takes the maximum of the fp32 dz it computed and THEN stores dz in the storage type, so
    in 16-bit storage the cell is the maximum before that store (measured: cell 0.5801062, stored maximum 0.58007812 = the cell
    rounded to fp16).  Rounding is monotonic -- the largest stored value is the rounded largest value -- so the property that
    holds bit for bit in every storage is  round_to_storage(cell) == max |stored dz|;  with fp32 storage that is cell == max |dz|."""

    def __init__(self, inner, dtype, log, cells, step):
        self._inner, self._dtype, self._log, self._cells, self._step = inner, dtype, log, cells, step

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if name not in WATCHED:
            return fn

        def call(*a):
            torch.cuda.synchronize()
            B, H, W, _ = C._geom(name, a)
            O_, P = a[2], B * H * W
            dz = torch.empty(P, O_, dtype=self._dtype, device=C._dev())
            self._inner.pp_copy_slab(a[0], a[1], dz.data_ptr(), O_, O_, P, 0, a[-1])
            torch.cuda.synchronize()
            ptr = a[-3] if name.endswith('_lazy') else a[-2]
            owner, cell = self._cells().get(ptr, (f'no cell of the plan at {ptr}', None))
            stored = None if cell is None else float(cell.to(self._dtype).float())       # the cell as the storage type holds it
            self._log.append((self._step[0], name, owner, None if cell is None else float(cell), stored, float(dz.float().abs().max())))
            return fn(*a)
        return call


def _watched_steps(storage, variant, swap=False):
    """One full-flags model at the census's batch-recording size, a train-mode and an eval-mode BatchNorm step with every plan's
    table a _CellProbe.  swap: after the first step the cells of two layers' ConvOps change places (the planted mistake; the
    backward of the normalisation goes on writing each layer's own cell).  Returns the log of the steps made after that."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd import engine as E
    from tests._launch_census import BATCH_IMAGE_SIZE
    log, step, box = [], [''], []

    def cells():
        return {op.amax.data_ptr(): (name, op.amax) for p in box[0].engine.plans.values() for name, op in p.conv.items() if op.amax is not None}
    real = E.lib_for
    names = {4: 'fp32', 2: 'fp16'}
    E.lib_for = lambda s: _CellProbe(real(s), {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}[names.get(s, s)],
                                     log, cells, step)
    try:
        args = O.full_flags(num_classes=5, ignored_index=5, output_stride=8)
        args.storage = storage
        torch.manual_seed(1)
        if variant == 'gn':
            from tests.test_gpu_groupnorm import build_gn_model
            model = build_gn_model(args)
        else:
            from tests.test_gpu_step import build_model
            model = build_model(args)
        box.append(model)
        s = BATCH_IMAGE_SIZE
        batch = {k: v.cuda() for k, v in O.synthetic_batch(3, s, s, num_classes=5, seed=7, keep=0.03).items() if k != 'label'}
        swapped = None
        for bn_eval in (False, True) + ((True,) if swap else ()):
            step[0] = f'{"eval" if bn_eval else "train"}-BN'
            model.train()
            if bn_eval:
                model.eval()
            model.zero_grad(set_to_none=True)
            out = model(batch, mode='train', step=0)
            loss = sum(out[k] * wt for k, wt in O.loss_weights(args, 0).items())
            loss.backward()
            torch.cuda.synchronize()
            if swap and bn_eval and swapped is None:
                plan = next(p for p in model.engine.plans.values() if any(op.amax is not None for op in p.conv.values()))
                seen = [line[2] for line in log]
                a, b = [n for n, op in plan.conv.items() if op.amax is not None and n in seen][:2]
                plan.conv[a].amax, plan.conv[b].amax = plan.conv[b].amax, plan.conv[a].amax
                swapped = (a, b)
                del log[:]
    finally:
        E.lib_for = real
    return log, swapped


def _mismatches(log):
    return [line for line in log if line[4] is None or line[4] != line[5]]


@pytest.mark.parametrize('storage,variant', [('fp32', ''), ('fp16', ''), ('fp32', 'gn')], ids=['fp32', 'fp16', 'groupnorm'])
def test_every_gradient_launch_reads_the_maximum_of_its_dz(storage, variant):
    """cell == max |dz| bit for bit (16-bit storage: the cell rounded to the storage type, see _CellProbe) at every split-fp16
    gradient launch of a train- and an eval-mode step: the operand scale of a
    launch is only as good as the cell it reads, and a cell of another layer or of an earlier pass passes every parity test as
    long as the two maxima lie within the headroom of the scale (2^6 for the direct kernels)."""
    log, _ = _watched_steps(storage, variant)
    seen = {}
    for step, name, *_ in log:
        seen[name] = seen.get(name, 0) + 1
    print(f'{storage} {variant or "batchnorm"}: {len(log)} launches, {seen}')
    assert {step for step, *_ in log} == {'train-BN', 'eval-BN'}
    wrong = _mismatches(log)
    assert not wrong, f'{len(wrong)} of {len(log)} launches read a cell that is not max |dz|:\n' + '\n'.join(
        f'  {step} {name} cell of {owner}: {cell!r} (stored as {st!r}), max |dz| {m!r}' for step, name, owner, cell, st, m in wrong[:20])
    lazy = 'pp_conv3x3_bwd_weight_f16x3_lazy'         # the lazy form: fp32-storage BatchNorm plans only (engine.LAZY_HALO_H16)
    missing = [n for n in WATCHED if n not in seen and (n != lazy or (storage, variant) == ('fp32', ''))]
    assert not missing, f'no launch of {missing} in the steps'


def test_swapped_cells_are_noticed():
    """The planted mistake: two layers' cells change places.  The check above must fail on exactly those layers' launches."""
    log, (a, b) = _watched_steps('fp32', '', swap=True)
    wrong = _mismatches(log)
    assert wrong, 'the swapped cells went unnoticed'
    assert {line[2] for line in wrong} == {a, b}, (a, b, wrong[:8])


# ------------------------------------------------------------------------------------- the measured envelope (report only)
def _envelope(ratio_of):
    """(lowest k, highest k) of the widest run of k containing 0 in which ratio_of[k] <= 1"""
    lo = hi = 0
    while lo - 2 in ratio_of and ratio_of[lo - 2] <= 1.0:
        lo -= 2
    while hi + 2 in ratio_of and ratio_of[hi + 2] <= 1.0:
        hi += 2
    return lo, hi


def measure(out=sys.stdout):
    """The tables of docs/operand_range.md, as markdown: nothing here is asserted."""
    def p(*a):
        print(*a, file=out, flush=True)
    p('### Forward: activation scale 2^k, k = -26 ... +16 (worst error / tolerance over the results of the launch)\n')
    ks = list(range(-26, 17, 2))
    p('| row | envelope (k) | ' + ' | '.join(f'{k:+d}' for k in ks) + ' |')
    p('|---|---|' + '---|' * len(ks))
    for tag, launch, _ in FWD:
        r = {k: _worst(_ratios('fp32', launch, Profile(act=2.0 ** k))) for k in ks}
        lo, hi = _envelope(r)
        p(f'| {tag} | {lo:+d} ... {hi:+d} | ' + ' | '.join(f'{r[k]:.2g}' for k in ks) + ' |')
    p('\n### Direct kernels beyond the fp16 range: activation scale 2^14 and 2^16\n')
    p('| row | k | outputs not finite | of |')
    p('|---|---|---|---|')
    for tag, launch, _ in FWD:
        if tag.startswith('fwd/'):
            for k in (14, 16):
                (label, (got, _)), = _launch('fp32', launch, Profile(act=2.0 ** k), want_ref=False).items()
                p(f'| {tag} | {k:+d} | {int((~torch.isfinite(got)).sum())} | {got.numel()} |')
    p('\n### Weight gradient per output channel, spread 2^-j over the channels of dz (worst channel, relative error)\n')
    p('| row | j = 12 | j = 16 | j = 20 |')
    p('|---|---|---|---|')
    for tag, launch, _ in WGRADS:
        errs = []
        for j in (12, 16, 20):
            (label, (got, ref)), = _launch('fp32', launch, Profile(spread=j)).items()
            errs.append(float(_channel_errors(got, ref).max()))
        p(f'| {tag} | ' + ' | '.join(f'{e:.2g}' for e in errs) + ' |')


if __name__ == '__main__':
    measure()
