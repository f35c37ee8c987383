"""The mean-to-spread envelope of the normalisation statistics on the MI355X (docs/norm_range.md).

Every train-mode BatchNorm / GroupNorm statistic is the one-pass var = sum z^2 / n - mean^2 over fp32 partial sums.  The censuses
hold it to float64 at |mean| <= 4 sigma and at 8 values per fp32 partial (the floor of col_plan); here both move, through the
census adapters (NormProfile / norm_operands of tests/test_gpu_conv_census.py, replay() of either census):
  A  the mean-to-spread ratio r in {0, 8, r_TOL_SUMS, r_TOL}, both signs, for every statistics producer at depth 8;
  B  the per-thread depth 64 and 256 of the streaming statistics and backward forms, at r in {0, r_TOL_SUMS};
  C  z * 2^k, k = -10 and +10;
  D  the consumers (z * scale + shift cancels about eps * r) at r_TOL;
  E  the 16-bit twins, against float64 of the tensor each takes its statistics from.
r_TOL_SUMS and r_TOL are the declared envelope, DERIVED by tests/test_norm_range.py from a numpy emulation of the kernels'
summation order with a margin of 4; statistics rows hold TOL_SUMS up to r_TOL_SUMS and TOL up to r_TOL, every other result its
census tolerance.  What lies beyond is measured by `python -m tests.test_gpu_norm_range` and written down, not asserted.
"""
import math
import re
import sys

import pytest
import torch

from tests import test_gpu_conv_census as C
from tests import test_gpu_stream_census as S
from tests import test_norm_range as N
from tests.test_gpu_conv_census import TOL, TOL_SUMS, NormProfile, norm_operands
from tests.test_gpu_operand_range import FWD_ROWS, WINO_ROWS

pytestmark = pytest.mark.gpu

assert (TOL, TOL_SUMS) == (N.TOL, N.TOL_SUMS)
R_SUMS, R_TOL = N.envelope()
OFFSETS = sorted({0, 8, R_SUMS, R_TOL})
EPS, MOM, SLOPE = S.EPS, S.MOM, S.SLOPE
# a statistics row: a result the finalize arithmetic forms from the sums (the census holds them to TOL_SUMS)
STAT = re.compile(r'save_mean|save_invstd|save_xbar|scale|shift|running_mean|running_var')
# every entry point that forms sums of z for a normalisation; test_every_statistics_producer_is_swept checks it against _PROTOS
PRODUCERS = ('pp_bn_train_stats', 'pp_bn_stats_sums', 'pp_bn_train_finalize', 'pp_bn_train_finalize_lazy', 'pp_gn_stats',
             'pp_conv3x3_fwd_bn', 'pp_conv3x3_fwd_bn_lazy', 'pp_conv3x3_wino_fwd_bn')
p = 'p'


# ------------------------------------------------------------------------------------------------------------------ launches
def _chain(key, run):
    """pp_bn_stats_sums into pp_bn_train_finalize[_lazy] as one chain: the kernel's own sums are the finalize's one partial row"""
    _, name, (Cn, P, G) = key
    ops = S._DOps(key)
    ld = Cn + 4
    z = ops.norm_z(G, P, 1, Cn)
    zd = run.d(ops.pad(z, ld))
    z64 = z.double().reshape(G, P, Cn)
    ws, nws = S._bn_ws('pp_bn_stats_sums', Cn, P, G)
    sums = C._full((G, 2, Cn), 7.0, dtype=torch.float64)
    run.K.pp_bn_stats_sums(zd.data_ptr(), ld, Cn, P, G, sums.data_ptr(), ws.data_ptr(), nws, run.st)
    gamma, beta, rm, rv = ops.affine(Cn)
    gd, bd, rmd, rvd = (S._f32(run, t.clone()) for t in (gamma, beta, rm, rv))
    nbt = C._full((), 3, dtype=torch.int64)
    coef = C._full((4, G, Cn), 7.0)
    args = (sums.data_ptr(), 1, Cn, P, G, EPS, MOM, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), nbt.data_ptr(),
            *(coef[i].data_ptr() for i in range(4)))
    if name.endswith('_lazy'):
        lz = C._full((G, 3, ld), 7.0)
        run.K.pp_bn_train_finalize_lazy(*args, lz.data_ptr(), ld, SLOPE, run.st)
    else:
        run.K.pp_bn_train_finalize(*args, run.st)
    ref = S._check_stats(run, z64, gamma, beta, rm, rv, EPS, MOM, coef, rmd, rvd, nbt)
    if name.endswith('_lazy'):
        run.check('lazy scale row', lz[:, 0, :Cn], ref[2], TOL_SUMS, act=False)
        run.check('lazy shift row', lz[:, 1, :Cn], ref[3], TOL_SUMS, act=False)
        run.canary('lazy rows', lz, Cn)


CHAIN = {'pp_bn_train_finalize': _chain, 'pp_bn_train_finalize_lazy': _chain}


def _gn_key(Cn, HW, Nimg, G):
    return ('pp_gn_stats', (p, Cn + 4, Cn, HW, Nimg, G, EPS, p, p, p, p, p, p, p, p, 'sz', p))


def _fwd_key(Cn, P, G):
    return ('pp_bn_lrelu_fwd', (p, Cn + 4, p, p, p, Cn + 8, Cn, P, G, SLOPE, p))


def _pool_key(Cn, Nimg, H, W, G):
    return ('pp_bn_lrelu_fwd_pool', (p, Cn + 4, p, p, p, Cn + 8, p, Cn + 12, Cn, Nimg, H, W, G, SLOPE, p))


def _lazy_form(launch, Cin):
    name, a = launch
    return (name + '_lazy', a[:-1] + (('lazy', Cin + 8, 1), p))


def _ratios(storage, launch, prof):
    """{label: error / tolerance} of one launch under a NormProfile, through the census that owns the entry"""
    with norm_operands(prof):
        if launch[0] in CHAIN:
            return dict(C.replay((storage,) + launch, CHAIN))
        return dict((S.replay if launch[0] in S.ADAPTERS else C.replay)((storage,) + launch))


def _raw(launch, prof):
    """{label: (device result, float64 reference)} of one fp32 launch (the stream census's adapters)"""
    from pacingpseudo_amd._lib import lib
    run = C._Run(lib, torch.float32, True)
    with norm_operands(prof):
        C._execute(CHAIN.get(launch[0]) or S.ADAPTERS[launch[0]], ('fp32',) + launch, run)
    return {label: (got, ref) for label, got, ref, _, _ in run.res if got is not None}


def _allowed(label, r):
    """statistics rows: TOL_SUMS up to r_TOL_SUMS, TOL up to r_TOL (as a multiple of the census tolerance TOL_SUMS)"""
    return TOL / TOL_SUMS if (r > R_SUMS and STAT.search(label)) else 1.0


def _hold(tag, res, r):
    assert r <= R_TOL
    worst = max(float('inf') if v != v else v for v in res.values())
    print(f'{tag} r = {r}: worst error / tolerance {worst:.3g} (' + ', '.join(f'{lab} {v:.2g}' for lab, v in res.items() if v > 0.05) + ')')
    bad = {lab: f'{v:.3g}' for lab, v in res.items() if not v <= _allowed(lab, r)}
    assert not bad, (tag, r, bad)


# ------------------------------------------------------------------------------------------- A: offset sweep at depth 8
# (C, P per group, groups): NORM_EDGES' rows32 / idle-lane / fewer-pixels-than-rows shapes and two groups of 64 channels
SHAPES = {'rows32-ragged': S.NORM_EDGES['rows32-nblk-above-192-ragged-last-chunk'], 'rows1-idle-lanes-C516': S.NORM_EDGES['rows1-idle-lanes-C516'],
          'fewer-pixels-than-rows': S.NORM_EDGES['fewer-pixels-than-rows'], 'C64-two-groups': (64, 4096, 2)}


def _stream_producers(Cn, P, G):
    keys = S._norm_edge_keys(Cn, P, G)
    return [keys[0], keys[1], ('pp_bn_train_finalize', (Cn, P, G)), ('pp_bn_train_finalize_lazy', (Cn, P, G))]


@pytest.mark.parametrize('r', OFFSETS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_streaming_statistics_off_centre(shape, r):
    """pp_bn_train_stats, pp_bn_stats_sums, and the sums of pp_bn_stats_sums fed to pp_bn_train_finalize[_lazy], at depth 8."""
    Cn, P, G = SHAPES[shape]
    assert N.depth(Cn, P, G) == 8
    for launch in _stream_producers(Cn, P, G):
        _hold(f'{launch[0]} {shape}', _ratios('fp32', launch, NormProfile(offset=r)), r)


@pytest.mark.parametrize('r', OFFSETS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_groupnorm_statistics_off_centre(shape, r):
    """pp_gn_stats with one group, four channels per group and one channel per group (the images are BatchNorm's groups); the
    offsets alternate in sign inside a group.  One channel per group: xbar = mean of xhat over the channel is 0 up to rounding in
    the kernel and in float64 alike, so the row has no magnitude to be relative to: it is held to TOL_SUMS absolutely (xhat has
    unit deviation)."""
    Cn, HW, Nimg = SHAPES[shape]
    for G in (1, Cn // 4, Cn):
        res = _ratios('fp32', _gn_key(Cn, HW, Nimg, G), NormProfile(offset=r))
        if G == Cn:
            got, ref = _raw(_gn_key(Cn, HW, Nimg, G), NormProfile(offset=r))['save_xbar']
            res['save_xbar'] = float((got.double() - ref).abs().max()) / TOL_SUMS
        _hold(f'pp_gn_stats {shape} G={G}', res, r)


def _epilogue_rows():
    rows = [(f'fwd_bn/{tag}', C._k_fwd_bn('f16x3', O_, Cin, *g, 1, 1)) for tag, (O_, Cin, g) in FWD_ROWS.items()]
    rows += [(f'wino_fwd_bn/{tag}', C._k_fwd_bn('wino-split', *g, 1)) for tag, g in WINO_ROWS.items()]
    O_, Cin, g = FWD_ROWS['halo2-one-row-per-wave']          # (a lazy input needs the two-half halo kernel: pp_conv3x3_lazy_ok)
    rows.append(('fwd_bn_lazy/halo2-one-row-per-wave', _lazy_form(C._k_fwd_bn('f16x3', O_, Cin, *g, 1, 1), Cin)))
    # the first layer: one true input channel in a row of four, the fp32 kernel (W % 16 == 0)
    rows.append(('fwd_bn/first-layer-fp32-Cin1', C._k_fwd_bn('fp32', 32, 4, 3, 6, 16, 1, 1)))
    return rows


EPILOGUES = _epilogue_rows()


@pytest.mark.parametrize('tag,launch', EPILOGUES, ids=[t for t, _ in EPILOGUES])
def test_fused_epilogue_statistics_off_centre(tag, launch):
    """Mode 1 of the fused epilogues with a conv bias of +-r deviations: z and the partial sums as in the census, and the partial
    rows finalized by pp_bn_train_finalize against the float64 statistics of the z the launch wrote."""
    for r in OFFSETS:
        res = _ratios('fp32', launch, NormProfile(offset=r))
        assert any(lab.startswith('finalized') for lab in res), sorted(res)
        _hold(tag, res, r)


# ----------------------------------------------------------------------------------------------------------------- B: depth
DEPTH_ROWS = [(32, 2, 64), (64, 1, 64), (1024, 1, 64), (516, 1, 64), (32, 2, 256)]          # (C, groups, depth)
FORMS = {'train_stats': 0, 'stats_sums': 1, 'bwd-train-statistics': 2, 'bwd-eval-statistics': 3, 'bwd_eval': 5, 'bwd_sums': 6, 'bwd_apply': 7}
DEPTH_CASES = [(Cn, G, d, form) for Cn, G, d in DEPTH_ROWS for form in FORMS
               if d == 64 or form in ('train_stats', 'stats_sums', 'bwd-train-statistics')]


def _assert_depth(Cn, G, d):
    """the row has the per-thread depth it claims: from the mirrored col_plan, and nblk through the library's workspace query"""
    from pacingpseudo_amd._lib import lib
    P = N.pixels_for_depth(Cn, G, d)
    c4, rows, chunk, nblk = N.col_plan(Cn, P, G)
    assert chunk // rows == d and nblk * G == N.BLOCKS and chunk * nblk == P, (Cn, G, d, (c4, rows, chunk, nblk))
    assert lib.pp_bn_workspace(Cn, P, G) == G * nblk * 2 * Cn * 8 + 256 == N.bn_workspace(Cn, P, G)
    return P


@pytest.mark.parametrize('r', sorted({0, R_SUMS}))
@pytest.mark.parametrize('Cn,G,d,form', DEPTH_CASES, ids=[f'C{c}-G{g}-depth{d}-{f}' for c, g, d, f in DEPTH_CASES])
def test_streaming_kernels_at_workload_depth(Cn, G, d, form, r):
    """The bn_* streaming kernels with d values per fp32 partial (the census has 8): the statistics, and the backward forms whose
    per-thread sums of g and g * xhat have the same depth, at the census tolerances.  Depth 256 at (32 channels, two groups) is
    the plan of the workload's widest tensors, 2 x 32 x 256^2 pixels."""
    P = _assert_depth(Cn, G, d)
    if (Cn, G, d) == (32, 2, 256):
        assert P == 32 * 256 * 256
    launch = S._norm_edge_keys(Cn, P, G)[FORMS[form]]
    _hold(f'{launch[0]} C={Cn} G={G} depth {d}', _ratios('fp32', launch, NormProfile(offset=r)), r)


# ----------------------------------------------------------------------------------------------------------------- C: scale
@pytest.mark.parametrize('k', (-10, 10))
@pytest.mark.parametrize('shape', ('rows32-ragged', 'C64-two-groups'))
def test_statistics_of_scaled_operands(shape, k):
    """z * 2^k at r_TOL_SUMS.  k = +10: eps is negligible beside var ~ 1e6.  k = -10: var ~ 1e-6 < eps, invstd is dominated by
    eps -- and still held to float64 at TOL_SUMS, like every other row."""
    Cn, P, G = SHAPES[shape]
    prof = NormProfile(offset=R_SUMS, scale=k)
    for launch in _stream_producers(Cn, P, G) + [_gn_key(Cn, P, G, Cn // 4)]:
        _hold(f'{launch[0]} {shape} k = {k}', _ratios('fp32', launch, prof), R_SUMS)


# ------------------------------------------------------------------------------------------------------------- D: consumers
CONSUMERS = [('bn_lrelu_fwd/C64-two-groups', _fwd_key(64, 4096, 2)), ('bn_lrelu_fwd/rows1-idle-lanes-C516', _fwd_key(516, 300, 1)),
             ('bn_lrelu_fwd_pool/C32-two-groups', _pool_key(32, 4, 18, 22, 2)), ('bn_lrelu_fwd_pool/C516', _pool_key(516, 2, 6, 10, 1)),
             ('fwd_bn/igemm-128x64/eval-epilogue', C._k_fwd_bn('f16x3', *FWD_ROWS['igemm-128x64'][:2], *FWD_ROWS['igemm-128x64'][2], 1, 2)),
             ('wino_fwd_bn/round-3-gemm-ragged-tiles/eval-epilogue', C._k_fwd_bn('wino-split', *WINO_ROWS['round-3-gemm-ragged-tiles'], 2))]


@pytest.mark.parametrize('tag,launch', CONSUMERS, ids=[t for t, _ in CONSUMERS])
def test_consumers_at_the_edge_of_the_envelope(tag, launch):
    """y = lrelu(z * scale + shift) with the rows of a normalisation whose mean is r_TOL deviations from zero (the streaming
    forms: shift = beta - mean * scale; the eval epilogues: a running mean of r_TOL * sqrt(running_var), which is the conv bias):
    the two terms cancel to about eps * r, and y holds TOL."""
    _hold(tag, _ratios('fp32', launch, NormProfile(offset=R_TOL)), R_TOL)


# -------------------------------------------------------------------------------------------------------- E: 16-bit storage
H16_EPILOGUE = 'fwd_bn/f16x3/O32-C160/3x12x96/dil1/train-statistics'          # H16_ROWS of the convolution census


@pytest.mark.parametrize('r', sorted({0, R_SUMS}))
@pytest.mark.parametrize('storage', ('fp16', 'bf16'))
def test_16bit_twins_take_their_statistics_from_what_they_read(storage, r):
    """pp_bn_train_stats_h16 / _bf16 at depth 64 reads the stored tensor: float64 of that same rounded z.  The fused epilogue
    sums its fp32 accumulators before the 16-bit store: float64 of the fp32 twin's z (at r = 8 the statistics of a bf16-rounded z
    differ from those by about 1e-4, ten times TOL_SUMS, so the wrong tensor would show)."""
    P = _assert_depth(32, 2, 64)
    _hold(f'pp_bn_train_stats [{storage}] depth 64', _ratios(storage, S._norm_edge_keys(32, P, 2)[0], NormProfile(offset=r)), r)
    res = _ratios(storage, C._EDGE_OF[H16_EPILOGUE], NormProfile(offset=r))
    assert any(lab.startswith('finalized') for lab in res), sorted(res)
    _hold(f'{H16_EPILOGUE} [{storage}]', res, r)


# ---------------------------------------------------------------------------------------------------------------- ownership
def test_every_statistics_producer_is_swept():
    """Every entry point of the library that sums z for a normalisation is in PRODUCERS, and every name there is launched by an
    asserted row of A: a new producer fails here by name."""
    from pacingpseudo_amd._lib import _PROTOS
    pattern = re.compile(r'^pp_(bn_train_stats|bn_stats_sums|bn_train_finalize|gn_stats|conv3x3_(wino_)?fwd_bn)')
    base = {re.sub(r'_(h16|bf16)$', '', n) for n in _PROTOS if pattern.match(n)}
    assert base == set(PRODUCERS), sorted(base ^ set(PRODUCERS))
    swept = {launch[0] for Cn, P, G in SHAPES.values() for launch in _stream_producers(Cn, P, G)}
    swept |= {_gn_key(4, 1, 1, 1)[0]} | {launch[0] for _, launch in EPILOGUES}
    assert swept == set(PRODUCERS), sorted(swept ^ set(PRODUCERS))


# ------------------------------------------------------------------------------------- the measured envelope (report only)
def measure(out=sys.stdout):
    """The tables of docs/norm_range.md, as markdown: nothing here is asserted."""
    def pr(*a):
        print(*a, file=out, flush=True)
    rs = [2 ** i for i in range(13)]
    limit = 0.999 / math.sqrt(EPS)

    def sweep(tag, launch, census):
        first, table = None, {}
        for r in rs:
            prof = NormProfile(offset=r)
            if census:
                res = _ratios('fp32', launch, prof)
            else:
                raw = _raw(launch, prof)
                res = {lab: C._rel(got, ref) / TOL_SUMS for lab, (got, ref) in raw.items() if ref is not None}
                inv = raw['save_invstd'][0]
                if first is None and bool((inv[..., :-1] >= limit).any()):
                    first = r
            for lab, v in res.items():
                if ('varying' in lab or 'running_var' in lab or lab.startswith('finalized')) and 'mean' not in lab:
                    table.setdefault(lab, []).append(v)
        for lab, vs in table.items():
            pr(f'| {tag} | {lab} | ' + ' | '.join(f'{v:.2g}' for v in vs) + ' |')
        return first

    pr('### Statistics rows, worst error / TOL_SUMS, mean-to-spread ratio r = 1 ... 4096 (TOL is 10 in these units)\n')
    pr('| producer | row | ' + ' | '.join(f'{r}' for r in rs) + ' |')
    pr('|---|---|' + '---|' * len(rs))
    clamps = []
    for d in N.DEPTHS:
        P = N.pixels_for_depth(32, 2, d)
        assert N.depth(32, P, 2) == d
        keys = S._norm_edge_keys(32, P, 2)
        clamps.append((f'pp_bn_train_stats depth {d}', sweep(f'pp_bn_train_stats C=32 G=2 depth {d}', keys[0], False)))
        clamps.append((f'pp_bn_stats_sums + pp_bn_train_finalize depth {d}',
                       sweep(f'sums + finalize C=32 G=2 depth {d}', ('pp_bn_train_finalize', (32, P, 2)), False)))
        clamps.append((f'pp_gn_stats G = C depth {d}', sweep(f'pp_gn_stats C=32 N=2 G=32 depth {d}', _gn_key(32, P, 2, 32), False)))
    for tag, launch in EPILOGUES:
        sweep(tag, launch, True)
    pr('\n### First r at which the variance of a non-constant channel clamps to 0 or invstd reaches 1 / sqrt(eps)\n')
    pr('| producer | first r |\n|---|---|')
    for tag, first in clamps:
        pr(f'| {tag} | {first if first is not None else "none up to 4096"} |')


if __name__ == '__main__':
    measure()
