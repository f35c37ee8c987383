"""Surface metrics (HD, ASSD, surface Dice, percentile distance) without a GPU: the scipy oracle of the GPU tests pinned against a
brute-force nearest-surface search, the host half of batch_surface_metrics on hand-made reductions, the C ABI of
pp_surface_reduce with its refusals before any launch, and the inference flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _surface_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'pp_surface_reduce'


def test_oracle_agrees_with_a_brute_force_search():
    rng = np.random.default_rng(11)
    scored = 0
    for i in range(60):
        H, W = (int(v) for v in rng.integers(1, 13, 2))
        spacing = R.SPACINGS[i % 3]
        a, b = rng.random((H, W)) < (0.2, 0.5, 0.8)[i % 3], rng.random((H, W)) < (0.5, 0.8, 0.2)[i % 3]
        if not R.is_scored(a, b):
            continue
        scored += 1
        d1, d2 = R.directed_sets(a, b, spacing)
        e1, e2 = R.brute_force_sets(a, b, spacing)
        # scipy walks the mask in row-major order and so does the brute force: the sets agree element by element
        np.testing.assert_allclose(d1, e1, rtol=1e-12, atol=0)
        np.testing.assert_allclose(d2, e2, rtol=1e-12, atol=0)
        m = R.metrics_of_sets(d1, d2, 2.0, 95.0)
        s = np.sort(np.hstack((e1, e2)))
        R.assert_tolerance_is_clear((d1, d2), 2.0)                 # ... to 1e-12, so both sides count the same elements below
        assert m['hd'] == max(d1.max(), d2.max()) and 0.0 <= m['nsd'] <= 1.0 and m['hdp'] <= m['hd']
        np.testing.assert_allclose([m['hd'], m['hdp']], [s[-1], np.percentile(s, 95.0)], rtol=1e-12)
        assert m['nsd'] == ((e1 <= 2.0).sum() + (e2 <= 2.0).sum()) / s.size
        np.testing.assert_allclose(m['assd'], (e1.sum() / e1.size + e2.sum() / e2.size) / 2, rtol=1e-12)
    assert scored > 30


def test_oracle_on_known_masks():
    a = np.zeros((9, 9), bool)
    a[2:7, 2:7] = True
    m = R.surface_metrics(a.astype(np.int64), a.astype(np.int64), 2, (1.0, 1.0))
    assert m['hd'].tolist() == [0.0, 0.0] and m['assd'].tolist() == [0.0, 0.0] and m['nsd'].tolist() == [1.0, 1.0]
    b = np.zeros((9, 9), bool)
    b[2:7, 5:8] = True                                            # shares the rows, not the columns
    d1, d2 = R.directed_sets(a, b, (1.0, 2.0))
    assert d1.max() == 6.0 and d2.max() == 2.0                  # column 2 to column 5 / column 7 to column 6, 2 mm per column
    full = np.ones((4, 4), np.int64)
    m = R.surface_metrics(full, full, 2, (1.0, 1.0))
    assert all(np.isnan(m[k]).all() for k in R.KEYS)            # class 1 fills the image, class 0 is empty
    with pytest.raises(AssertionError):
        R.assert_tolerance_is_clear([np.array([2.0, 2.00001])], 2.0)
    R.assert_tolerance_is_clear([np.array([2.0, 2.1, 1.9])], 2.0)


def _rows(sets, pixels, tolerance, percentile):
    """counts / out of hand-made items: (a, b, |pred|, |label|) -> the arrays the two device calls would leave."""
    counts = np.array([[a.size, b.size, ta, tb] for a, b, ta, tb in sets], np.int32)
    out = np.stack([R.reduce_row(a, b, tolerance, percentile) for a, b, _, _ in sets])
    return counts, out


def test_host_finish_on_hand_made_reductions():
    from pacingpseudo_amd.utils import surface_metrics_from_reduction as finish
    from pacingpseudo_amd.utils.metrics import surface_metrics_from_reduction
    assert finish is surface_metrics_from_reduction
    f = np.float64
    a21, none = np.arange(21, dtype=f) * 0.37, np.zeros(0, f)
    sets = [(np.array([1.0], f), np.array([3.0], f), 5, 7),         # n = 2
            (a21[:11], a21[11:], 30, 40),                           # n = 21 at 95: v = 19 exactly, fraction 0
            (np.array([0.5, 2.0, 2.5], f), np.array([4.0], f), 3, 1),
            (none, none, 0, 9),                                     # empty prediction
            (none, none, 9, 0),                                     # empty label
            (np.array([1.0], f), np.array([1.0], f), 100, 50),      # the prediction fills the image
            (np.array([1.0], f), np.array([1.0], f), 50, 100)]      # the label does
    counts, out = _rows(sets, 100, 2.0, 95.0)
    got = finish(counts, out, 100, 95.0)
    assert all(got[k].shape == (7,) and got[k].dtype == np.float64 for k in R.KEYS)
    assert all(np.isnan(got[k][3:]).all() and not np.isnan(got[k][:3]).any() for k in R.KEYS)
    assert got['hd'][:3].tolist() == [3.0, a21[20], 4.0]
    assert got['hdp'][0] == 1.0 + 2.0 * 0.95 and got['hdp'][1] == a21[19]
    assert got['assd'][:3].tolist() == [2.0, (a21[:11].mean() + a21[11:].mean()) / 2, (5.0 / 3 + 4.0) / 2]
    assert got['nsd'][:3].tolist() == [0.5, 6 / 21, 0.5]            # 0.37 i <= 2 for i <= 5; {0.5, 2.0} of four
    # percentile 100: j = n - 1, the upper index is clamped
    counts, out = _rows(sets[:3], 100, 2.0, 100.0)
    assert np.array_equal(out[:, 5], out[:, 6]) and np.array_equal(out[:, 5], out[:, 0])
    got = finish(counts, out, 100, 100.0)
    assert np.array_equal(got['hdp'], got['hd'])
    for bad in (0.0, -5.0, 100.5, float('nan')):
        with pytest.raises(ValueError, match='percentile'):
            finish(counts, out, 100, bad)


def test_host_finish_against_numpy_percentile():
    """hdp from the two bracketing order statistics against numpy.percentile of the float64 set: 4e-16 relative (numpy takes
    hi - (hi - lo) (1 - g) for g >= 0.5, so the two differ by roundings only)."""
    from pacingpseudo_amd.utils import surface_metrics_from_reduction as finish
    rng = np.random.default_rng(5)
    sets, pcts = [], (50.0, 95.0, 100.0, 37.5, 99.0)
    for i in range(2000):
        na, nb = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        scale = (1.0, 100.0, 1e-3)[i % 3]
        sets.append((rng.random(na) * scale, rng.random(nb) * scale, 5, 5))
    worst = 0.0
    for pct in pcts:
        counts, out = _rows(sets, 100, 0.5, pct)
        got = finish(counts, out, 100, pct)
        want = np.array([np.percentile(np.hstack((a, b)), pct) for a, b, _, _ in sets])
        worst = max(worst, float(np.max(np.abs(got['hdp'] - want) / want)))
        assert np.array_equal(got['hd'], [max(a.max(), b.max()) for a, b, _, _ in sets])
        np.testing.assert_allclose(got['assd'], [(a.mean() + b.mean()) / 2 for a, b, _, _ in sets], rtol=1e-14)
    print(f'worst relative deviation of hdp from numpy.percentile: {worst:.3e}')
    assert worst <= 4e-16


def test_abi_names_the_entry_point_and_both_versions_are_606():
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert NAME in _lib._PROTOS and NAME in _lib.EXPORTED_SYMBOLS
    m = re.search(r'\bint ' + NAME + r'\s*\(([^;]*)\)\s*;', header)
    assert m, f'{NAME} is not declared in the header'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == len(_lib._PROTOS[NAME][1]) == 8
    assert params[4].startswith('double ') and params[5].startswith('float ') and params[6].startswith('double*')
    assert _lib._PROTOS[NAME][1][4] is ctypes.c_double and _lib._PROTOS[NAME][1][5] is ctypes.c_float
    assert NAME not in _lib.H16_ENTRIES                            # fp32 distances in every storage mode: one symbol
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert NAME not in open(os.path.join(ROOT, 'include', h)).read()
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION == 606
    assert 'pp_surface_reduce' in open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_post.hip')).read()


def test_entry_point_refuses_bad_arguments_without_a_launch():
    """No GPU is needed: every call below must return an error from its argument checks.  The pointers are made up and never
    dereferenced by the host side."""
    from pacingpseudo_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'library not built (run __graft_entry__.build())'
    lib = _lib.lib
    dll = lib.load()                                                 # argtypes / restypes are set
    assert hasattr(dll, NAME) and lib.pp_version() == 606
    vp = ctypes.c_void_p
    p, q, r = 0x10000, 0x10000 + (1 << 40), 0x10000 + (1 << 41)

    def call(dist=p, counts=q, items=10, cap=4096, percentile=95.0, tolerance=2.0, out=r):
        return dll.pp_surface_reduce(vp(dist), vp(counts), items, cap, percentile, tolerance, vp(out), None)
    inf, nan = float('inf'), float('nan')
    bad = [dict(dist=None), dict(counts=None), dict(out=None), dict(items=0), dict(items=-3), dict(cap=0), dict(cap=-1),
           dict(percentile=0.0), dict(percentile=-1.0), dict(percentile=100.0000001), dict(percentile=inf), dict(percentile=nan),
           dict(tolerance=-1e-30), dict(tolerance=inf), dict(tolerance=nan), dict(tolerance=-inf),
           dict(items=1 << 14, cap=1 << 16),                         # items * 2 * cap = 2^31 exactly
           dict(items=1, cap=1 << 30)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b'surface_reduce' in dll.pp_last_error(), kw
    with pytest.raises(_lib.HipLibraryError, match='percentile'):
        lib.pp_surface_reduce(vp(p), vp(q), 10, 4096, 0.0, 2.0, vp(r), None)


def test_inference_flags_parse(capsys):
    from pacingpseudo_amd.inference import evaluate, parser
    import inspect
    base = ['--fold', '0', '--checkpoint_file', 'run-fold0']
    off = parser.parse_args(base)
    assert off.surface_metrics is False and off.nsd_tolerance == 2.0
    on = parser.parse_args(base + ['--surface_metrics', '--nsd_tolerance', '1.5'])
    assert on.surface_metrics is True and on.nsd_tolerance == 1.5
    assert parser.parse_args(base + ['--nsd_tolerance', '0']).nsd_tolerance == 0.0
    for bad in ('-1', 'inf', 'nan', '-inf', 'x'):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(base + ['--surface_metrics', '--nsd_tolerance=' + bad])
        assert e.value.code == 2, bad
        assert '--nsd_tolerance' in capsys.readouterr().err
    sig = inspect.signature(evaluate).parameters
    assert sig['surface_metrics'].default is False and sig['nsd_tolerance'].default == 2.0
