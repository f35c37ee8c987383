"""Test-time augmentation without a GPU: the view geometry of the fp64 oracle (tests/_tta_reference.py), the modes, the
inference flag, the wrapper's argument checks and the refusals of the three C entry points before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _tta_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pp_tta_view', 'pp_tta_accumulate', 'pp_tta_finalize')


def test_views_invert_differ_and_swap_shapes():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((2, 3, 5, 7))                      # non-square, no symmetry
    views = [R.view(a, op) for op in range(8)]
    for op, v in enumerate(views):
        assert v.shape == ((2, 3, 7, 5) if op & 4 else (2, 3, 5, 7)), op
        assert np.array_equal(R.inverse(v, op), a), op
        assert np.array_equal(R.view(R.inverse(a if not op & 4 else v, op), op), a if not op & 4 else v), op
    for p in range(8):
        for q in range(p + 1, 8):
            assert views[p].shape != views[q].shape or not np.array_equal(views[p], views[q]), (p, q)
    # the definition, spelled out on one element: op 7 = transpose, flip H, flip W
    assert R.view(a, 7)[1, 2, 0, 0] == a[1, 2, 4, 6] and R.view(a, 4)[0, 0, 6, 1] == a[0, 0, 1, 6]
    assert R.view(a, 1)[0, 0, 2, 0] == a[0, 0, 2, 6] and R.view(a, 2)[0, 0, 0, 3] == a[0, 0, 4, 3]


def test_oracle_mean_of_identical_views_is_the_softmax():
    rng = np.random.default_rng(4)
    z = rng.standard_normal((2, 5, 6, 9))
    ops = (0, 1, 2, 3, 4, 5, 6, 7)
    prob, cls = R.tta_mean([R.view(z, op) for op in ops], ops)
    assert np.allclose(prob, R.softmax(z), rtol=0, atol=1e-15) and np.array_equal(cls, z.argmax(1))
    assert np.allclose(prob.sum(1), 1.0, rtol=0, atol=1e-14)


def test_modes():
    from pacingpseudo_amd import utils
    from pacingpseudo_amd.utils import tta as T
    assert utils.tta_predict is T.tta_predict and utils.tta_view is T.tta_view and utils.tta_ops is T.tta_ops
    assert utils.TTA_MODES == T.TTA_MODES == ('none', 'flips', 'd4')
    assert T.tta_ops('none') == (0,)
    assert T.tta_ops('flips') == (0, 1, 2, 3)
    assert T.tta_ops('d4') == (0, 1, 2, 3, 4, 5, 6, 7)
    for bad in ('D4', 'rot', '', None, 4):
        with pytest.raises(ValueError, match='mode'):
            T.tta_ops(bad)
    assert T.view_shape(5, 7, 3) == (5, 7) and T.view_shape(5, 7, 6) == (7, 5)


def test_inference_flag_parses(capsys):
    from pacingpseudo_amd.inference import parser
    base = ['--fold', '0', '--checkpoint_file', 'run-fold0']
    assert parser.parse_args(base).tta == 'none'
    for mode in ('none', 'flips', 'd4'):
        assert parser.parse_args(base + ['--tta', mode]).tta == mode
    for bad in ('rot90', 'D4', '8'):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(base + ['--tta', bad])
        assert e.value.code == 2, bad
        assert '--tta' in capsys.readouterr().err


def test_evaluate_refuses_an_unknown_mode_before_anything_runs():
    from pacingpseudo_amd import inference as I

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'touched ({name})')
    with pytest.raises(ValueError, match='mode'):
        I.evaluate(Untouchable(), Untouchable(), 4, (1.0, 1.0), 'cpu', tta='rot')


def test_wrapper_raises_before_touching_the_library(monkeypatch):
    from pacingpseudo_amd import _lib
    from pacingpseudo_amd.utils import tta as T

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'the library was touched ({name})')
    monkeypatch.setattr(T, 'lib', Untouchable())
    monkeypatch.setattr(_lib, 'lib', Untouchable())

    def never(x):
        raise AssertionError('forward was called')
    cpu = torch.zeros(2, 1, 4, 6)
    huge = torch.zeros(1).expand(2, 1, 1 << 15, 1 << 15)                 # 2^31 elements, no memory behind them
    with pytest.raises(ValueError, match='mode'):
        T.tta_predict(never, cpu, 'rot')
    for op in (-1, 8, 1.0, '1', True, None):
        with pytest.raises(ValueError, match='op'):
            T.tta_view(cpu, op)
    for call in (lambda t: T.tta_view(t, 5), lambda t: T.tta_predict(never, t, 'd4'), lambda t: T.tta_predict(never, t, 'none')):
        with pytest.raises(ValueError, match='CUDA'):
            call(cpu)
        with pytest.raises(ValueError, match='float32'):
            call(cpu.double())
        with pytest.raises(ValueError, match='float32'):
            call(cpu.to(torch.int64))
        with pytest.raises(ValueError, match=r'\(N, C, H, W\)'):
            call(torch.zeros(4, 6))
        with pytest.raises(ValueError, match=r'\(N, C, H, W\)'):
            call(torch.zeros(1, 2, 1, 4, 6))
        with pytest.raises(ValueError, match='empty'):
            call(torch.zeros(2, 1, 0, 6))
        with pytest.raises(ValueError, match='tensor'):
            call(np.zeros((2, 1, 4, 6), np.float32))
        with pytest.raises(ValueError, match=r'2\^31'):
            call(huge)
    # what `forward` hands back, view by view: N = 2 slices of 4 x 6
    ok = T._check_logits
    with pytest.raises(ValueError, match='CUDA'):
        ok(torch.zeros(2, 5, 4, 6), 2, 4, 6, 3, None)                    # everything but the device is right
    with pytest.raises(ValueError, match='CUDA'):
        ok(torch.zeros(2, 5, 6, 4), 2, 4, 6, 6, 5)
    with pytest.raises(ValueError, match='forward returned'):
        ok(torch.zeros(2, 5, 4, 6), 2, 4, 6, 6, None)                    # a transposing view comes back 6 x 4
    with pytest.raises(ValueError, match='forward returned'):
        ok(torch.zeros(2, 5, 6, 4), 2, 4, 6, 1, None)
    with pytest.raises(ValueError, match='forward returned'):
        ok(torch.zeros(3, 5, 4, 6), 2, 4, 6, 0, None)
    with pytest.raises(ValueError, match='K = 33'):
        ok(torch.zeros(2, 33, 4, 6), 2, 4, 6, 0, None)
    with pytest.raises(ValueError, match='K = 4'):
        ok(torch.zeros(2, 4, 4, 6), 2, 4, 6, 1, 5)
    with pytest.raises(ValueError, match='float32'):
        ok(torch.zeros(2, 5, 4, 6, dtype=torch.float16), 2, 4, 6, 0, None)
    with pytest.raises(ValueError, match=r'\(N, C, H, W\)'):
        ok(torch.zeros(2, 4, 6), 2, 4, 6, 0, None)
    with pytest.raises(ValueError, match=r'2\^31'):
        ok(torch.zeros(1).expand(2, 32, 1 << 13, 1 << 12), 2, 1 << 13, 1 << 12, 0, None)      # N K H W = 2^31


def test_abi_names_the_entry_points():
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NAMES:
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\bint ' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        assert len(m.group(1).split(',')) == len(_lib._PROTOS[name][1]), name
        assert name not in _lib.H16_ENTRIES                        # logits are fp32 in every storage mode: one symbol
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert 'pp_tta' not in open(os.path.join(ROOT, 'include', h)).read()
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """No GPU is needed: every call below must return an error from its argument checks.  The pointers are made up and never
    dereferenced by the host side."""
    from pacingpseudo_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'library not built (run __graft_entry__.build())'
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(dll, name), name
    lib = _lib.lib
    lib.load()                                                       # argtypes / restypes are set
    p, q = 0x10000, 0x10000 + (1 << 40)                              # two "device pointers" far apart
    N, K, H, W = 2, 5, 37, 53
    vp = ctypes.c_void_p

    def view(x=p, planes=N * 3, h=H, w=W, op=5, out=q):
        return dll.pp_tta_view(vp(x), planes, h, w, op, vp(out), None)

    def accumulate(z=p, n=N, k=K, h=H, w=W, op=5, first=1, acc=q):
        return dll.pp_tta_accumulate(vp(z), n, k, h, w, op, first, vp(acc), None)

    def finalize(acc=p, n=N, k=K, h=H, w=W, views=8, cls=q):
        return dll.pp_tta_finalize(vp(acc), n, k, h, w, views, vp(cls), None)
    big = dict(n=1 << 11, h=1 << 10, w=1 << 10)                      # times K = 1: exactly 2^31
    bad_view = [dict(x=None), dict(out=None), dict(planes=0), dict(h=0), dict(w=-1), dict(op=-1), dict(op=8), dict(out=p),
                dict(out=p + 4 * (N * 3 * H * W - 1)), dict(planes=1 << 11, h=1 << 10, w=1 << 10)]
    bad_acc = [dict(z=None), dict(acc=None), dict(n=0), dict(h=0), dict(w=0), dict(k=0), dict(k=33), dict(op=-1), dict(op=8),
               dict(k=1, **big), dict(k=32, n=1 << 6, h=1 << 10, w=1 << 10)]
    bad_fin = [dict(acc=None), dict(n=0), dict(h=-3), dict(w=0), dict(k=0), dict(k=33), dict(views=0), dict(views=3), dict(views=6),
               dict(views=16), dict(views=-8), dict(k=1, **big)]
    for fn, cases in ((view, bad_view), (accumulate, bad_acc), (finalize, bad_fin)):
        for kw in cases:
            rc = fn(**kw)
            assert rc < 0, (fn.__name__, kw, rc)
            assert lib.pp_last_error(), (fn.__name__, kw)
    assert b'op=8' in (view(op=8) and lib.pp_last_error())
    assert b'overlap' in (view(out=p) and lib.pp_last_error())
    assert b'K=33' in (accumulate(k=33) and lib.pp_last_error())
    assert b'2^31' in (accumulate(k=1, **big) and lib.pp_last_error())
    assert b'views=3' in (finalize(views=3) and lib.pp_last_error())
    assert b'null' in (finalize(acc=None) and lib.pp_last_error())
