"""Keep-largest-component post-processing without a GPU: the scipy oracle of the GPU tests pinned against a brute-force flood fill,
the inference flags, the wrapper's argument checks, the C ABI of the three entry points and their refusals before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _cc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pp_components_workspace', 'pp_label_components', 'pp_keep_largest_components')


@pytest.mark.parametrize('connectivity', [1, 2])
def test_oracle_agrees_with_a_flood_fill(connectivity):
    rng = np.random.default_rng(7 + connectivity)
    ties = 0
    for i in range(40):
        H, W = (int(v) for v in rng.integers(1, 13, 2))
        K = (2, 3, 5)[i % 3]
        cm = rng.integers(0, K, (H, W)) if i % 2 else (rng.random((H, W)) < (0.3, 0.6, 0.9)[i % 3]).astype(np.int64)
        assert np.array_equal(R.canonical_labels(cm, connectivity), R.flood_fill_labels(cm, connectivity)), (i, H, W)
        out, stats = R.keep_largest(cm, K, connectivity)
        out_f, stats_f = R.flood_fill_keep_largest(cm, K, connectivity)
        assert np.array_equal(out, out_f) and np.array_equal(stats, stats_f), (i, H, W)
        lab = R.flood_fill_labels(cm, connectivity)
        for k in range(1, K):
            sizes = np.unique(lab[cm == k], return_counts=True)[1]
            ties += len(sizes) > 1 and (sizes == sizes.max()).sum() > 1
    assert ties > 5                                            # the tie rule was exercised, not assumed


def test_oracle_on_the_structured_maps():
    s = R.serpentine(67, 130)
    lab = R.canonical_labels(s, 1)
    assert int(s.sum()) == 4453 and (lab[s == 1] == 0).all()              # one component, 34 rows + 33 joints
    c = R.comb(20, 21)
    assert (R.canonical_labels(c, 1)[c == 1] == 0).all()
    d = np.eye(9, dtype=np.int64)
    assert len(np.unique(R.canonical_labels(d, 1)[d == 1])) == 9 and len(np.unique(R.canonical_labels(d, 2)[d == 1])) == 1
    yy, xx = np.mgrid[0:40, 0:44]
    chk = 1 + (yy + xx) % 2
    out, stats = R.keep_largest(chk, 3, 1)
    assert stats.tolist() == [[0, 0], [880, 1], [880, 1]]
    assert np.flatnonzero(out == 1).tolist() == [0] and np.flatnonzero(out == 2).tolist() == [1]
    out, stats = R.keep_largest(chk, 3, 2)
    assert np.array_equal(out, chk) and stats.tolist() == [[0, 0], [1, 880], [1, 880]]


def test_inference_flags_parse(capsys):
    from pacingpseudo_amd.inference import parser
    base = ['--fold', '0', '--checkpoint_file', 'run-fold0']
    off = parser.parse_args(base)
    assert off.keep_largest_cc is False and off.cc_connectivity == 1
    on = parser.parse_args(base + ['--keep_largest_cc', '--cc_connectivity', '2'])
    assert on.keep_largest_cc is True and on.cc_connectivity == 2
    for bad in ('0', '3', 'x'):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(base + ['--keep_largest_cc', '--cc_connectivity', bad])
        assert e.value.code == 2, bad
        assert '--cc_connectivity' in capsys.readouterr().err


def test_wrapper_raises_before_touching_the_library(monkeypatch):
    from pacingpseudo_amd import _lib, utils
    from pacingpseudo_amd.utils import postprocess as P
    assert utils.label_components is P.label_components and utils.keep_largest_components is P.keep_largest_components

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'the library was touched ({name})')
    monkeypatch.setattr(P, 'lib', Untouchable())
    monkeypatch.setattr(_lib, 'lib', Untouchable())
    cpu = torch.zeros(4, 5, dtype=torch.int64)
    for call in (lambda t, **kw: P.label_components(t, **kw), lambda t, **kw: P.keep_largest_components(t, 4, **kw)):
        with pytest.raises(ValueError, match='CUDA'):
            call(cpu)
        for c in (0, 3, '1', True, 1.0):
            with pytest.raises(ValueError, match='connectivity'):
                call(cpu, connectivity=c)
        with pytest.raises(ValueError, match=r'\(N, H, W\)'):
            call(torch.zeros(5, dtype=torch.int64))
        with pytest.raises(ValueError, match=r'\(N, H, W\)'):
            call(torch.zeros(1, 1, 4, 5, dtype=torch.int64))
        with pytest.raises(ValueError, match='empty'):
            call(torch.zeros(2, 0, 5, dtype=torch.int64))
        with pytest.raises(ValueError, match='integers'):
            call(torch.zeros(4, 5))
        with pytest.raises(ValueError, match='tensor'):
            call(np.zeros((4, 5), np.int64))
    for k in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match='num_classes'):
            P.keep_largest_components(cpu, k)


def test_abi_names_the_entry_points_and_both_versions_are_606():
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NAMES:
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\b' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        assert len(m.group(1).split(',')) == len(_lib._PROTOS[name][1]), name
        assert name not in _lib.H16_ENTRIES                        # integer class maps: one symbol in every storage mode
    assert _lib._PROTOS['pp_components_workspace'][0] is _lib.sz
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION == 606
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        txt = open(os.path.join(ROOT, 'include', h)).read()
        assert 'components' not in txt
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'pp_post.hip' in re.search(r'^SRCS := (.*)$', mk, flags=re.M).group(1)
    assert 'pp_post.hip' not in re.search(r'^H16_SRCS := (.*)$', mk, flags=re.M).group(1)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """No GPU is needed: every call below must return an error from its argument checks.  The pointers are made up and never
    dereferenced by the host side."""
    from pacingpseudo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(dll, name), name
    lib = _lib.lib
    assert lib.pp_version() == 606
    N, K, H, W = 2, 5, 37, 53
    need = lib.pp_components_workspace(N, K, H, W)
    assert need >= 3 * 4 * N * H * W + 12 * N * K                  # parent, size, labels + the per-(image, class) block
    assert lib.pp_components_workspace(N, 1, H, W) <= need < lib.pp_components_workspace(N, 32, H, W)
    assert lib.pp_components_workspace(N, K, 512, 512) > need
    p = 0x10000                                                     # "device pointers"
    big = 1 << 40

    def label(cls=p, n=N, h=H, w=W, c=1, labels=p, ws=p, nws=big):
        return dll.pp_label_components(ctypes.c_void_p(cls), n, h, w, c, ctypes.c_void_p(labels), ctypes.c_void_p(ws), ctypes.c_size_t(nws), None)

    def keep(cls=p, n=N, k=K, h=H, w=W, c=1, out=p, stats=p, ws=p, nws=big):
        return dll.pp_keep_largest_components(ctypes.c_void_p(cls), n, k, h, w, c, ctypes.c_void_p(out), ctypes.c_void_p(stats),
                                              ctypes.c_void_p(ws), ctypes.c_size_t(nws), None)
    lib.load()                                                       # argtypes / restypes are set
    bad_label = [dict(cls=None), dict(labels=None), dict(ws=None), dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=3),
                 dict(n=1 << 11, h=1 << 10, w=1 << 10), dict(nws=lib.pp_components_workspace(N, 1, H, W) - 1), dict(nws=0)]
    for kw in bad_label:
        rc = label(**kw)
        assert rc < 0, (kw, rc)
        assert lib.pp_last_error(), kw
    bad_keep = [dict(cls=None), dict(out=None), dict(stats=None), dict(ws=None), dict(n=0), dict(h=0), dict(w=0), dict(k=0), dict(k=33),
                dict(c=3), dict(c=0), dict(n=1 << 11, h=1 << 10, w=1 << 10), dict(nws=need - 1), dict(nws=0)]
    for kw in bad_keep:
        rc = keep(**kw)
        assert rc < 0, (kw, rc)
        assert lib.pp_last_error(), kw
    assert b'connectivity' in (keep(c=3) and lib.pp_last_error())
    assert b'K=33' in (keep(k=33) and lib.pp_last_error())
    assert b'workspace' in (keep(nws=need - 1) and lib.pp_last_error())
    assert b'null' in (label(cls=None) and lib.pp_last_error())
