"""--rw_refresh without a GPU: the float64 oracle of the GPU tests checked against the definition's own properties, the C ABI of
the third library against its binding, the parameter checks and the parser, resume compatibility with state files older than the
flags, the shared-memory maps under a loader with persistent workers, and the sanitizer run of the library's host side."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _rw_prior_reference as P
from tests import _rw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rw_refresh', 'rw_refresh_start', 'rw_prior_gamma')
ENTRIES = ('prwp_version', 'prwp_last_error', 'prwp_workspace_bytes', 'prwp_solve')
GAMMAS = (0.01, 0.1, 1.0)


@pytest.fixture(scope='module')
def phantoms():
    """The three 32 x 32 K = 5 phantoms with their test prior and the oracle's probabilities per gamma, computed once."""
    cases = []
    for seed in (0, 1, 2):
        img, lab, scb = R.phantom(seed, 32, 5)
        z = P.prior_logits(seed, lab, 5)
        cases.append(dict(img=img, lab=lab, scb=scb, z=z, prob={g: P.rw_prob(img, scb, z, 5, g) for g in GAMMAS}))
    return cases


# ---- the oracle against the definition --------------------------------------------------------------------------------------
def test_oracle_gamma_zero_is_the_plain_walker(phantoms):
    c = phantoms[0]
    assert np.array_equal(P.rw_prob(c['img'], c['scb'], c['z'], 5, 0.0), R.rw_prob(c['img'], c['scb'], 5))
    tiny = P.rw_prob(c['img'], c['scb'], c['z'], 5, 1e-12)                  # ... and the limit of the shifted system
    assert np.abs(tiny - R.rw_prob(c['img'], c['scb'], 5)).max() <= 1e-6


def test_oracle_sums_to_one_and_keeps_the_seeds(phantoms):
    for c in phantoms:
        for g, prob in c['prob'].items():
            assert np.abs(prob.sum(0) - 1.0).max() <= 1e-12, g
            assert prob.min() >= -1e-12 and prob.max() <= 1 + 1e-12
            for k in range(5):
                assert np.array_equal(prob[k][c['scb'] < 5], (c['scb'][c['scb'] < 5] == k).astype(np.float64))
                assert abs(P.relres(c['img'], c['scb'], c['z'], 5, g, k, prob[k])) <= 1e-12


def test_oracle_unseeded_systems():
    """gamma > 0: a class without a seed is an ordinary system; without any seed and with a constant prior the answer is the prior."""
    img, lab, scb = R.phantom(0, 32, 5)
    z = P.prior_logits(0, lab, 5)
    scb2 = np.where(scb == 2, 5, scb)
    prob = P.rw_prob(img, scb2, z, 5, 0.1)
    assert prob[2].max() > 0.5 and np.abs(prob.sum(0) - 1.0).max() <= 1e-12
    const = np.broadcast_to(np.array([0.3, -1.0, 2.0])[:, None, None], (3, 16, 16)).astype(np.float32)
    flat = P.rw_prob(np.full((16, 16), 4.0, np.float32), np.full((16, 16), 3), const, 3, 0.1)
    assert np.abs(flat - P.softmax(const)).max() <= 1e-12                   # L const = 0
    lone = P.rw_prob(np.ones((1, 1), np.float32), np.full((1, 1), 3), const[:, :1, :1], 3, 0.5)
    assert np.abs(lone - P.softmax(const[:, :1, :1])).max() <= 1e-14


def test_oracle_differs_from_the_plain_walker_and_leaves_few_pixels_undecided(phantoms):
    """The share of pixels the GPU label test may leave out, for exactly the cases it uses, from the oracle alone: under its 2 % cap.
    The labels differ from the plain walker's, so that test cannot pass on the plain walker."""
    for n, c in enumerate(phantoms):
        plain = R.rw_prob(c['img'], c['scb'], 5)
        for g in GAMMAS:
            for tau in (0.5, 0.9):
                assert R.undecided(c['prob'][g], tau)[c['scb'] == 5].mean() <= 0.02, (n, g, tau)
                differ = (R.rw_labels(c['prob'][g], c['scb'], 5, tau) != R.rw_labels(plain, c['scb'], 5, tau)).mean()
                assert differ >= 0.01, (n, g, tau, differ)


def test_truncation_error_of_the_shifted_system(phantoms):
    """smallest eigenvalue >= gamma, so the iterate the rule stops at lies within tol ||rhs|| / gamma of the solution."""
    c = phantoms[1]
    for g in GAMMAS:
        te = P.truncation_error(c['img'], c['scb'], c['z'], 5, g)
        rhs = np.linalg.norm(P.system(c['img'], c['scb'], c['z'], 5, g)[1], axis=0)
        assert (te > 0).all() and (te <= 1e-6 * rhs / g).all(), (g, te.tolist(), rhs.tolist())
    assert np.array_equal(P.truncation_error(c['img'], c['scb'], c['z'], 5, 0.0), R.truncation_error(c['img'], c['scb'], 5))


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_rwp.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(prwp_\w+)\s*\(([^;{]*)\)\s*;', header):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ('', 'void') else len(args.split(','))
    return out


def test_header_and_binding_agree():
    from pacingpseudo_amd import _lib, _prep, _rwp
    decls = _header_decls()
    assert set(decls) == set(_rwp._PROTOS) == set(ENTRIES) and _rwp.EXPORTED_SYMBOLS == tuple(_rwp._PROTOS)
    for name, (_, argtypes) in _rwp._PROTOS.items():
        assert len(argtypes) == decls[name], name
    assert not any(n.startswith('prwp_') for n in list(_lib._PROTOS) + list(_prep._PROTOS))
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'prep', 'pp_rw_prior.hip')).read()
    assert int(re.search(r'#define PRWP_VERSION (\d+)', src).group(1)) == _rwp.MIN_RWP_VERSION
    assert 'getenv' not in src                                              # no new environment switch


def _need_lib():
    from pacingpseudo_amd import _rwp
    if not os.path.exists(_rwp.RWP_LIB_PATH):
        pytest.skip('libpacingpseudo_rwp.so is not built')
    return _rwp


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    _rwp = _need_lib()
    dll = _rwp._RwpLib().load()
    for name in _rwp.EXPORTED_SYMBOLS:
        getattr(dll, name)
    lib = _rwp.rwp
    assert lib.prwp_version() >= _rwp.MIN_RWP_VERSION
    assert lib.prwp_workspace_bytes(2, 5, 40, 48) >= 2 * (3 + 15) * 40 * 48 * 4
    assert lib.prwp_workspace_bytes(2, 33, 40, 48) == 0 and b'K = 33' in lib.prwp_last_error()
    assert lib.prwp_workspace_bytes(2, 5, 1025, 48) == 0 and b'H = 1025' in lib.prwp_last_error()
    with pytest.raises(_rwp.HipLibraryError, match='null pointer'):
        lib.prwp_solve(None, None, None, None, 1, 5, 8, 8, 13.0, 1e-4, 0.1, 1e-6, 10, None, None, None, None)
    fake = 4096                                                             # a non-null, aligned address: rejected before any use
    for gamma, msg in ((-0.1, 'gamma = -0.1'), (float('nan'), 'gamma = nan'), (float('inf'), 'gamma = inf')):
        with pytest.raises(_rwp.HipLibraryError, match=msg):
            lib.prwp_solve(fake, fake, fake, None, 1, 5, 8, 8, 13.0, 1e-4, gamma, 1e-6, 10, fake, fake, fake, None)
    with pytest.raises(_rwp.HipLibraryError, match=r'rc=-2.*K = 33'):
        lib.prwp_solve(fake, fake, fake, None, 1, 33, 8, 8, 13.0, 1e-4, 0.1, 1e-6, 10, fake, fake, fake, None)
    with pytest.raises(_rwp.HipLibraryError, match=r'rc=-2.*W = 1025'):
        lib.prwp_solve(fake, fake, fake, None, 1, 5, 8, 1025, 13.0, 1e-4, 0.1, 1e-6, 10, fake, fake, fake, None)


def test_missing_or_stale_library_raises(tmp_path, monkeypatch):
    from pacingpseudo_amd import _rwp
    with pytest.raises(_rwp.HipLibraryError, match='is missing'):
        _rwp._RwpLib(str(tmp_path / 'libpacingpseudo_rwp.so')).load()
    _need_lib()
    monkeypatch.setattr(_rwp, 'MIN_RWP_VERSION', 10 ** 6)
    with pytest.raises(_rwp.HipLibraryError, match='prwp_version'):
        _rwp._RwpLib().load()
    monkeypatch.undo()
    monkeypatch.setitem(_rwp._PROTOS, 'prwp_not_there', (_rwp.i32, []))
    with pytest.raises(_rwp.HipLibraryError, match='prwp_not_there'):
        _rwp._RwpLib().load()


# ---- parameters, parser, types -------------------------------------------------------------------------------------------------
def test_check_rw_prior_params():
    from pacingpseudo_amd.utils import check_rw_prior_params
    assert check_rw_prior_params() == 0.1 and check_rw_prior_params(0) == 0.0 and check_rw_prior_params(7) == 7.0
    for bad in (-1e-3, float('nan'), float('inf'), True):
        with pytest.raises(ValueError, match='gamma'):
            check_rw_prior_params(bad)


def test_parser_defaults_and_rejections():
    from pacingpseudo_amd.train import parse_args, parser
    a = parse_args(['--tag', 'x'])
    assert (a.rw_refresh, a.rw_refresh_start, a.rw_prior_gamma) == (0, 0, 0.1)
    on = parse_args(['--tag', 'x', '--rw_refresh', '5', '--rw_refresh_start', '20', '--rw_prior_gamma', '0'])
    assert (on.rw_refresh, on.rw_refresh_start, on.rw_prior_gamma, on.rw_scribbles) == (5, 20, 0.0, False)
    for bad in (['--rw_refresh', '-1'], ['--rw_refresh', '2.5'], ['--rw_refresh_start', '-3'], ['--rw_prior_gamma', '-0.1'],
                ['--rw_prior_gamma', 'nan'], ['--rw_prior_gamma', 'inf']):
        with pytest.raises(SystemExit) as e:
            parse_args(['--tag', 'x'] + bad)
        assert e.value.code == 2, bad
    helps = {o: a.help for a in parser._actions for o in a.option_strings}
    assert 'untuned' in helps['--rw_prior_gamma']
    from pacingpseudo_amd.upper_bound import parser as ub                  # the fully-supervised driver has none of the three
    assert not any(o.lstrip('-') in NAMES for a in ub._actions for o in a.option_strings)


def test_refresh_epochs():
    from pacingpseudo_amd.utils.random_walker import refresh_epochs
    assert refresh_epochs(0, 0, 100) == [] and refresh_epochs(5, 0, 16) == [5, 10, 15] and refresh_epochs(5, 2, 12) == [2, 7, 12]
    assert refresh_epochs(1, 1, 0) == []


def test_cpu_tensors_and_wrong_types_are_refused_before_the_library(monkeypatch):
    from pacingpseudo_amd import _rwp
    from pacingpseudo_amd.utils import random_walker_prior, refresh_scribbles
    monkeypatch.setattr(_rwp.rwp, '_path', '/nonexistent/libpacingpseudo_rwp.so')      # touching the library would raise HipLibraryError
    monkeypatch.setattr(_rwp.rwp, '_dll', None)
    img, scb, z = torch.zeros(1, 8, 8), torch.full((1, 8, 8), 2, dtype=torch.int64), torch.zeros(1, 2, 8, 8)
    for f in (random_walker_prior, refresh_scribbles):
        with pytest.raises(TypeError, match='CUDA'):
            f(img, scb, z, 2)
        with pytest.raises(TypeError, match='torch tensor'):
            f(img, scb, z.numpy(), 2)
        with pytest.raises(TypeError, match='torch tensor'):
            f(img.numpy(), scb, z, 2)
        with pytest.raises(ValueError, match='gamma'):
            f(img, scb, z, 2, gamma=-1.0)
        with pytest.raises(ValueError, match='random walker'):
            f(img, scb, z, 2, eps=0.0)
    with pytest.raises(ValueError, match='threshold'):
        refresh_scribbles(img, scb, z, 2, None, 0.0)


# ---- resume -------------------------------------------------------------------------------------------------------------------
def test_resume_compatibility_in_both_directions():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    new = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x'])))
    for n in NAMES:
        assert n not in resume.MAY_DIFFER and resume.ABSENT_DEFAULTS[n] == new[n], n
    saved = {k: v for k, v in new.items() if k not in NAMES}
    resume.check_compatible(saved, new, 1, 1)                               # absent from the file = off, the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--rw_refresh', '5'])))
    with pytest.raises(resume.ResumeError, match='--rw_refresh'):
        resume.check_compatible(saved, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--rw_refresh'):
        resume.check_compatible(on, new, 1, 1)
    for extra, name in ((['--rw_prior_gamma', '0.5'], '--rw_prior_gamma'), (['--rw_refresh_start', '2'], '--rw_refresh_start')):
        other = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--rw_refresh', '5'] + extra)))
        with pytest.raises(resume.ResumeError, match=name):
            resume.check_compatible(on, other, 1, 1)
        with pytest.raises(resume.ResumeError, match=name):
            resume.check_compatible(other, on, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


def test_refresh_maps_files(tmp_path):
    """maps_<t>.npz round-trips ragged maps; a run resumed after epoch e reads the largest refresh epoch t <= e, and says which
    file it misses."""
    from pacingpseudo_amd import resume
    rng = np.random.default_rng(0)
    maps = [rng.integers(0, 6, s).astype(np.uint8) for s in ((4, 5), (1, 1), (7, 3))]
    shapes = [m.shape for m in maps]
    rep = dict(changed=np.array([0.5, 0.0, 1.0]), skipped=np.array([False, True, False]))
    for t in (2, 5):
        resume.save_refresh_maps(resume.refresh_maps_path(str(tmp_path), t), [m + (t == 5) for m in maps], rep, dict(gamma=0.1))
    assert sorted(os.listdir(tmp_path / 'rw_refresh')) == ['maps_2.npz', 'maps_5.npz']      # no temporary file left
    z = np.load(resume.refresh_maps_path(str(tmp_path), 2))
    assert z['maps'].dtype == np.uint8 and z['param_gamma'] == 0.1 and z['report_skipped'].tolist() == [False, True, False]
    assert resume.load_refresh_maps(str(tmp_path), 1, 3, 2, shapes) is None and resume.load_refresh_maps(str(tmp_path), 9, 0, 0, shapes) is None
    for e, plus in ((2, 0), (4, 0), (5, 1), (7, 1)):
        got = resume.load_refresh_maps(str(tmp_path), e, 3, 2, shapes)
        assert all(np.array_equal(a, b + plus) for a, b in zip(got, maps)), e
    with pytest.raises(resume.ResumeError, match=r'maps_8\.npz'):
        resume.load_refresh_maps(str(tmp_path), 9, 3, 2, shapes)
    with pytest.raises(resume.ResumeError, match='one map per training slice'):
        resume.load_refresh_maps(str(tmp_path), 2, 3, 2, shapes[:2])


# ---- the shared maps ----------------------------------------------------------------------------------------------------------
def test_shared_maps_basics():
    from pacingpseudo_amd.utils import SharedMaps
    maps = [np.full((3, 4), 1, np.uint8), np.full((1, 1), 2, np.uint8), np.arange(10, dtype=np.uint8).reshape(5, 2)]
    sm = SharedMaps(maps)
    assert len(sm) == 3 and sm.buffer.is_shared() and sm.buffer.numel() == 23
    assert all(sm[i].shape == m.shape and sm[i].dtype == np.uint8 and np.array_equal(sm[i], m) for i, m in enumerate(maps))
    sm.update(2, maps[2] + 1)
    assert np.array_equal(sm[2], maps[2] + 1) and np.array_equal(sm[0], maps[0]) and np.array_equal(sm[1], maps[1])
    with pytest.raises(ValueError):
        sm.update(0, np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError):
        sm.update(0, np.zeros((3, 4), np.int64))
    with pytest.raises(IndexError):
        sm[3]
    with pytest.raises(TypeError):
        SharedMaps([np.zeros((2, 2), np.int32)])


def _collate(items):
    return np.stack([it['scb'] for it in items])


def test_shared_maps_reach_persistent_workers_and_a_replaced_list_does_not():
    from pacingpseudo_amd.data import SyntheticPhantoms, loader_context
    from pacingpseudo_amd.utils import SharedMaps
    K, S, n = 3, 16, 4
    old = [np.full((S, S), 0, np.uint8) for _ in range(n)]
    new = [np.full((S, S), 1 + i % 2, np.uint8) for i in range(n)]

    def two_passes(install, change):
        ds = SyntheticPhantoms(n, K, size=S, raw=True)
        ds.scribble_override = install(old)
        loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=1, persistent_workers=True, collate_fn=_collate,
                                             multiprocessing_context=loader_context(1))
        first = np.concatenate(list(loader))
        change(ds)
        second = np.concatenate(list(loader))
        del loader
        return first, second

    def in_place(ds):
        for i, m in enumerate(new):
            ds.scribble_override.update(i, m)

    first, second = two_passes(SharedMaps, in_place)
    assert first.dtype == np.int32 and np.array_equal(first, np.stack(old)) and np.array_equal(second, np.stack(new))
    # the failure the class exists for: the workers hold their own copy of a list
    first, second = two_passes(list, lambda ds: setattr(ds, 'scribble_override', new))
    assert np.array_equal(first, np.stack(old)) and np.array_equal(second, np.stack(old))


# ---- the host side under AddressSanitizer ---------------------------------------------------------------------------------------
def test_rwp_host_side_under_address_sanitizer():
    """`make asan-rwp` instruments the host half of pp_rw_prior.hip and runs tests/native/asan_rwp_args.cpp, a program of its own
    that feeds invalid arguments to every prwp_* entry point.  No GPU needed: every call must be rejected before anything is
    launched, without a sanitizer report."""
    import shutil
    import subprocess
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-rwp'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout and 'AddressSanitizer' not in r.stdout + r.stderr
