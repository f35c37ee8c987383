"""--rw_scribbles without a GPU: the float64 oracle of the GPU tests checked against the definition's own properties, the C ABI of
the companion library against its binding, the parameter checks and the parser, the data-set substitution, resume compatibility
with state files older than the flags, and the sanitizer run of the library's host side."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _rw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rw_scribbles', 'rw_beta', 'rw_threshold', 'rw_eps', 'rw_tol', 'rw_max_iters')
ENTRIES = ('pprep_version', 'pprep_last_error', 'pprep_rw_workspace_bytes', 'pprep_rw_solve', 'pprep_rw_labels')


def _random_case(h, w, K, seed, every_class=True):
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 1, (h, w)).astype(np.float32)
    scb = np.full((h, w), K, np.int64)
    flat = rng.permutation(h * w)
    for k in range(K if every_class else K - 1):
        scb.flat[flat[2 * k]] = k
        scb.flat[flat[2 * k + 1]] = k
    return img, scb


# ---- the oracle against the definition --------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,K,seed', [(8, 8, 2, 0), (9, 13, 3, 1), (16, 16, 5, 2), (32, 32, 5, 3), (32, 17, 4, 4)])
def test_oracle_is_a_probability_and_harmonic(h, w, K, seed):
    img, scb = _random_case(h, w, K, seed)
    prob = R.rw_prob(img, scb, K)
    assert np.abs(prob.sum(0) - 1.0).max() <= 1e-10                        # every class seeded: the K solutions sum to one
    assert prob.min() >= -1e-12 and prob.max() <= 1 + 1e-12
    for k in range(K):                                                     # seeds are one-hot
        assert np.array_equal(prob[k][scb < K], (scb[scb < K] == k).astype(np.float64))
    wr, wd = R.edge_weights(img)
    num, den = np.zeros((K, h, w)), np.zeros((h, w))
    num[:, :, :-1] += wr * prob[:, :, 1:]; den[:, :-1] += wr
    num[:, :, 1:] += wr * prob[:, :, :-1]; den[:, 1:] += wr
    num[:, :-1, :] += wd * prob[:, 1:, :]; den[:-1, :] += wd
    num[:, 1:, :] += wd * prob[:, :-1, :]; den[1:, :] += wd
    unk = scb == K
    assert np.abs(num / den - prob)[:, unk].max() <= 1e-10                 # an unknown = the weighted mean of its neighbours


def test_oracle_seedless_class_is_exactly_zero():
    img, scb = _random_case(16, 16, 4, 5, every_class=False)
    prob = R.rw_prob(img, scb, 4)
    assert not prob[3].any() and np.abs(prob[:3].sum(0) - 1.0).max() <= 1e-10
    none = R.rw_prob(img, np.full((16, 16), 4), 4)
    assert not none.any() and (R.rw_labels(none, np.full((16, 16), 4), 4) == 4).all()


def test_oracle_chain_is_the_linear_ramp():
    scb = np.array([[0, 2, 2, 2, 2, 2, 1]])
    prob = R.rw_prob(np.full((1, 7), 3.0, np.float32), scb, 2)
    assert np.abs(prob[1, 0] - np.arange(7) / 6.0).max() <= 1e-10 and np.abs(prob[0, 0] - (1 - np.arange(7) / 6.0)).max() <= 1e-10
    lab = R.rw_labels(prob, scb, 2, 0.6)
    assert lab.tolist() == [[0, 0, 0, 2, 1, 1, 1]]
    assert R.undecided(prob, 0.5)[0].tolist() == [False, False, False, True, False, False, False]
    assert abs(R.relres(np.full((1, 7), 3.0), scb, 2, 1, prob[1])) <= 1e-12


def test_gpu_cases_leave_few_pixels_undecided():
    """The share of pixels the GPU label test may leave out, for the cases it uses, from the oracle alone: under its 2 % cap."""
    for seed in (0, 1, 2):
        img, _, scb = R.phantom(seed, 32, 5)
        prob = R.rw_prob(img, scb, 5)
        for tau in (0.5, 0.9):
            assert R.undecided(prob, tau)[scb == 5].mean() <= 0.02, (seed, tau)


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_prep.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(pprep_\w+)\s*\(([^;{]*)\)\s*;', header):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ('', 'void') else len(args.split(','))
    return out


def test_header_and_binding_agree():
    from pacingpseudo_amd import _prep
    decls = _header_decls()
    assert set(decls) == set(_prep._PROTOS) == set(ENTRIES) and _prep.EXPORTED_SYMBOLS == tuple(_prep._PROTOS)
    for name, (_, argtypes) in _prep._PROTOS.items():
        assert len(argtypes) == decls[name], name
    assert not any(n.startswith('pprep_') for n in __import__('pacingpseudo_amd._lib', fromlist=['x'])._PROTOS)
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'prep', 'pp_random_walker.hip')).read()
    assert int(re.search(r'#define PPREP_VERSION (\d+)', src).group(1)) == _prep.MIN_PREP_VERSION


def test_library_loads_without_a_gpu():
    from pacingpseudo_amd import _prep
    if not os.path.exists(_prep.PREP_LIB_PATH):
        pytest.skip('libpacingpseudo_prep.so is not built')
    dll = _prep._PrepLib().load()
    for name in _prep.EXPORTED_SYMBOLS:
        getattr(dll, name)
    assert _prep.prep.pprep_version() >= _prep.MIN_PREP_VERSION
    assert _prep.prep.pprep_rw_workspace_bytes(2, 5, 40, 48) >= 2 * (3 + 15) * 40 * 48 * 4
    assert _prep.prep.pprep_rw_workspace_bytes(2, 33, 40, 48) == 0 and b'K = 33' in _prep.prep.pprep_last_error()
    with pytest.raises(_prep.HipLibraryError, match='null pointer'):
        _prep.prep.pprep_rw_solve(None, None, None, 1, 5, 8, 8, 13.0, 1e-4, 1e-6, 10, None, None, None, None)


def test_missing_or_stale_library_raises(tmp_path, monkeypatch):
    from pacingpseudo_amd import _prep
    with pytest.raises(_prep.HipLibraryError, match='is missing'):
        _prep._PrepLib(str(tmp_path / 'libpacingpseudo_prep.so')).load()
    if not os.path.exists(_prep.PREP_LIB_PATH):
        pytest.skip('libpacingpseudo_prep.so is not built')
    monkeypatch.setattr(_prep, 'MIN_PREP_VERSION', 10 ** 6)
    with pytest.raises(_prep.HipLibraryError, match='pprep_version'):
        _prep._PrepLib().load()
    monkeypatch.undo()
    monkeypatch.setitem(_prep._PROTOS, 'pprep_not_there', (_prep.i32, []))
    with pytest.raises(_prep.HipLibraryError, match='pprep_not_there'):
        _prep._PrepLib().load()


# ---- parameters, parser, types -------------------------------------------------------------------------------------------------
def test_check_rw_params():
    from pacingpseudo_amd.utils import check_rw_params
    assert check_rw_params() == dict(beta=13.0, eps=1e-4, tol=1e-6, max_iters=10000, threshold=0.9)
    assert check_rw_params(0, 1, 1, 1, 1.0, K=32)['threshold'] == 1.0 and check_rw_params(K=1)['beta'] == 13.0
    for kw in (dict(beta=-1), dict(beta=float('nan')), dict(beta=float('inf')), dict(eps=0), dict(eps=-1e-4), dict(tol=0), dict(tol=float('nan')),
               dict(max_iters=0), dict(max_iters=2.5), dict(max_iters=True), dict(threshold=0), dict(threshold=1.01), dict(threshold=float('nan')),
               dict(K=0), dict(K=2.5)):
        with pytest.raises(ValueError, match='random walker'):
            check_rw_params(**kw)
    with pytest.raises(NotImplementedError, match='32'):
        check_rw_params(K=33)


def test_parser_defaults_and_rejections():
    from pacingpseudo_amd.train import parse_args, parser
    a = parse_args(['--tag', 'x'])
    assert (a.rw_scribbles, a.rw_beta, a.rw_threshold, a.rw_eps, a.rw_tol, a.rw_max_iters) == (False, 13.0, 0.9, 1e-4, 1e-6, 10000)
    on = parse_args(['--tag', 'x', '--rw_scribbles', '--rw_beta', '5', '--rw_threshold', '0.5', '--rw_max_iters', '7'])
    assert on.rw_scribbles and on.rw_beta == 5.0 and on.rw_threshold == 0.5 and on.rw_max_iters == 7 and on.max_iters == 0
    for bad in (['--rw_beta', '-1'], ['--rw_eps', '0'], ['--rw_tol', '0'], ['--rw_max_iters', '0'], ['--rw_threshold', '0'],
                ['--rw_threshold', '1.5'], ['--rw_beta', 'nan'], ['--rw_max_iters', '2.5']):
        with pytest.raises(SystemExit) as e:
            parse_args(['--tag', 'x'] + bad)
        assert e.value.code == 2, bad
    helps = {o: a.help for a in parser._actions for o in a.option_strings}
    assert all('untuned' in helps[o] for o in ('--rw_beta', '--rw_threshold', '--rw_eps'))
    from pacingpseudo_amd.upper_bound import parser as ub                  # the fully-supervised driver has no such flag
    assert not any(o.startswith('--rw_') for a in ub._actions for o in a.option_strings)


def test_cpu_tensors_and_wrong_types_are_refused_before_the_library():
    from pacingpseudo_amd.utils import expand_scribbles, random_walker
    img, scb = torch.zeros(1, 8, 8), torch.full((1, 8, 8), 2, dtype=torch.int64)
    for f in (random_walker, expand_scribbles):
        with pytest.raises(TypeError, match='CUDA'):
            f(img, scb, 2)
        with pytest.raises(TypeError, match='torch tensor'):
            f(img.numpy(), scb, 2)
        with pytest.raises(ValueError, match='random walker'):
            f(img, scb, 2, eps=0.0)
    with pytest.raises(ValueError, match='threshold'):
        expand_scribbles(img, scb, 2, None, 0.0)


# ---- the data set -------------------------------------------------------------------------------------------------------------
def _equal_items(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (v.numpy() if torch.is_tensor(v) else v for v in (a[k], b[k]))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize('raw', [True, False])
def test_scribble_override_replaces_scb(raw, tmp_path):
    from pacingpseudo_amd.data import NpzSlices, SyntheticPhantoms
    K, S = 3, 16
    syn = SyntheticPhantoms(3, K, size=S, raw=raw, do_strong=not raw)
    assert syn.scribble_override is None
    plain = [syn[i] for i in range(3)]
    maps = [np.full((S, S), i % K, np.uint8) for i in range(3)]
    files = []
    for i in range(3):
        img, lab, scb = syn.raw_arrays(i)
        files.append(str(tmp_path / f's{i}.npz'))
        np.savez(files[-1], uid=i, img=img, lab=lab, scb=scb)
    npz = NpzSlices(files, K, size=S, raw=raw, do_strong=not raw)
    for ds in (syn, npz):
        for i in range(3):
            _equal_items(ds[i], plain[i])                                   # None: byte-identical items, from either reader
        ds.scribble_override = maps
        for i in (2, 0, 1):
            d = ds[i]
            if raw:
                assert d['scb'].dtype == np.int32 and (d['scb'] == i % K).all()
                assert d['img'].tobytes() == plain[i]['img'].tobytes() and d['lab'].tobytes() == plain[i]['lab'].tobytes()
            else:
                assert d['scribble'].shape == (K + 1, S, S) and bool((d['scribble'][i % K] == 1).all()) and float(d['scribble'].sum()) == S * S
                assert torch.equal(d['image'], plain[i]['image']) and torch.equal(d['label'], plain[i]['label'])
        ds.scribble_override = None
        _equal_items(ds[1], plain[1])
    val = SyntheticPhantoms(2, K, size=S, train=False, native=True, compact=True)
    val.scribble_override = [np.zeros((S, S), np.uint8)] * 2               # every kind of item goes through the one substitution
    assert not val[1]['scribble_idx'].any()


# ---- resume -------------------------------------------------------------------------------------------------------------------
def test_resume_compatibility_in_both_directions():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    new = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x'])))
    for n in NAMES:
        assert n not in resume.MAY_DIFFER and resume.ABSENT_DEFAULTS[n] == new[n], n
    saved = {k: v for k, v in new.items() if k not in NAMES}
    resume.check_compatible(saved, new, 1, 1)                               # absent from the file = off, the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--rw_scribbles'])))
    with pytest.raises(resume.ResumeError, match='--rw_scribbles'):
        resume.check_compatible(saved, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--rw_scribbles'):
        resume.check_compatible(on, new, 1, 1)
    other = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--rw_scribbles', '--rw_threshold', '0.5'])))
    with pytest.raises(resume.ResumeError, match='--rw_threshold'):
        resume.check_compatible(on, other, 1, 1)
    with pytest.raises(resume.ResumeError, match='--rw_threshold'):
        resume.check_compatible(other, on, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


# ---- the host side under AddressSanitizer ---------------------------------------------------------------------------------------
def test_prep_host_side_under_address_sanitizer():
    """`make asan-prep` instruments the host half of pp_random_walker.hip and runs tests/native/asan_prep_args.cpp, a program of
    its own that feeds invalid arguments to every pprep_* entry point.  No GPU needed: every call must be rejected before anything
    is launched, without a sanitizer report."""
    import shutil
    import subprocess
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-prep'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout and 'AddressSanitizer' not in r.stdout + r.stderr
