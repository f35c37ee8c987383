"""Uncertainty mask of the mean-teacher consistency term (--cr_uncertainty), the parts that need no GPU: the float64 reference's
generator against the published Philox-4x32-10 known-answer vectors, the parser's rules, the parameter checks, the threshold
schedule, the resume tables, the output keys, and header / binding / library agreeing symbol for symbol."""
import math
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _unc_reference as R  # noqa: E402

FLAGS = ('cr_uncertainty', 'cr_uncertainty_sigma', 'cr_uncertainty_clip', 'cr_uncertainty_start')
DEFAULTS = dict(cr_uncertainty=0, cr_uncertainty_sigma=0.1, cr_uncertainty_clip=0.2, cr_uncertainty_start=0.75)
TEACHER = ['--tag', 'x', '--do_decoder_consistency', '--cr_teacher', 'ema', '--ema_decay', '0.99']


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('counter,key,expect', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_reference_philox_reproduces_the_known_answer_vectors(counter, key, expect):
    got = tuple(int(v[0]) for v in R.philox4x32_10(counter, key))
    assert got == expect, [hex(v) for v in got]


def test_reference_noise_depends_on_the_element_index_alone():
    a = R.normals(1027, seed=7, step=2 ** 32 + 5, pass_index=3)
    assert np.array_equal(a[:35], R.normals(35, 7, 2 ** 32 + 5, 3))
    assert not np.array_equal(a[:35], R.normals(35, 7, 2 ** 32 + 5, 2)) and not np.array_equal(a[:35], R.normals(35, 7, 5, 3))
    assert not np.array_equal(a[:35], R.normals(35, 7 + 2 ** 32, 2 ** 32 + 5, 3))
    big = R.normals(200000, 1, 0, 0)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1.0) < 0.01
    u = R.uniforms(np.array([0, 0xffffffff], dtype=np.uint64))
    assert 0.0 < u[0] < u[1] < 1.0
    n = R.noise(4096, 0.1, 0.05, 1, 0, 0)
    assert n.min() == -0.05 and n.max() == 0.05 and (np.abs(n) < 0.05).any()


def test_reference_entropy_mask_and_stats():
    z = np.zeros((1, 4, 1, 2))
    z[0, 0, 0, 1] = 80.0
    z[0, 1:, 0, 1] = -80.0
    u = R.entropy(R.mean_softmax([z]))
    assert abs(u[0, 0, 0] - math.log(4)) < 1e-12 and 0.0 <= u[0, 0, 1] < 1e-30
    v = np.array([[[1.0, 0.0]]])
    m = R.mask(u, 1.0, v)
    assert m.tolist() == [[[0.0, 0.0]]] and R.mask(u, 1.0).tolist() == [[[0.0, 1.0]]]
    assert R.stats(u, R.mask(u, 1.0)).tolist() == [1.0, float(u.sum()), 2.0]


# ---------------------------------------------------------------- parser
def test_parser_defaults_and_rules():
    from pacingpseudo_amd import train
    a = train.parse_args(['--tag', 'x'])
    assert {k: getattr(a, k) for k in FLAGS} == DEFAULTS
    a = train.parse_args(TEACHER + ['--cr_uncertainty', '4', '--cr_uncertainty_sigma', '0.2', '--cr_uncertainty_clip', '0.3',
                                    '--cr_uncertainty_start', '1.0'])
    assert (a.cr_uncertainty, a.cr_uncertainty_sigma, a.cr_uncertainty_clip, a.cr_uncertainty_start) == (4, 0.2, 0.3, 1.0)
    assert train.parse_args(TEACHER + ['--cr_uncertainty', '1', '--cr_uncertainty_sigma', '0']).cr_uncertainty == 1
    for name in FLAGS:
        assert '_nc' not in name and '_ms' not in name and not name.startswith(('crf', 'rw_', 'nc_', 'ms_'))
    help_text = train.parser.format_help()
    for act in train.parser._actions:
        if act.dest in FLAGS:
            assert 'untuned first value' in act.help, act.dest
    assert '--cr_uncertainty_start' in help_text


@pytest.mark.parametrize('argv', [
    ['--tag', 'x', '--cr_uncertainty', '4'],                                              # no teacher
    ['--tag', 'x', '--do_decoder_consistency', '--cr_uncertainty', '2'],
    TEACHER + ['--cr_uncertainty', '1', '--num_classes', '1'],                            # K = 1
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_sigma', '0'],                   # sigma = 0 with T != 1
    TEACHER + ['--cr_uncertainty', '17'],
    TEACHER + ['--cr_uncertainty', '-1'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_sigma', '-0.1'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_sigma', 'nan'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_clip', '-1'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_clip', 'inf'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_start', '0'],
    TEACHER + ['--cr_uncertainty', '2', '--cr_uncertainty_start', '1.01'],
    TEACHER + ['--cr_uncertainty', '2.5'],
])
def test_parser_refuses_with_exit_status_2(argv, capsys, monkeypatch):
    from pacingpseudo_amd import _unc, train
    with pytest.raises(SystemExit) as e:
        train.parse_args(argv)
    assert e.value.code == 2
    assert 'cr_uncertainty' in capsys.readouterr().err
    assert _unc.unc._dll is None          # refused before any device call: the library was not even loaded


def test_the_upper_bound_driver_has_none_of_the_flags():
    from pacingpseudo_amd import upper_bound
    dests = {a.dest for a in upper_bound.parser._actions}
    assert not [d for d in dests if 'uncertainty' in d]


# ---------------------------------------------------------------- parameter checks
def test_check_uncertainty_params():
    from pacingpseudo_amd.utils import check_uncertainty_params as chk
    assert chk(4, 0.1, 0.2, 0.75, 3, K=5) == dict(passes=4, sigma=0.1, clip=0.2, start=0.75, seed=3)
    assert chk(1, 0, 0, 1.0, 2 ** 64 - 1, K=32)['sigma'] == 0.0
    assert chk(16, 1.0, 0.0, 0.01, 0, K=2)['passes'] == 16
    for bad in (dict(passes=0), dict(passes=-2), dict(passes=2.5), dict(passes=True), dict(passes='4'), dict(sigma=-0.1),
                dict(sigma=float('nan')), dict(sigma=float('inf')), dict(clip=-0.1), dict(clip=float('nan')), dict(start=0.0),
                dict(start=-0.5), dict(start=1.5), dict(start=float('nan')), dict(passes=2, sigma=0.0), dict(seed=-1),
                dict(seed=2 ** 64), dict(seed=1.5), dict(K=1), dict(K=0)):
        with pytest.raises(ValueError):
            chk(**{**dict(passes=2, sigma=0.1, clip=0.2, start=0.75, seed=0, K=5), **bad})
    for bad in (dict(passes=17), dict(K=33)):
        with pytest.raises(NotImplementedError):
            chk(**{**dict(passes=2, sigma=0.1, clip=0.2, start=0.75, seed=0, K=5), **bad})


def test_cpu_tensors_are_refused_before_the_library():
    import torch
    from pacingpseudo_amd import _unc
    from pacingpseudo_amd.utils import add_noise, uncertainty_mask
    with pytest.raises(ValueError):
        add_noise(torch.zeros(2, 1, 4, 4), 0.1, 0.2, 0, 0, 0)
    with pytest.raises(ValueError):
        add_noise(np.zeros(4), 0.1, 0.2, 0, 0, 0)
    with pytest.raises(ValueError):
        uncertainty_mask([torch.zeros(1, 5, 4, 4)], 1.0)
    with pytest.raises(ValueError):
        uncertainty_mask([], 1.0)
    with pytest.raises(ValueError):
        uncertainty_mask([torch.zeros(1, 5, 4, 4)], float('nan'))
    assert _unc.unc._dll is None


# ---------------------------------------------------------------- threshold schedule
@pytest.mark.parametrize('K', [2, 5, 32])
@pytest.mark.parametrize('scale', [5.0, 8.0, 10.0])
@pytest.mark.parametrize('start', [0.25, 0.75, 1.0])
def test_threshold_schedule(K, scale, start):
    from pacingpseudo_amd.utils import gaussian_ramp_up, uncertainty_threshold as theta
    lnk = math.log(K)
    t0 = theta(0, start, K, scale)
    assert abs(t0 - (start + (1 - start) * gaussian_ramp_up(0, 1.0, scale=scale)) * lnk) < 1e-15
    assert start * lnk <= t0 <= (start + (1 - start) * math.exp(-scale)) * lnk + 1e-15      # s ln K up to the ramp's value at 0
    vals = [theta(e, start, K, scale) for e in range(0, 120)]
    assert all(b >= a for a, b in zip(vals, vals[1:])) and (start == 1.0 or vals[40] > vals[0])
    assert vals[80] == lnk and vals[-1] == lnk and max(vals) <= lnk
    for e in (0, 13, 79, 80, 400):
        assert abs(theta(e, start, K, scale) - R.threshold(e, start, K, scale)) < 1e-15
    with pytest.raises(ValueError):
        theta(0, start, 1, scale)
    with pytest.raises(ValueError):
        theta(0, 0.0, K, scale)


# ---------------------------------------------------------------- resume tables
def test_resume_tables_and_older_state_files():
    from pacingpseudo_amd import resume, train
    for k, v in DEFAULTS.items():
        assert resume.ABSENT_DEFAULTS[k] == v and k not in resume.MAY_DIFFER
        assert train.parser.get_default(k) == v
    new = resume.flag_dict(train.parse_args(['--tag', 'x']))
    old = {k: v for k, v in new.items() if k not in FLAGS}          # a state file written before the flags existed
    resume.check_compatible(old, new, 1, 1)
    resume.check_compatible(new, new, 1, 1)
    on = resume.flag_dict(train.parse_args(TEACHER + ['--cr_uncertainty', '4']))
    older_on = {k: v for k, v in on.items() if k not in FLAGS}
    with pytest.raises(resume.ResumeError, match='--cr_uncertainty '):
        resume.check_compatible(older_on, on, 1, 1)
    other = resume.flag_dict(train.parse_args(TEACHER + ['--cr_uncertainty', '2']))
    with pytest.raises(resume.ResumeError, match='--cr_uncertainty '):
        resume.check_compatible(on, other, 1, 1)
    sig = resume.flag_dict(train.parse_args(TEACHER + ['--cr_uncertainty', '4', '--cr_uncertainty_sigma', '0.3']))
    with pytest.raises(resume.ResumeError, match='--cr_uncertainty_sigma'):
        resume.check_compatible(on, sig, 1, 1)


# ---------------------------------------------------------------- output keys
def test_expected_keys_with_and_without_the_feature():
    from oracle import pacing_oracle as O
    from pacingpseudo_amd.models import ConsistencyRegulr
    args = O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    fake = SimpleNamespace(args=args, engine=SimpleNamespace(teacher=None, unc=None))
    keys = lambda: ConsistencyRegulr._expected_keys(fake, 'train')      # noqa: E731
    base = keys()
    assert 'segmentation/logits_teacher' not in base and 'segmentation/uncertainty_mask' not in base
    fake.engine.teacher = {1: None}
    with_teacher = keys()
    assert 'segmentation/uncertainty_mask' not in with_teacher
    fake.engine.unc = dict(passes=2)
    on = keys()
    i = on.index('segmentation/logits_teacher')
    assert on[i + 1] == 'segmentation/uncertainty_mask' and [k for k in on if k != 'segmentation/uncertainty_mask'] == with_teacher
    assert 'segmentation/uncertainty_mask' not in ConsistencyRegulr._expected_keys(fake, 'val')
    fake.engine.teacher = None           # a mask without a teacher cannot be: no key either
    assert keys() == base


def test_set_uncertainty_needs_a_teacher():
    from pacingpseudo_amd.engine import StepEngine
    eng = SimpleNamespace(teacher=None, unc='x')
    StepEngine.set_uncertainty(eng, None)
    assert eng.unc is None
    with pytest.raises(ValueError, match='attach_teacher'):
        StepEngine.set_uncertainty(eng, 2)


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_unc.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(punc_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _lib, _unc
    decls = _header_decls()
    assert list(decls) == list(_unc.EXPORTED_SYMBOLS) == list(_unc._PROTOS)
    for name, (_, argtypes) in _unc._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'unc', 'pp_uncertainty.hip')).read()
    assert int(re.search(r'#define PUNC_VERSION (\d+)', src).group(1)) == _unc.MIN_UNC_VERSION == 100
    defined = re.findall(r'extern "C"[^\n(]*?\b(punc_\w+)\s*\(', src)
    assert sorted(defined) == sorted(decls)
    assert 'asm' not in re.sub(r'//.*', '', src) and 'getenv' not in src
    assert len(_lib.EXPORTED_SYMBOLS) == 254          # the per-step library is as it was
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('punc_')]
    if os.path.exists(_unc.UNC_LIB_PATH):
        import ctypes
        dll = ctypes.CDLL(_unc.UNC_LIB_PATH)
        for name in decls:
            assert hasattr(dll, name), name
        out = subprocess.run(['nm', '-D', '--defined-only', _unc.UNC_LIB_PATH], capture_output=True, text=True)
        if out.returncode == 0:
            exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('punc_'))
            assert exported == sorted(decls)


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _unc
    from pacingpseudo_amd._lib import HipLibraryError
    if not os.path.exists(_unc.UNC_LIB_PATH):
        pytest.skip('libpacingpseudo_unc.so is not built')
    lib = _unc._UncLib()
    assert lib.punc_version() >= _unc.MIN_UNC_VERSION
    assert lib.punc_workspace_bytes(2, 5, 300) == 3 * 3 * 8 and lib.punc_workspace_bytes(1, 1, 64) == 0
    assert lib.punc_workspace_bytes(1, 33, 64) == 0
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.punc_noise_add(None, 4, 0.1, 0.2, None, 0, None, None)
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.punc_advance(None, None)
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.punc_accumulate(None, 1, 5, 64, 0, 1, None, 1.0, None, None, None, None, None, 0, None)


def test_missing_or_stale_library_raises(tmp_path):
    from pacingpseudo_amd import _unc
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing'):
        _unc._UncLib(str(tmp_path / 'nope.so')).punc_version()
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler for the stale-library stand-ins')
    for tag, body, msg in (('old', 'int punc_version(void) { return 99; }', 'punc_version\\(\\) = 99'),
                           ('part', 'int punc_version(void) { return 100; } const char* punc_last_error(void) { return ""; }', 'lacks 4 entry')):
        c = tmp_path / f'{tag}.c'
        c.write_text(body)
        so = tmp_path / f'lib{tag}.so'
        subprocess.run([cc, '-shared', '-fPIC', str(c), '-o', str(so)], check=True)
        with pytest.raises(HipLibraryError, match=msg):
            _unc._UncLib(str(so)).load()


def test_the_binding_is_not_loaded_at_import():
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.engine, pacingpseudo_amd.train, sys\n'
            'from pacingpseudo_amd import _unc\n'
            'assert _unc.unc._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_unc_host_side_under_address_sanitizer():
    """`make asan-unc` instruments the host half of pp_uncertainty.hip and runs tests/native/asan_unc_args.cpp, a program of its own
    that feeds every punc_* entry point the arguments it must refuse before any launch."""
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-unc'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
