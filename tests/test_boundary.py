"""Boundary loss (upper_bound_chaos.py --do_loss_boundary; libpacingpseudo_dist.so), the parts that need no GPU: the float64 / scipy
reference against a brute-force nearest-pixel search, every ValueError path of the three Python functions, the parser's flags, the
resume tables, and header / binding / library agreeing symbol for symbol."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _boundary_reference as R  # noqa: E402

FLAGS = ('do_loss_boundary', 'loss_boundary_weight', 'ramp_up_loss_boundary')
DEFAULTS = dict(do_loss_boundary=False, loss_boundary_weight=0.01, ramp_up_loss_boundary=0)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('shape,spacing', [((17, 23), (1.0, 1.0)), ((33, 9), (1.5, 0.75)), ((1, 40), (1.0, 1.0)), ((40, 1), (2.0, 1.0))])
def test_reference_edt_against_brute_force(shape, spacing):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    for frac in (0.5, 0.9):
        m = rng.rand(*shape) < frac
        m.flat[rng.randint(m.size)] = False
        assert np.abs(R.edt(m, spacing) - R.brute_edt(m, spacing)).max() == 0.0
    if spacing == (1.0, 1.0):
        assert np.array_equal(R.edt_squared_int(m), np.rint(R.brute_edt(m) ** 2).astype(np.int64))


def test_reference_deviations_and_one_hot2dist():
    full = np.ones((2, 4, 5), dtype=bool)
    full[1, 2, 3] = False
    d = R.edt(full)
    assert np.isinf(d[0]).all() and d[1, 2, 3] == 0.0 and d[1, 2, 4] == 1.0 and np.array_equal(R.edt_squared_int(full)[0], -np.ones((4, 5)))
    cm = np.zeros((2, 6, 7), dtype=np.int64)
    cm[0, 2:4, 2:5] = 1
    cm[0, 0, 0] = 3                                     # K = 3: outside every class
    phi = R.signed_maps(cm, 3)
    assert not phi[0, 2].any()                          # absent
    assert not phi[1].any()                             # image 1 is all class 0: class 0 whole (deviation 2), 1 and 2 absent
    pos = cm[0] == 1
    from scipy.ndimage import distance_transform_edt as sedt
    assert np.array_equal(phi[0, 1], sedt(~pos) * ~pos - (sedt(pos) - 1) * pos)          # Kervadec's one_hot2dist
    assert phi[0, 1][2, 2] == 0.0 and phi[0, 1][0, 0] > 0 and (phi[0, 1][pos] <= 0).all() and (phi[0, 1][~pos] > 0).all()
    assert phi[0, 0][0, 0] == 1.0                       # the ignored pixel is outside class 0
    aniso = R.signed_maps(cm, 3, (2.0, 0.5))
    assert aniso[0, 1][2, 2] == 0.0 and aniso[0, 1][2, 1] == 0.5 and aniso[0, 1][1, 2] == 2.0


def test_reference_loss_gradient_formula():
    g = torch.Generator().manual_seed(2)
    for K in (1, 2, 5):
        z = torch.randn(2, K, 3, 4, generator=g, dtype=torch.float64)
        phi = torch.randn(2, K, 3, 4, generator=g, dtype=torch.float64)
        val, grad = R.loss_and_grad(z, phi, 1.7)
        p = torch.softmax(z, 1)
        ind = torch.zeros(K, dtype=torch.float64)
        ind[R.foreground(K)] = 1.0
        m = ind.view(1, K, 1, 1) * phi
        want = 1.7 * p * (m - (p * m).sum(1, keepdim=True)) / (2 * len(R.foreground(K)) * 12)
        assert np.abs(grad - want.numpy()).max() < 1e-15 and abs(val - float((p * m).sum() / (2 * len(R.foreground(K)) * 12))) < 1e-15


# ---------------------------------------------------------------- argument checks, before the library
def _lib_untouched():
    from pacingpseudo_amd import _dist
    return _dist.dist._dll is None


def test_distance_functions_refuse_before_the_library():
    from pacingpseudo_amd.utils import distance_transform_edt as edt, signed_distance_maps as sdm
    was = _lib_untouched()
    m = torch.ones(4, 5, dtype=torch.uint8)
    c = torch.zeros(2, 4, 5, dtype=torch.int64)
    bad_edt = [lambda: edt(m),                                               # a CPU tensor
               lambda: edt(np.ones((4, 5))), lambda: edt(m.float()), lambda: edt(m[None, None]), lambda: edt(m[0]),
               lambda: edt(torch.ones(0, 5, dtype=torch.uint8)), lambda: edt(torch.ones(1, 2049, dtype=torch.uint8)),
               lambda: edt(torch.ones(2049, 1, dtype=torch.uint8)),
               lambda: edt(m, spacing=(1.0,)), lambda: edt(m, spacing=(0.0, 1.0)), lambda: edt(m, spacing=(1.0, -1.0)),
               lambda: edt(m, spacing=(float('nan'), 1.0)), lambda: edt(m, spacing=(1.0, float('inf'))), lambda: edt(m, spacing=2.0),
               lambda: edt(m, spacing=('a', 'b')), lambda: edt(m, squared=2), lambda: edt(m, squared='yes')]
    bad_sdm = [lambda: sdm(c, 5),                                            # a CPU tensor
               lambda: sdm(np.zeros((4, 5), dtype=np.int64), 5), lambda: sdm(c.float(), 5), lambda: sdm(c.bool(), 5),
               lambda: sdm(c[None], 5), lambda: sdm(c[0, 0], 5), lambda: sdm(torch.zeros(2, 0, 5, dtype=torch.int64), 5),
               lambda: sdm(torch.zeros(1, 1, 2049, dtype=torch.int64), 5),
               lambda: sdm(c, 0), lambda: sdm(c, 33), lambda: sdm(c, 5.0), lambda: sdm(c, True), lambda: sdm(c, -1),
               lambda: sdm(c, 5, spacing=(1.0, 0.0)), lambda: sdm(c, 5, spacing=(1.0, 1.0, 1.0)), lambda: sdm(c, 5, spacing=None)]
    for i, f in enumerate(bad_edt + bad_sdm):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f'case {i} was not refused')
    assert _lib_untouched() == was


def test_boundary_loss_refuses_before_the_library():
    from pacingpseudo_amd.losses.losses import boundary_loss as bl
    was = _lib_untouched()
    z = torch.zeros(2, 5, 4, 6)
    t1 = torch.zeros(2, 5, 4, 6)
    tc = torch.zeros(2, 4, 6, dtype=torch.int64)
    bad = [lambda: bl(z, t1), lambda: bl(z, tc), lambda: bl(z, t1, dist_maps=t1),            # CPU tensors
           lambda: bl(z.double(), t1), lambda: bl(z[0], t1), lambda: bl(np.zeros((2, 5, 4, 6), dtype=np.float32), t1),
           lambda: bl(torch.zeros(2, 33, 4, 6), tc), lambda: bl(torch.zeros(1, 2, 1, 2049), tc), lambda: bl(torch.zeros(0, 5, 4, 6), tc),
           lambda: bl(z, None), lambda: bl(z, np.zeros((2, 4, 6), dtype=np.int64)), lambda: bl(z, tc.int()), lambda: bl(z, tc[:1]),
           lambda: bl(z, t1[:, :4]), lambda: bl(z, tc[0]), lambda: bl(z, tc.float()),
           lambda: bl(z, tc, dist_maps=t1.double()), lambda: bl(z, tc, dist_maps=t1[:, :4]), lambda: bl(z, tc, dist_maps=np.zeros(3)),
           lambda: bl(z, tc, spacing=(0.0, 1.0)), lambda: bl(z, tc, spacing=(1.0,)), lambda: bl(z, tc, spacing=(1.0, float('nan')))]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f'case {i} was not refused')
    assert _lib_untouched() == was


# ---------------------------------------------------------------- parser and resume tables
def test_parser_flags_and_defaults():
    from pacingpseudo_amd import upper_bound
    a = upper_bound.parser.parse_args(['--tag', 'x'])
    assert {k: getattr(a, k) for k in FLAGS} == DEFAULTS
    a = upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_boundary', '--loss_boundary_weight', '0.05', '--ramp_up_loss_boundary', '40'])
    assert (a.do_loss_boundary, a.loss_boundary_weight, a.ramp_up_loss_boundary) == (True, 0.05, 40)
    helps = {act.dest: act.help for act in upper_bound.parser._actions}
    assert 'untuned first value' in helps['loss_boundary_weight'] and 'gaussian_ramp_up' in helps['ramp_up_loss_boundary']
    for argv in (['--ramp_up_loss_boundary', '-1'], ['--loss_boundary_weight', 'nan']):
        with pytest.raises(SystemExit) as e:
            upper_bound.train_main(['--tag', 'x', '--do_loss_boundary'] + argv)
        assert e.value.code == 2


def test_the_scribble_driver_has_none_of_the_flags():
    from pacingpseudo_amd import train
    assert not [a.dest for a in train.parser._actions if 'boundary' in a.dest]


def test_resume_tables_and_older_state_files():
    from pacingpseudo_amd import resume, upper_bound
    for k, v in DEFAULTS.items():
        assert resume.ABSENT_DEFAULTS[k] == v and type(resume.ABSENT_DEFAULTS[k]) is type(v) and k not in resume.MAY_DIFFER
        assert upper_bound.parser.get_default(k) == v
    new = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x']))
    old = {k: v for k, v in new.items() if k not in FLAGS}          # a state file written before the flags existed
    resume.check_compatible(old, new, 1, 1)
    on = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_boundary']))
    with pytest.raises(resume.ResumeError, match='--do_loss_boundary'):
        resume.check_compatible(old, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--do_loss_boundary'):
        resume.check_compatible(on, new, 1, 1)
    w = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_boundary', '--loss_boundary_weight', '0.1']))
    with pytest.raises(resume.ResumeError, match='--loss_boundary_weight'):
        resume.check_compatible(on, w, 1, 1)
    r = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_boundary', '--ramp_up_loss_boundary', '10']))
    with pytest.raises(resume.ResumeError, match='--ramp_up_loss_boundary'):
        resume.check_compatible(on, r, 1, 1)


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_dist.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(pdist_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _dist, _lib
    decls = _header_decls()
    assert len(decls) == 9
    assert list(decls) == list(_dist.EXPORTED_SYMBOLS) == list(_dist._PROTOS)
    for name, (_, argtypes) in _dist._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'distance', 'pp_distance.hip')).read()
    assert int(re.search(r'#define PDIST_VERSION (\d+)', src).group(1)) == _dist.MIN_DIST_VERSION == 100
    defined = re.findall(r'extern "C"[^\n(]*?\b(pdist_\w+)\s*\(', src)
    assert sorted(defined) == sorted(decls)
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src
    assert 'atomic' not in code.lower()                       # sums are fixed-order reductions
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMalloc' not in code
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('pdist_')]          # the per-step library is as it was
    if os.path.exists(_dist.DIST_LIB_PATH):
        import ctypes
        dll = ctypes.CDLL(_dist.DIST_LIB_PATH)
        for name in decls:
            assert hasattr(dll, name), name
        out = subprocess.run(['nm', '-D', '--defined-only', _dist.DIST_LIB_PATH], capture_output=True, text=True)
        if out.returncode == 0:
            exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('pdist_'))
            assert exported == sorted(decls)


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _dist
    from pacingpseudo_amd._lib import HipLibraryError
    if not os.path.exists(_dist.DIST_LIB_PATH):
        pytest.skip('libpacingpseudo_dist.so is not built')
    lib = _dist._DistLib()
    assert lib.pdist_version() >= _dist.MIN_DIST_VERSION
    assert lib.pdist_edt_workspace(3, 8, 8) == 384 and lib.pdist_edt_workspace(1, 2049, 8) == 0
    assert lib.pdist_signed_maps_workspace(2, 5, 3, 3) == 184 and lib.pdist_signed_maps_workspace(1, 33, 8, 8) == 0      # 180 -> 184
    assert lib.pdist_signed_maps_workspace(16, 32, 2048, 2048) == 0
    assert lib.pdist_boundary_loss_workspace(2, 5, 10, 30) == 3 * 8 and lib.pdist_boundary_loss_workspace(1, 0, 8, 8) == 0
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.pdist_edt(None, 1, 8, 8, 1.0, 1.0, 0, None, None, 0, None)
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.pdist_signed_maps(None, 1, 5, 8, 8, 1.0, 1.0, None, None, 0, None)
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.pdist_boundary_loss_fwd(None, None, 1, 5, 8, 8, None, None, 0, None)
    with pytest.raises(HipLibraryError, match='null pointer'):
        lib.pdist_boundary_loss_bwd(None, None, 1, 5, 8, 8, None, None, None)


def test_missing_or_stale_library_raises(tmp_path):
    from pacingpseudo_amd import _dist
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing.*make dist'):
        _dist._DistLib(str(tmp_path / 'nope.so')).pdist_version()
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler for the stale-library stand-ins')
    for tag, body, msg in (('old', 'int pdist_version(void) { return 99; }', 'pdist_version\\(\\) = 99'),
                           ('part', 'int pdist_version(void) { return 100; } const char* pdist_last_error(void) { return ""; }', 'lacks 7 entry')):
        c = tmp_path / f'{tag}.c'
        c.write_text(body)
        so = tmp_path / f'lib{tag}.so'
        subprocess.run([cc, '-shared', '-fPIC', str(c), '-o', str(so)], check=True)
        with pytest.raises(HipLibraryError, match=msg):
            _dist._DistLib(str(so)).load()


def test_the_binding_is_not_loaded_at_import():
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.losses.losses, pacingpseudo_amd.upper_bound, sys\n'
            'from pacingpseudo_amd import _dist\n'
            'assert _dist.dist._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_dist_host_side_under_address_sanitizer():
    """`make asan-dist` instruments the host half of pp_distance.hip and runs tests/native/asan_dist_args.cpp, a program of its own
    that feeds every pdist_* entry point the arguments it must refuse before any launch."""
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-dist'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
