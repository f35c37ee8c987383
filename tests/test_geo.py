"""Geodesic scribbles (train_chaos.py --geo_scribbles; libpacingpseudo_geo.so), the parts that need no GPU: the float32 Dijkstra
reference against whole-plane sweep relaxation bit for bit, every refusal of the Python functions, the parser's flags, the resume
tables, header / binding / library agreeing symbol for symbol, and the host half of the library under AddressSanitizer."""
import math
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

from tests import _geo_reference as R  # noqa: E402

FLAGS = ('geo_scribbles', 'geo_lambda', 'geo_ratio', 'geo_max_dist', 'geo_max_sweeps')
DEFAULTS = dict(geo_scribbles=False, geo_lambda=20.0, geo_ratio=0.25, geo_max_dist=math.inf, geo_max_sweeps=100000)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('shape', [(1, 40), (40, 1), (37, 70)])
def test_reference_dijkstra_equals_sweep_relaxation_bitwise(shape):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    g = rng.randn(*shape).astype(np.float32)
    seeds = np.zeros(shape, dtype=bool)
    seeds.flat[rng.choice(g.size, 2, replace=False)] = True
    ref = R.dijkstra(g, seeds, 3.0)
    assert np.isfinite(ref).all() and (ref[seeds] == 0).all() and (ref[~seeds] >= 1).all()
    for order in (R.NEIGHBOURS, R.NEIGHBOURS[::-1]):
        got, sweeps = R.sweep_relaxation(g, seeds, 3.0, order)
        assert sweeps >= 1 and np.array_equal(_bits(got), _bits(ref)), (shape, sweeps)


def test_reference_spiral_needs_many_sweeps_and_still_agrees():
    g, seeds = R.spiral_maze(67, 100.0)
    ref = R.dijkstra(g, seeds, 5.0)
    got, sweeps = R.sweep_relaxation(g, seeds, 5.0)
    assert np.array_equal(_bits(got), _bits(ref)) and sweeps > 20 and ref.max() > 3 * (67 + 67)


def test_reference_without_an_image_is_the_chamfer_distance():
    h, w, sy, sx = 40, 50, 13, 21
    seeds = np.zeros((h, w), dtype=bool)
    seeds[sy, sx] = True
    d = R.dijkstra(np.zeros((h, w), np.float32), seeds, 0.0)
    dy, dx = np.abs(np.arange(h) - sy)[:, None], np.abs(np.arange(w) - sx)[None, :]
    want = np.maximum(dy, dx) + (math.sqrt(2.0) - 1.0) * np.minimum(dy, dx)
    assert np.abs(d - want).max() < 1e-4


def test_reference_walls_seedless_classes_and_labels():
    g = np.zeros((9, 9), np.float32)
    g[4] = np.nan
    scb = np.full((9, 9), 3)
    scb[1, 1], scb[2, 7] = 0, 1
    d = R.distances(g, scb, 3, 2.0)
    assert np.isinf(d[:, 4:]).all() and np.isfinite(d[:2, :4]).all() and np.isinf(d[2]).all()
    lab = R.labels(d, scb, 3, ratio=1.0)
    assert (lab[4:] == 3).all() and (lab[:4] < 2).all() and lab[1, 1] == 0 and lab[2, 7] == 1
    near = R.labels(d, scb, 3, ratio=1.0, max_dist=1.0)
    assert (near != 3).sum() == 2 + 4 + 4          # the seeds and their axis neighbours; the diagonal ones lie at 1.414 > 1
    tie = np.zeros((1, 5), np.float32)
    s2 = np.array([[0, 2, 2, 2, 1]])
    dt = R.distances(tie, s2, 2, 0.0)
    assert R.labels(dt, s2, 2, ratio=1.0).tolist() == [[0, 0, 0, 1, 1]]          # the tie in the middle goes to the first class
    assert R.labels(dt, s2, 2, ratio=0.25).tolist() == [[0, 2, 2, 2, 1]]


# ---------------------------------------------------------------- argument checks, before the library
def _lib_untouched():
    from pacingpseudo_amd import _geo
    return _geo.geo._dll is None


def test_check_geo_params():
    from pacingpseudo_amd.utils import check_geo_params as chk
    assert chk() == dict(lam=20.0, ratio=0.25, max_dist=math.inf, max_sweeps=100000)
    assert chk(0, 1, 3, 1, K=32) == dict(lam=0.0, ratio=1.0, max_dist=3.0, max_sweeps=1)
    for kw in (dict(lam=-1.0), dict(lam=math.nan), dict(lam=math.inf), dict(lam=True), dict(ratio=0.0), dict(ratio=1.01),
               dict(ratio=math.nan), dict(ratio=-0.5), dict(max_dist=0.0), dict(max_dist=-math.inf), dict(max_dist=math.nan),
               dict(max_sweeps=0), dict(max_sweeps=-3), dict(max_sweeps=2.5), dict(max_sweeps=True), dict(max_sweeps=math.inf),
               dict(K=0), dict(K=2.5), dict(K=True), dict(K=-1)):
        with pytest.raises(ValueError):
            chk(**kw)
    for kw in (dict(max_sweeps=2 ** 31), dict(K=33)):
        with pytest.raises(NotImplementedError):
            chk(**kw)


def test_utilities_refuse_before_the_library():
    from pacingpseudo_amd.utils import geodesic_distance as gd, geodesic_expand_scribbles as ge
    was = _lib_untouched()
    img, scb = torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    bad = [lambda: gd(img, scb, 3), lambda: ge(img, scb, 3),                                   # CPU tensors
           lambda: gd(np.zeros((2, 4, 5), np.float32), scb, 3), lambda: ge(img, None, 3),
           lambda: gd(img, scb, 3, lam=-1.0), lambda: gd(img, scb, 3, max_sweeps=0), lambda: gd(img, scb, 3, lam=math.nan),
           lambda: ge(img, scb, 3, ratio=0.0), lambda: ge(img, scb, 3, ratio=2.0), lambda: ge(img, scb, 3, max_dist=0.0),
           lambda: ge(img, scb, 3, max_sweeps=2 ** 31), lambda: ge(img, scb, 3, lam=math.inf)]
    for i, f in enumerate(bad):
        with pytest.raises((TypeError, ValueError, NotImplementedError)):
            f()
            pytest.fail(f'case {i} was not refused')
    assert _lib_untouched() == was


# ---------------------------------------------------------------- parser and resume tables
def test_parser_flags_and_defaults():
    from pacingpseudo_amd import train
    a = train.parse_args(['--tag', 'x'])
    assert {k: getattr(a, k) for k in FLAGS} == DEFAULTS
    a = train.parse_args(['--tag', 'x', '--geo_scribbles', '--geo_lambda', '5', '--geo_ratio', '0.5', '--geo_max_dist', '30',
                          '--geo_max_sweeps', '7'])
    assert (a.geo_scribbles, a.geo_lambda, a.geo_ratio, a.geo_max_dist, a.geo_max_sweeps) == (True, 5.0, 0.5, 30.0, 7)
    helps = {act.dest: act.help for act in train.parser._actions}
    assert all('untuned first value' in helps[k] for k in ('geo_lambda', 'geo_ratio', 'geo_max_dist'))
    for argv in (['--geo_scribbles', '--rw_scribbles'], ['--geo_lambda', '-1'], ['--geo_lambda', 'nan'], ['--geo_ratio', '0'],
                 ['--geo_ratio', '1.5'], ['--geo_max_dist', '0'], ['--geo_max_sweeps', '0'], ['--geo_max_sweeps', '2147483648']):
        with pytest.raises(SystemExit) as e:
            train.parse_args(['--tag', 'x'] + argv)
        assert e.value.code == 2, argv


def test_the_supervised_driver_has_none_of_the_flags():
    from pacingpseudo_amd import upper_bound
    assert not [a.dest for a in upper_bound.parser._actions if a.dest.startswith('geo')]


def test_resume_tables_and_older_state_files():
    from pacingpseudo_amd import resume, train
    for k, v in DEFAULTS.items():
        assert resume.ABSENT_DEFAULTS[k] == v and type(resume.ABSENT_DEFAULTS[k]) is type(v) and k not in resume.MAY_DIFFER
        assert train.parser.get_default(k) == v
    new = resume.flag_dict(train.parse_args(['--tag', 'x']))
    old = {k: v for k, v in new.items() if k not in FLAGS}          # a state file written before the flags existed
    resume.check_compatible(old, new, 1, 1)
    on = resume.flag_dict(train.parse_args(['--tag', 'x', '--geo_scribbles']))
    with pytest.raises(resume.ResumeError, match='--geo_scribbles'):
        resume.check_compatible(old, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--geo_scribbles'):
        resume.check_compatible(on, new, 1, 1)
    lam = resume.flag_dict(train.parse_args(['--tag', 'x', '--geo_scribbles', '--geo_lambda', '5']))
    with pytest.raises(resume.ResumeError, match='--geo_lambda'):
        resume.check_compatible(on, lam, 1, 1)


def test_tool_parser_keeps_rw_as_the_default_method():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_expand_scribbles_tool', os.path.join(ROOT, 'scripts', 'expand_scribbles.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.build_parser().parse_args(['--synthetic', '2', '--out', 'x'])
    assert a.method == 'rw' and a.rw_beta == 13.0 and a.geo_lambda == 20.0
    assert tool.build_parser().parse_args(['--synthetic', '2', '--out', 'x', '--method', 'geo']).method == 'geo'
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(['--synthetic', '2', '--out', 'x', '--method', 'edt'])


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_geo.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(pgeo_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _geo, _lib
    decls = _header_decls()
    assert len(decls) == 6
    assert list(decls) == list(_geo.EXPORTED_SYMBOLS) == list(_geo._PROTOS)
    for name, (_, argtypes) in _geo._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'geo', 'pp_geodesic.hip')).read()
    assert int(re.search(r'#define PGEO_VERSION (\d+)', src).group(1)) == _geo.MIN_GEO_VERSION == 100
    defined = re.findall(r'extern "C"[^\n(]*?\b(pgeo_\w+)\s*\(', src)
    assert sorted(defined) == sorted(decls)
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src and '#include "pp_' not in src          # self-contained
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicMin', 'atomicOr'}          # integer minimum / or in LDS, nothing else
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMalloc' not in code and 'hipMemcpy' not in code
    assert 'fp contract(off)' in src
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('pgeo_')]          # the per-step library is as it was
    if os.path.exists(_geo.GEO_LIB_PATH):
        import ctypes
        dll = ctypes.CDLL(_geo.GEO_LIB_PATH)
        for name in decls:
            assert hasattr(dll, name), name
        out = subprocess.run(['nm', '-D', '--defined-only', _geo.GEO_LIB_PATH], capture_output=True, text=True)
        if out.returncode == 0:
            exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('pgeo_'))
            assert exported == sorted(decls)


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _geo
    from pacingpseudo_amd._lib import HipLibraryError
    if not os.path.exists(_geo.GEO_LIB_PATH):
        pytest.skip('libpacingpseudo_geo.so is not built')
    lib = _geo._GeoLib()
    assert lib.pgeo_version() >= _geo.MIN_GEO_VERSION
    assert lib.pgeo_distance_workspace(1, 1, 8, 8) == 8 and lib.pgeo_distance_workspace(2, 5, 65, 129) == 64
    assert lib.pgeo_distance_workspace(1, 33, 8, 8) == 0 and lib.pgeo_distance_workspace(1, 5, 1025, 8) == 0
    assert lib.pgeo_distance_workspace(64, 32, 1024, 1024) == 0 and lib.pgeo_distance_workspace(0, 5, 8, 8) == 0
    import ctypes
    inf = math.inf
    bad_sizes = (ctypes.c_int * 2)(9, 8)
    calls = {
        'null pointer': [lambda: lib.pgeo_normalize(None, None, 1, 8, 8, None, None),
                         lambda: lib.pgeo_distance(None, None, None, 1, 5, 8, 8, 20.0, 100, None, None, None, 0, None),
                         lambda: lib.pgeo_labels(None, None, None, 1, 5, 8, 8, inf, 0.25, None, None)],
        'aligned': [lambda: lib.pgeo_normalize(258, None, 1, 8, 8, 256, None),
                    lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, 20.0, 100, 256, 256, 260, 64, None),
                    lambda: lib.pgeo_labels(256, 256, None, 1, 5, 8, 8, inf, 0.25, 257, None)],
        'need N >= 1': [lambda: lib.pgeo_normalize(256, None, 0, 8, 8, 256, None)],
        'need 1 <= K': [lambda: lib.pgeo_distance(256, 256, None, 1, 33, 8, 8, 20.0, 100, 256, 256, 256, 64, None),
                        lambda: lib.pgeo_labels(256, 256, None, 1, 0, 8, 8, inf, 0.25, 256, None)],
        'need 1 <= H, W': [lambda: lib.pgeo_normalize(256, None, 1, 1025, 8, 256, None),
                           lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 0, 20.0, 100, 256, 256, 256, 64, None)],
        '2\\^31': [lambda: lib.pgeo_distance(256, 256, None, 64, 32, 1024, 1024, 20.0, 100, 256, 256, 256, 1 << 20, None)],
        'does not lie inside': [lambda: lib.pgeo_normalize(256, bad_sizes, 1, 8, 8, 256, None),
                                lambda: lib.pgeo_labels(256, 256, bad_sizes, 1, 5, 8, 8, inf, 0.25, 256, None)],
        'lam': [lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, -1.0, 100, 256, 256, 256, 64, None),
                lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, math.nan, 100, 256, 256, 256, 64, None),
                lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, inf, 100, 256, 256, 256, 64, None)],
        'max_sweeps': [lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, 20.0, 0, 256, 256, 256, 64, None)],
        'workspace of': [lambda: lib.pgeo_distance(256, 256, None, 1, 5, 8, 8, 20.0, 100, 256, 256, 256, 7, None)],
        'max_dist': [lambda: lib.pgeo_labels(256, 256, None, 1, 5, 8, 8, 0.0, 0.25, 256, None),
                     lambda: lib.pgeo_labels(256, 256, None, 1, 5, 8, 8, math.nan, 0.25, 256, None)],
        'ratio': [lambda: lib.pgeo_labels(256, 256, None, 1, 5, 8, 8, inf, 0.0, 256, None),
                  lambda: lib.pgeo_labels(256, 256, None, 1, 5, 8, 8, inf, 1.5, 256, None)],
    }
    for msg, fs in calls.items():
        for f in fs:
            with pytest.raises(HipLibraryError, match=r'rc=-1\).*' + msg):
                f()


def test_missing_or_stale_library_raises(tmp_path):
    from pacingpseudo_amd import _geo
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing.*make geo'):
        _geo._GeoLib(str(tmp_path / 'nope.so')).pgeo_version()
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler for the stale-library stand-ins')
    for tag, body, msg in (('old', 'int pgeo_version(void) { return 99; }', 'pgeo_version\\(\\) = 99.*make geo'),
                           ('part', 'int pgeo_version(void) { return 100; } const char* pgeo_last_error(void) { return ""; }',
                            'lacks 4 entry.*make geo')):
        c = tmp_path / f'{tag}.c'
        c.write_text(body)
        so = tmp_path / f'lib{tag}.so'
        subprocess.run([cc, '-shared', '-fPIC', str(c), '-o', str(so)], check=True)
        with pytest.raises(HipLibraryError, match=msg):
            _geo._GeoLib(str(so)).load()


def test_the_binding_is_not_loaded_at_import():
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.utils.geodesic, pacingpseudo_amd.train, sys\n'
            'from pacingpseudo_amd import _geo\n'
            'assert _geo.geo._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_geo_host_side_under_address_sanitizer():
    """`make asan-geo` instruments the host half of pp_geodesic.hip and runs tests/native/asan_geo_args.cpp, a program of its own
    that feeds every pgeo_* entry point the arguments it must refuse before any launch.  Nothing is loaded into Python."""
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-geo'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
