"""The size threshold and hole filling (inference.py --min_component_size / --fill_holes; libpacingpseudo_morph.so), the parts that
need no GPU: the numpy / scipy restatement of tests/_morph_reference.py against scipy.ndimage.binary_fill_holes and against
hand-drawn cases, the parser, every refusal of the Python functions and of the library, header / binding / library agreeing symbol
for symbol, and the host half of the library under AddressSanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _morph_reference as M  # noqa: E402


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('shape', [(37, 53), (64, 64), (1, 130), (5, 19, 33), (9, 16, 70)])
def test_reference_with_two_classes_is_scipys_binary_fill_holes(shape):
    cavities = 0
    for seed, density in enumerate((0.35, 0.5, 0.65)):
        mask = np.random.RandomState(seed).rand(*shape) < density
        for ch in range(1, len(shape) + 1):
            out, stats = M.fill_holes(mask.astype(np.int64), 2, ch)
            want = ndimage.binary_fill_holes(mask, M.structure(len(shape), ch))
            assert np.array_equal(out.astype(bool), want), (density, ch)
            assert stats[0].tolist() == [0, 0] and stats[1, 1] == int(want.sum() - mask.sum())
            cavities += int(stats[1, 0])
    assert cavities > 0 or 1 in shape[:-1]                               # a single row has no interior


def test_reference_on_random_class_maps_takes_both_branches():
    for K in (5, 32):
        for shape in ((37, 53), (9, 16, 70)):
            _, stats = M.fill_holes(M.random_map(shape, K, 0), K, 1)
            assert stats[0, 0] > 0 and stats[1:, 0].sum() > 0 and stats[K - 1, 0] > 0, (K, shape)
            _, stats = M.remove_small(M.random_map(shape, K, 0), K, 4)
            assert stats[1:, 0].sum() > 0 and stats[0].tolist() == [0, 0]


@pytest.mark.parametrize('name', list(M.hand_drawn()))
def test_reference_on_hand_drawn_cavities(name):
    case = M.hand_drawn()[name]
    out, stats = M.fill_holes(case['cm'], case['K'], case['ch'])
    want = case['cm'].copy()
    for (y, x), k in case['filled'].items():
        want[y, x] = k
    assert np.array_equal(out, want)
    assert stats[0, 0] == case['mixed'] and stats[1:, 1].sum() == len(case['filled'])
    assert (out[case['cm'] != 0] == case['cm'][case['cm'] != 0]).all()   # nothing non-zero is overwritten


def test_reference_size_threshold_keeps_exactly_min_size():
    cm, want = M.size_case(5)
    out, stats = M.remove_small(cm, 3, 5)
    assert np.array_equal(out, want) and stats.tolist() == [[0, 0], [1, 4], [1, 4]]
    out, stats = M.remove_small(cm, 3, [0, 6, 1])                        # per class: 6 takes both of class 1, <= 1 leaves class 2
    assert not (out == 1).any() and np.array_equal(out == 2, cm == 2) and stats.tolist() == [[0, 0], [2, 9], [0, 0]]
    assert np.array_equal(M.remove_small(cm, 3, 0)[0], cm) and np.array_equal(M.remove_small(cm, 3, 1)[0], cm)
    diag = np.array([[1, 0], [0, 1]])                                    # two components of one pixel, or one of two
    assert M.remove_small(diag, 2, 2, 1)[0].sum() == 0 and M.remove_small(diag, 2, 2, 2)[0].sum() == 2
    cm9 = np.array([[9, 9, 0, 1]])
    assert np.array_equal(M.remove_small(cm9, 3, 5)[0], [[9, 9, 0, 0]])   # a value outside [0, K) is copied


def test_reference_chain_closes_the_cavity_a_removed_speck_leaves():
    cm = np.ones((7, 7), np.int64)
    cm[0] = cm[-1] = 0
    cm[3, 3] = 2                                                         # a speck of class 2 inside class 1
    assert np.array_equal(M.fill_holes(cm, 3, 1)[0], cm)
    out = M.chain(cm, 3, 2, 1, None, 1)
    assert out[3, 3] == 1 and (out[1:-1] == 1).all()


# ---------------------------------------------------------------- the parser
BASE = ['--fold', '0', '--checkpoint_file', 'runs/fold0']
VOL = ['--volumes', '--slice_spacing', '5']


@pytest.mark.parametrize('argv, message', [
    (['--min_component_size', '-1'], 'an integer >= 0'),
    (['--min_component_size', 'x'], 'invalid int value'),
    (['--min_component_size_3d', '10'], 'belongs to --volumes'),
    (['--fill_holes', '--fill_holes_connectivity_3d', '2'], 'belongs to --volumes'),
    (['--fill_holes_connectivity', '2'], 'belongs to --fill_holes'),
    (['--fill_holes', '--fill_holes_connectivity', '3'], 'invalid choice'),
    (VOL + ['--fill_holes_connectivity_3d', '3'], 'belongs to --fill_holes'),
    (VOL + ['--fill_holes', '--fill_holes_connectivity_3d', '4'], 'invalid choice'),
    (VOL + ['--min_component_size_3d', '-5'], 'an integer >= 0'),
])
def test_cross_flag_errors_exit_with_status_2(argv, message, capsys):
    from pacingpseudo_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.parse_args(BASE + argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_parser_flags_defaults_and_the_argument_dump():
    from pacingpseudo_amd import inference
    a = inference.parse_args(BASE)
    assert (a.min_component_size, a.fill_holes, a.fill_holes_connectivity, a.min_component_size_3d, a.fill_holes_connectivity_3d) == (0, False, 1, 0, 1)
    assert inference.MORPH_FLAGS == ('min_component_size', 'fill_holes', 'fill_holes_connectivity', 'min_component_size_3d',
                                     'fill_holes_connectivity_3d')
    assert not inference.morph_used(a)
    assert inference.morph_settings(a) == dict(min_component_size=0, fill_holes=False, fill_holes_connectivity=1, min_component_size_3d=0,
                                               fill_holes_connectivity_3d=1)
    a = inference.parse_args(BASE + ['--min_component_size', '20', '--fill_holes', '--fill_holes_connectivity', '2'])
    assert inference.morph_used(a) and inference.morph_settings(a)['min_component_size'] == 20 and a.fill_holes_connectivity == 2
    a = inference.parse_args(BASE + VOL + ['--fill_holes', '--min_component_size_3d', '50', '--fill_holes_connectivity_3d', '3'])
    assert inference.morph_used(a) and a.min_component_size_3d == 50 and a.fill_holes_connectivity_3d == 3
    # the dump of main(): a run without the flags does not name them
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'inference.py')).read()
    assert 'morph_used(args) or k not in MORPH_FLAGS' in src
    from pacingpseudo_amd import train, upper_bound                     # the training drivers have no such stage
    for p in (train.parser, upper_bound.parser):
        assert not [x.dest for x in p._actions if x.dest in inference.MORPH_FLAGS]


def test_evaluate_and_score_volumes_keep_their_signatures():
    import inspect
    from pacingpseudo_amd import inference
    ev = inspect.signature(inference.evaluate).parameters
    assert list(ev)[:13] == ['model', 'loader', 'num_classes', 'spacing', 'device', 'keep_largest_cc', 'cc_connectivity', 'tta', 'extra',
                             'surface_metrics', 'nsd_tolerance', 'crf', 'volume_maps']
    assert (ev['min_component_size'].default, ev['fill_holes'].default, ev['fill_holes_connectivity'].default) == (0, False, 1)
    sv = inspect.signature(inference.score_volumes).parameters
    assert list(sv)[:8] == ['volume_maps', 'groups', 'num_classes', 'spacing', 'keep_largest_cc', 'connectivity', 'surface_metrics', 'nsd_tolerance']
    assert (sv['min_component_size'].default, sv['fill_holes'].default, sv['fill_holes_connectivity'].default) == (0, False, 1)


# ---------------------------------------------------------------- the Python functions refuse before the library
def test_utilities_refuse_before_the_library():
    from pacingpseudo_amd.utils import (binary_fill_holes, check_morph_params, fill_holes, fill_holes_3d, remove_small_components,
                                        remove_small_components_3d)
    cpu = torch.zeros((2, 4, 4), dtype=torch.int64)
    for f in (lambda: remove_small_components(cpu, 3, 5), lambda: remove_small_components_3d(cpu, 3, 5), lambda: fill_holes(cpu, 3),
              lambda: fill_holes_3d(cpu, 3), lambda: binary_fill_holes(cpu != 0), lambda: binary_fill_holes(cpu[0] != 0)):
        with pytest.raises(ValueError, match='CUDA tensor'):
            f()
    for k in (0, 33, True, 2.0):
        for f in (remove_small_components, remove_small_components_3d):
            with pytest.raises(ValueError, match='num_classes must be'):
                f(cpu, k, 5)
        for f in (fill_holes, fill_holes_3d):
            with pytest.raises(ValueError, match='num_classes must be'):
                f(cpu, k)
    for bad in (-1, 2.0, True, [1, 2], [0, 1, -2], [0, 1, 2.5], 'abc', None, 2 ** 31):
        with pytest.raises(ValueError, match='min_size'):
            remove_small_components(cpu, 3, bad)
        with pytest.raises(ValueError, match='min_size'):
            remove_small_components_3d(cpu, 3, bad)
    for c in (0, 3, True, 1.0):
        with pytest.raises(ValueError, match='connectivity must be'):
            fill_holes(cpu, 3, c)
        with pytest.raises(ValueError, match='connectivity must be'):
            remove_small_components(cpu, 3, 5, c)
    for c in (0, 4, True, 1.0):
        with pytest.raises(ValueError, match='connectivity must be'):
            fill_holes_3d(cpu, 3, c)
        with pytest.raises(ValueError, match='connectivity must be'):
            remove_small_components_3d(cpu, 3, 5, c)
    with pytest.raises(ValueError, match='must hold integers'):
        fill_holes(torch.zeros((4, 4)), 3)
    with pytest.raises(ValueError, match=r'\(N, H, W\) or \(H, W\)'):
        fill_holes(torch.zeros((1, 2, 4, 4), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match=r'one \(D, H, W\) volume'):
        fill_holes_3d(torch.zeros((4, 4), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match='empty axis'):
        remove_small_components(torch.zeros((0, 4, 4), dtype=torch.int64), 3, 5)
    with pytest.raises(ValueError, match='bool tensor'):
        binary_fill_holes(cpu)
    with pytest.raises(ValueError, match=r'\(H, W\) or \(D, H, W\)'):
        binary_fill_holes(torch.zeros((4,), dtype=torch.bool))
    assert check_morph_params() == dict(min_component_size=0, fill_holes=False, fill_holes_connectivity=1, min_component_size_3d=0,
                                        fill_holes_connectivity_3d=1)
    assert check_morph_params(20, True, 2, 50, 3, volumes=True)['fill_holes_connectivity_3d'] == 3
    for kwargs, msg in ((dict(min_component_size=-1), '--min_component_size'), (dict(min_component_size=1.5), '--min_component_size'),
                        (dict(fill_holes=2), '--fill_holes'), (dict(fill_holes_connectivity=3), '--fill_holes_connectivity'),
                        (dict(fill_holes_connectivity_3d=4, volumes=True), '--fill_holes_connectivity_3d'),
                        (dict(min_component_size_3d=5), 'belongs to --volumes'), (dict(fill_holes_connectivity_3d=2), 'belongs to --volumes')):
        with pytest.raises(ValueError, match=msg):
            check_morph_params(**kwargs)


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_morph.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(pmor_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


SYMBOLS = ['pmor_version', 'pmor_last_error', 'pmor_workspace', 'pmor_remove_small', 'pmor_fill_holes']
ARGS = {'pmor_version': 0, 'pmor_last_error': 0, 'pmor_workspace': 6, 'pmor_remove_small': 14, 'pmor_fill_holes': 14}


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _dist, _geo, _lib, _morph, _vol
    decls = _header_decls()
    assert list(decls) == SYMBOLS == list(_morph.EXPORTED_SYMBOLS) == list(_morph._PROTOS)
    assert decls == ARGS
    for name, (_, argtypes) in _morph._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'morph', 'pp_morph.hip')).read()
    assert int(re.search(r'#define PMOR_VERSION (\d+)', src).group(1)) == _morph.MIN_MORPH_VERSION == 100
    defined = re.findall(r'extern "C"[^\n(]*?\b(pmor_\w+)\s*\(', src)
    assert sorted(defined) == sorted(decls)
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src and '#include "pp_' not in src          # self-contained
    assert set(re.findall(r'\b(?:atomic\w+|__hip_atomic_\w+)', code)) == {'__hip_atomic_fetch_add', '__hip_atomic_fetch_or', '__hip_atomic_load'}
    assert 'float' not in code and 'double' not in code                                      # integer work only
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMalloc' not in code and 'hipMemcpy' not in code
    for other in (_lib, _dist, _geo, _vol):                                                  # the other libraries are as they were
        assert not [s for s in other.EXPORTED_SYMBOLS if s.startswith('pmor_')]
    assert os.path.exists(_morph.MORPH_LIB_PATH), 'libpacingpseudo_morph.so is not built (make morph)'
    import ctypes
    dll = ctypes.CDLL(_morph.MORPH_LIB_PATH)
    for name in decls:
        assert hasattr(dll, name), name
    out = subprocess.run(['nm', '-D', '--defined-only', _morph.MORPH_LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('pmor_'))
        assert exported == sorted(decls)


def test_build_targets_are_wired():
    from tests._wiring import wired
    wired('morph', 'pacingpseudo_amd/csrc/morph/pp_morph.hip')


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    import ctypes
    from pacingpseudo_amd import _morph
    from pacingpseudo_amd._lib import HipLibraryError
    lib = _morph._MorphLib()
    assert lib.pmor_version() >= _morph.MIN_MORPH_VERSION
    pad8 = lambda b: (b + 7) // 8 * 8  # noqa: E731
    assert lib.pmor_workspace(3, 5, 1, 5, 7, 2) == pad8(4 * 105) and lib.pmor_workspace(1, 5, 3, 5, 7, 3) == pad8(4 * 105)
    assert lib.pmor_workspace(1, 1, 1, 1, 1, 2) == 8
    for bad in ((0, 5, 1, 5, 7, 2), (3, 0, 1, 5, 7, 2), (3, 33, 1, 5, 7, 2), (3, 5, 2, 5, 7, 2), (1, 5, 4097, 5, 7, 3), (3, 5, 1, 2049, 7, 2),
                (3, 5, 1, 5, 0, 2), (3, 5, 1, 5, 7, 1), (3, 5, 1, 5, 7, 4), (1, 5, 512, 2048, 2048, 3), (512, 5, 1, 2048, 2048, 2)):
        assert lib.pmor_workspace(*bad) == 0, bad
    big = 1 << 20
    thr = (ctypes.c_int32 * 5)(0, 5, 5, 5, 5)
    calls = {
        'null pointer': [lambda: lib.pmor_remove_small(None, 256, 3, 5, 1, 5, 7, 2, thr, 256, 256, 256, big, None),
                         lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 5, 7, 2, None, 256, 256, 256, big, None),
                         lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 5, 7, 2, thr, 256, None, 256, big, None),
                         lambda: lib.pmor_fill_holes(256, None, 3, 5, 1, 5, 7, 2, 1, 256, 256, 256, big, None),
                         lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 1, None, 256, 256, big, None),
                         lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 1, 256, 256, None, big, None)],
        'aligned': [lambda: lib.pmor_remove_small(260, 256, 3, 5, 1, 5, 7, 2, thr, 256, 256, 256, big, None),
                    lambda: lib.pmor_remove_small(256, 258, 3, 5, 1, 5, 7, 2, thr, 256, 256, 256, big, None),
                    lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 5, 7, 2, thr, 260, 256, 256, big, None),
                    lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 1, 256, 257, 256, big, None),
                    lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 1, 256, 256, 260, big, None)],
        'dims = ': [lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 5, 7, 1, thr, 256, 256, 256, big, None),
                    lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 4, 1, 256, 256, 256, big, None)],
        'at least one item': [lambda: lib.pmor_remove_small(256, 256, 0, 5, 1, 5, 7, 2, thr, 256, 256, 256, big, None)],
        'need 1 <= K': [lambda: lib.pmor_remove_small(256, 256, 3, 33, 1, 5, 7, 2, thr, 256, 256, 256, big, None),
                        lambda: lib.pmor_fill_holes(256, 256, 3, 0, 1, 5, 7, 2, 1, 256, 256, 256, big, None)],
        'need 1 <= D': [lambda: lib.pmor_fill_holes(256, 256, 1, 5, 4097, 5, 7, 3, 1, 256, 256, 256, big, None),
                        lambda: lib.pmor_remove_small(256, 256, 1, 5, 0, 5, 7, 3, thr, 256, 256, 256, big, None)],
        'a slice has D = 1': [lambda: lib.pmor_fill_holes(256, 256, 3, 5, 2, 5, 7, 2, 1, 256, 256, 256, big, None)],
        'need 1 <= H, W': [lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 0, 7, 2, thr, 256, 256, 256, big, None),
                           lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 2049, 2, 1, 256, 256, 256, big, None)],
        '2\\^31 voxels': [lambda: lib.pmor_fill_holes(256, 256, 1, 5, 512, 2048, 2048, 3, 1, 256, 256, 256, big, None),
                          lambda: lib.pmor_remove_small(256, 256, 512, 5, 1, 2048, 2048, 2, thr, 256, 256, 256, big, None)],
        'connectivity': [lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 0, 256, 256, 256, big, None),
                         lambda: lib.pmor_fill_holes(256, 256, 3, 5, 1, 5, 7, 2, 3, 256, 256, 256, big, None),
                         lambda: lib.pmor_fill_holes(256, 256, 1, 5, 3, 5, 7, 3, 4, 256, 256, 256, big, None)],
        'workspace of': [lambda: lib.pmor_remove_small(256, 256, 3, 5, 1, 5, 7, 2, thr, 256, 256, 256, pad8(4 * 105) - 1, None),
                         lambda: lib.pmor_fill_holes(256, 256, 1, 5, 3, 5, 7, 3, 1, 256, 256, 256, 0, None)],
    }
    for msg, fs in calls.items():
        for f in fs:
            with pytest.raises(HipLibraryError, match=r'rc=-1\).*' + msg):
                f()


def test_missing_library_raises_and_the_binding_is_not_loaded_at_import(tmp_path):
    from pacingpseudo_amd import _morph
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing.*make morph'):
        _morph._MorphLib(str(tmp_path / 'nope.so')).pmor_version()
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.utils.morphology, pacingpseudo_amd.inference, sys\n'
            'from pacingpseudo_amd import _morph, _vol\n'
            'assert _morph.morph._dll is None and _vol.vol._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_morph_host_side_under_address_sanitizer():
    """`make asan-morph` instruments the host half of pp_morph.hip and runs tests/native/asan_morph_args.cpp, a program of its own
    that feeds every pmor_* entry point the arguments it must refuse before any launch.  Nothing is loaded into Python."""
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-morph'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
