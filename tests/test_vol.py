"""Volume-wise evaluation (inference.py --volumes; libpacingpseudo_vol.so), the parts that need no GPU: the scipy reference of
tests/_vol_reference.py against the 2-D references on a single slice, group_volumes, the parser's cross-flag errors, every refusal
of the Python functions and of the library, header / binding / library agreeing symbol for symbol, the synthetic volumes, and the
host half of the library under AddressSanitizer."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _cc_reference as C2  # noqa: E402
from tests import _surface_reference as S2  # noqa: E402
from tests import _vol_reference as V  # noqa: E402


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('connectivity', [1, 2])
def test_reference_on_one_slice_is_the_2d_component_reference(connectivity):
    rng = np.random.RandomState(3)
    for cm in (rng.randint(0, 3, size=(23, 41)), C2.serpentine(17, 20), C2.comb(9, 14)):
        vol = cm[None]
        assert np.array_equal(V.canonical_labels(vol, connectivity)[0], C2.canonical_labels(cm, connectivity))
        assert np.array_equal(V.canonical_labels(cm, connectivity), C2.flood_fill_labels(cm, connectivity))
        out3, stats3 = V.keep_largest(vol, 3, connectivity)
        out2, stats2 = C2.keep_largest(cm, 3, connectivity)
        assert np.array_equal(out3[0], out2) and np.array_equal(stats3[:, 0], stats2[:, 0])
        for k in range(1, 3):                                            # 3-D: voxels removed; 2-D: pixels kept
            assert stats3[k, 1] + stats2[k, 1] == int((cm == k).sum())


def test_reference_connectivities_in_3d():
    cm = np.zeros((3, 3, 3), np.int64)
    cm[0, 0, 0] = cm[1, 1, 0] = cm[2, 2, 1] = 1                          # an edge contact, then a corner contact
    assert [len(np.unique(V.canonical_labels(cm, c)[cm == 1])) for c in (1, 2, 3)] == [3, 2, 1]
    assert V.canonical_labels(cm, 3)[2, 2, 1] == 0
    m = V.serpentine_3d(7, 9, 11)
    assert (V.canonical_labels(m, 1)[m == 1] == 0).all() and m[0, 0, 0] == 1
    cut = m.copy()
    cut[1::2] = 0                                                        # without the bridges: one component per filled slice
    assert len(np.unique(V.canonical_labels(cut, 1)[cut == 1])) == 4 and m[1::2].sum() == 3
    out, stats = V.keep_largest(np.array([[[1, 0, 1, 1, 0, 1, 1]]]), 2, 1)           # sizes 1, 2, 2: the first of the two largest
    assert out.ravel().tolist() == [0, 0, 1, 1, 0, 0, 0] and stats[1].tolist() == [3, 3]


@pytest.mark.parametrize('spacing', [(1.0, 1.0), (1.51, 1.51), (0.7, 2.3)])
def test_reference_on_one_slice_is_the_2d_surface_reference(spacing):
    pred, label = S2.seeded_maps((37, 53))
    for p, t in zip(pred, label):                                        # a slice handed over as a plane: the cross is the 2-D one
        got = V.surface_metrics(p, t, 5, spacing, check_tolerance=False)
        ref = S2.surface_metrics(p, t, 5, spacing, check_tolerance=False)
        for key in V.KEYS:
            assert np.array_equal(got[key], ref[key], equal_nan=True), key
        for c in range(5):
            a, b = p == c, t == c
            if S2.is_scored(a, b):
                for x, y in zip(V.directed_sets(a, b, spacing), S2.directed_sets(a, b, spacing)):
                    assert np.array_equal(x, y)
    # as a volume of one slice every voxel has a neighbour outside the volume: the surface is the mask itself
    a = pred[0][None] == 1
    sa, _ = V.surfaces(a, a)
    assert np.array_equal(sa, a)


def test_reference_edt_and_dice():
    m = np.ones((3, 4, 5), np.uint8)
    assert np.isinf(V.edt(m)).all() and (V.edt_squared_int(m) == -1).all()
    m[2, 3, 0] = 0
    assert V.edt_squared_int(m)[0, 0, 4] == 4 + 9 + 16 and V.edt(m, (2.0, 1.0, 0.5))[0, 0, 4] == math.sqrt(16 + 9 + 4)
    d = V.dice(np.array([0, 1, 1, 3]), np.array([0, 1, 2, 3]), 5)
    assert d[:4].tolist() == [1.0, 2 / 3, 0.0, 1.0] and np.isnan(d[4])


# ---------------------------------------------------------------- group_volumes
def test_group_volumes_on_good_names():
    from pacingpseudo_amd.utils import group_volumes
    names = ['vol001_slice002', 'vol000_slice001', 'vol001_slice001', 'vol000_slice000', 'vol001_slice003']
    g = group_volumes(names)
    assert list(g.items()) == [('vol001', [2, 0, 4]), ('vol000', [3, 1])]            # first appearance; slices by number
    assert list(group_volumes(['patient007_frame01_3', 'patient007_frame01_4', 'patient007_frame12_0']).items()) == [
        ('patient007_frame01', [0, 1]), ('patient007_frame12', [2])]
    assert list(group_volumes(['a-9', 'a-10', 'a-11', 'bslice1', 'b_slice2', 'c7']).items()) == [('a', [0, 1, 2]), ('b', [3, 4]), ('c', [5])]
    assert list(group_volumes(['s10_p3', 's9_p3', 's11_p4'], r's(?P<slice>\d+)_(?P<volume>p\d+)').items()) == [('p3', [1, 0]), ('p4', [2])]
    assert len(group_volumes([])) == 0


def test_group_volumes_refuses_bad_names():
    from pacingpseudo_amd.utils import group_volumes
    with pytest.raises(ValueError, match="'noslice' does not match"):
        group_volumes(['v_1', 'noslice'])
    with pytest.raises(ValueError, match="'v_01' repeats slice 1 of volume 'v'"):
        group_volumes(['v_1', 'v_2', 'v_01'])
    with pytest.raises(ValueError, match="'v_5'.*no slice 4"):
        group_volumes(['v_2', 'v_3', 'v_5', 'w_0'])
    with pytest.raises(ValueError, match='named groups'):
        group_volumes(['v_1'], r'(.*)_(\d+)')
    with pytest.raises(ValueError, match='not a regular expression'):
        group_volumes(['v_1'], r'(?P<volume>.*')
    with pytest.raises(ValueError, match='is not a number'):
        group_volumes(['v_x'], r'(?P<volume>.*)_(?P<slice>.*)')


# ---------------------------------------------------------------- the parser
BASE = ['--fold', '0', '--checkpoint_file', 'runs/fold0']


@pytest.mark.parametrize('argv, message', [
    (['--volumes'], '--slice_spacing MM on real data'),
    (['--volumes', '--slice_spacing', '0'], 'millimetres, > 0'),
    (['--volumes', '--slice_spacing', 'nan'], 'millimetres, > 0'),
    (['--volumes', '--synthetic', '8'], 'needs --synthetic_depth'),
    (['--volumes', '--synthetic', '9', '--synthetic_depth', '4'], 'not a multiple'),
    (['--synthetic', '9', '--synthetic_depth', '4'], 'not a multiple'),
    (['--synthetic_depth', '4'], 'pass --synthetic as well'),
    (['--synthetic', '8', '--synthetic_depth', '-4'], '>= 1'),
    (['--slice_spacing', '5'], 'belongs to --volumes'),
    (['--volume_regex', 'x'], 'belongs to --volumes'),
    (['--cc_connectivity_3d', '2'], 'belongs to --volumes'),
    (['--volumes', '--slice_spacing', '5', '--cc_connectivity_3d', '4'], 'invalid choice'),
    (['--volumes', '--slice_spacing', '5', '--volume_regex', '(?P<volume>.*)'], 'named groups'),
    (['--volumes', '--slice_spacing', '5', '--volume_regex', '(abc'], 'not a regular expression'),
])
def test_cross_flag_errors_exit_with_status_2(argv, message, capsys):
    from pacingpseudo_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.parse_args(BASE + argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_parser_flags_and_defaults():
    from pacingpseudo_amd import inference
    a = inference.parse_args(BASE)
    assert (a.volumes, a.volume_regex, a.slice_spacing, a.cc_connectivity_3d, a.synthetic_depth) == (False, None, None, 1, 0)
    assert set(inference.VOLUME_FLAGS) == {'volumes', 'volume_regex', 'slice_spacing', 'cc_connectivity_3d', 'synthetic_depth'}
    a = inference.parse_args(BASE + ['--volumes', '--slice_spacing', '5.5', '--cc_connectivity_3d', '3'])
    assert a.volumes and a.slice_spacing == 5.5 and a.cc_connectivity_3d == 3
    a = inference.parse_args(BASE + ['--volumes', '--synthetic', '8', '--synthetic_depth', '4'])
    assert a.slice_spacing is None                                       # the in-plane spacing is taken where the data set is known
    from pacingpseudo_amd import train, upper_bound                     # the training drivers stay per slice
    for p in (train.parser, upper_bound.parser):
        assert not [x.dest for x in p._actions if x.dest in inference.VOLUME_FLAGS]


# ---------------------------------------------------------------- the synthetic volumes
def test_synthetic_volumes_stack_to_ellipsoids():
    from pacingpseudo_amd.data import SyntheticPhantoms, SyntheticVolumes
    from pacingpseudo_amd.utils import group_volumes
    ds = SyntheticVolumes(12, 5, depth=6, size=32, seed=1)
    assert len(ds) == 12 and ds.names[7] == 'vol001_slice001'
    assert list(group_volumes(ds.names).items()) == [('vol000', list(range(6))), ('vol001', list(range(6, 12)))]
    labs = np.stack([ds.raw_arrays(i)[1] for i in range(12)]).reshape(2, 6, 32, 32)
    assert np.array_equal(labs[0], np.stack([SyntheticVolumes(12, 5, depth=6, size=32, seed=1).raw_arrays(i)[1] for i in range(6)]))
    assert not np.array_equal(labs[0], labs[1])
    for v in range(2):
        present = [k for k in range(1, 5) if (labs[v] == k).any()]
        assert len(present) >= 3
        for k in present:                                                # an ellipsoid (less what later ones cover) is one 26-component at most twice cut
            area = (labs[v] == k).sum((1, 2))
            assert area.max() > 0 and len(np.unique(V.canonical_labels(labs[v], 3)[labs[v] == k])) <= 2
    item = ds[3]
    assert item['image'].shape == (1, 32, 32) and item['label_idx'].dtype == torch.uint8
    with pytest.raises(ValueError, match='multiple of depth'):
        SyntheticVolumes(10, 5, depth=4)
    # SyntheticPhantoms is what it was: its slices do not depend on this class
    a = SyntheticPhantoms(2, 5, size=32, train=False, seed=1, native=True, compact=True).raw_arrays(1)[1]
    assert a.shape == (32, 32) and not np.array_equal(a, ds.raw_arrays(1)[1])


# ---------------------------------------------------------------- the Python functions refuse before the library
def test_utilities_refuse_before_the_library():
    from pacingpseudo_amd.utils import (distance_transform_edt_3d, keep_largest_components_3d, label_components_3d, volume_dice,
                                        volume_surface_metrics)
    cpu = torch.zeros((2, 4, 4), dtype=torch.int64)
    for f in (lambda: label_components_3d(cpu), lambda: keep_largest_components_3d(cpu, 3), lambda: distance_transform_edt_3d(cpu),
              lambda: volume_surface_metrics(cpu, cpu, 3, (1, 1, 1)), lambda: volume_dice(cpu, cpu, 3)):
        with pytest.raises(ValueError, match='CUDA tensor'):
            f()
    with pytest.raises(ValueError, match=r'one \(D, H, W\) volume'):
        label_components_3d(torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='must be one of'):
        label_components_3d(torch.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match='empty axis'):
        label_components_3d(torch.zeros((0, 4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match='D <= 4096'):
        label_components_3d(torch.zeros((4097, 1, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match='H, W <= 2048'):
        distance_transform_edt_3d(torch.zeros((1, 1, 2049), dtype=torch.uint8))
    for c in (0, 4, True, 1.0):
        with pytest.raises(ValueError, match='connectivity must be'):
            label_components_3d(cpu, c)
    for k in (0, 33, True, 2.0):
        with pytest.raises(ValueError, match='num_classes must be'):
            keep_largest_components_3d(cpu, k)
    for sp in ((1, 1), (1, 0, 1), (1, math.inf, 1), 'abc', 1.0):
        with pytest.raises(ValueError, match='spacing must be'):
            distance_transform_edt_3d(cpu, sp)
    with pytest.raises(ValueError, match='squared must be'):
        distance_transform_edt_3d(cpu, squared=2)
    with pytest.raises(ValueError, match='tolerance'):
        volume_surface_metrics(cpu, cpu, 3, (1, 1, 1), tolerance=-1.0)
    with pytest.raises(ValueError, match='percentile'):
        volume_surface_metrics(cpu, cpu, 3, (1, 1, 1), percentile=0.0)


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_vol.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(pvol_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


SYMBOLS = ['pvol_version', 'pvol_last_error', 'pvol_label_workspace', 'pvol_keep_largest_workspace', 'pvol_edt_workspace',
           'pvol_surface_workspace', 'pvol_label_components', 'pvol_keep_largest_components', 'pvol_edt', 'pvol_surface_distances',
           'pvol_dice_counts']


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _lib, _vol
    decls = _header_decls()
    assert list(decls) == SYMBOLS == list(_vol.EXPORTED_SYMBOLS) == list(_vol._PROTOS)
    for name, (_, argtypes) in _vol._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'vol', 'pp_volume.hip')).read()
    assert int(re.search(r'#define PVOL_VERSION (\d+)', src).group(1)) == _vol.MIN_VOL_VERSION == 100
    assert tuple(int(re.search(rf'#define PVOL_B{a} (\d+)', src).group(1)) for a in 'DHW') == _vol.BRICK
    defined = re.findall(r'extern "C"[^\n(]*?\b(pvol_\w+)\s*\(', src)
    assert sorted(defined) == sorted(decls)
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src and '#include "pp_' not in src          # self-contained
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicAdd', 'atomicMax'}              # on int / unsigned long long only:
    assert not re.search(r'atomic\w+\s*\(\s*&?\s*\(?\s*(float|double)', code) and 'unsafeAtomicAdd' not in code
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMalloc' not in code and 'hipMemcpy' not in code
    assert 'fp contract(off)' in src
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('pvol_')]          # the per-step library is as it was
    assert os.path.exists(_vol.VOL_LIB_PATH), 'libpacingpseudo_vol.so is not built (make vol)'
    import ctypes
    dll = ctypes.CDLL(_vol.VOL_LIB_PATH)
    for name in decls:
        assert hasattr(dll, name), name
    out = subprocess.run(['nm', '-D', '--defined-only', _vol.VOL_LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('pvol_'))
        assert exported == sorted(decls)


def test_build_targets_are_wired():
    from tests._wiring import wired
    wired('vol', 'pacingpseudo_amd/csrc/vol/pp_volume.hip')


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _vol
    from pacingpseudo_amd._lib import HipLibraryError
    lib = _vol._VolLib()
    assert lib.pvol_version() >= _vol.MIN_VOL_VERSION
    n = 3 * 5 * 7
    pad8 = lambda b: (b + 7) // 8 * 8  # noqa: E731
    assert lib.pvol_label_workspace(3, 5, 7) == pad8(4 * n) and lib.pvol_edt_workspace(3, 5, 7) == pad8(2 * n)
    assert lib.pvol_keep_largest_workspace(5, 3, 5, 7) == 80 + 3 * pad8(4 * n)
    assert lib.pvol_surface_workspace(5, 3, 5, 7) == pad8(4 * n) + pad8(2 * n) + 2 * pad8(n) + 24
    assert lib.pvol_surface_workspace(4, 2, 64, 33) == 8 * 4224 + 48                       # two blocks of 4096 voxels
    assert lib.pvol_label_workspace(0, 5, 7) == 0 and lib.pvol_label_workspace(4097, 5, 7) == 0 and lib.pvol_edt_workspace(3, 2049, 7) == 0
    assert lib.pvol_label_workspace(512, 2048, 2048) == 0 and lib.pvol_keep_largest_workspace(33, 3, 5, 7) == 0
    assert lib.pvol_surface_workspace(32, 8, 2048, 2048) == 0 and lib.pvol_surface_workspace(0, 3, 5, 7) == 0
    big = 1 << 20
    nan, inf = math.nan, math.inf
    calls = {
        'null pointer': [lambda: lib.pvol_label_components(None, 3, 5, 7, 1, None, None, 0, None),
                         lambda: lib.pvol_keep_largest_components(256, 5, 3, 5, 7, 1, None, 256, 256, big, None),
                         lambda: lib.pvol_edt(256, 3, 5, 7, 1.0, 1.0, 1.0, 0, 256, None, big, None),
                         lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 7, 1.0, 1.0, 1.0, 256, None, 256, big, None),
                         lambda: lib.pvol_dice_counts(256, None, 5, 3, 5, 7, 256, None)],
        'aligned': [lambda: lib.pvol_label_components(260, 3, 5, 7, 1, 256, 256, big, None),
                    lambda: lib.pvol_label_components(256, 3, 5, 7, 1, 258, 256, big, None),
                    lambda: lib.pvol_label_components(256, 3, 5, 7, 1, 256, 260, big, None),
                    lambda: lib.pvol_keep_largest_components(256, 5, 3, 5, 7, 1, 260, 256, 256, big, None),
                    lambda: lib.pvol_keep_largest_components(256, 5, 3, 5, 7, 1, 256, 257, 256, big, None),
                    lambda: lib.pvol_edt(256, 3, 5, 7, 1.0, 1.0, 1.0, 0, 258, 256, big, None),
                    lambda: lib.pvol_edt(257, 3, 5, 7, 1.0, 1.0, 1.0, 0, 256, 260, big, None),
                    lambda: lib.pvol_surface_distances(256, 260, 5, 3, 5, 7, 1.0, 1.0, 1.0, 256, 256, 256, big, None),
                    lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 7, 1.0, 1.0, 1.0, 257, 256, 256, big, None),
                    lambda: lib.pvol_dice_counts(256, 256, 5, 3, 5, 7, 258, None)],
        'need 1 <= D': [lambda: lib.pvol_label_components(256, 0, 5, 7, 1, 256, 256, big, None),
                        lambda: lib.pvol_edt(256, 4097, 5, 7, 1.0, 1.0, 1.0, 0, 256, 256, big, None),
                        lambda: lib.pvol_dice_counts(256, 256, 5, -1, 5, 7, 256, None)],
        'need 1 <= H, W': [lambda: lib.pvol_keep_largest_components(256, 5, 3, 0, 7, 1, 256, 256, 256, big, None),
                           lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 2049, 1.0, 1.0, 1.0, 256, 256, 256, big, None)],
        '2\\^31 voxels': [lambda: lib.pvol_label_components(256, 512, 2048, 2048, 1, 256, 256, big, None)],
        '2\\^31 distances': [lambda: lib.pvol_surface_distances(256, 256, 32, 8, 2048, 2048, 1.0, 1.0, 1.0, 256, 256, 256, big, None)],
        'need 1 <= K': [lambda: lib.pvol_keep_largest_components(256, 0, 3, 5, 7, 1, 256, 256, 256, big, None),
                        lambda: lib.pvol_surface_distances(256, 256, 33, 3, 5, 7, 1.0, 1.0, 1.0, 256, 256, 256, big, None),
                        lambda: lib.pvol_dice_counts(256, 256, 33, 3, 5, 7, 256, None)],
        'connectivity': [lambda: lib.pvol_label_components(256, 3, 5, 7, 0, 256, 256, big, None),
                         lambda: lib.pvol_keep_largest_components(256, 5, 3, 5, 7, 4, 256, 256, 256, big, None)],
        'spacing': [lambda: lib.pvol_edt(256, 3, 5, 7, 0.0, 1.0, 1.0, 0, 256, 256, big, None),
                    lambda: lib.pvol_edt(256, 3, 5, 7, 1.0, nan, 1.0, 0, 256, 256, big, None),
                    lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 7, 1.0, 1.0, inf, 256, 256, 256, big, None),
                    lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 7, -1.0, 1.0, 1.0, 256, 256, 256, big, None)],
        'squared': [lambda: lib.pvol_edt(256, 3, 5, 7, 1.0, 1.0, 1.0, 2, 256, 256, big, None)],
        'workspace of': [lambda: lib.pvol_label_components(256, 3, 5, 7, 1, 256, 256, pad8(4 * n) - 1, None),
                         lambda: lib.pvol_keep_largest_components(256, 5, 3, 5, 7, 1, 256, 256, 256, 80 + 3 * pad8(4 * n) - 1, None),
                         lambda: lib.pvol_edt(256, 3, 5, 7, 1.0, 1.0, 1.0, 0, 256, 256, pad8(2 * n) - 1, None),
                         lambda: lib.pvol_surface_distances(256, 256, 5, 3, 5, 7, 1.0, 1.0, 1.0, 256, 256, 256, 0, None)],
    }
    for msg, fs in calls.items():
        for f in fs:
            with pytest.raises(HipLibraryError, match=r'rc=-1\).*' + msg):
                f()


def test_missing_library_raises_and_the_binding_is_not_loaded_at_import(tmp_path):
    from pacingpseudo_amd import _vol
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing.*make vol'):
        _vol._VolLib(str(tmp_path / 'nope.so')).pvol_version()
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.utils.volume, pacingpseudo_amd.inference, sys\n'
            'from pacingpseudo_amd import _vol\n'
            'assert _vol.vol._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_vol_host_side_under_address_sanitizer():
    """`make asan-vol` instruments the host half of pp_volume.hip and runs tests/native/asan_vol_args.cpp, a program of its own that
    feeds every pvol_* entry point the arguments it must refuse before any launch.  Nothing is loaded into Python."""
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-vol'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
