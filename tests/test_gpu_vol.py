"""Volume-wise evaluation on the device (libpacingpseudo_vol.so): 3-D component labels and the keep-largest filter against
scipy (exact), the 3-D EDT against scipy (exact squared field at unit spacing, 1 ulp for the root, 2^-21 relative for anisotropic
spacing), the surface-distance sets and the four surface metrics against medpy's definition restated in tests/_vol_reference.py
(rtol 1e-6), every output and workspace of the raw entry points between sentinel bands, and ``inference.py --volumes``.

Bounds.  Unit spacing: every candidate (g sz)^2 + (dy sy)^2 + (dx sx)^2 is an integer below 2^24, so the squared field is exact and
the distance is one correctly rounded fp32 root away from it: 1 ulp.  Anisotropic spacing: the fp32 chain is three rounded
products, their squares, two sums and one root: about 3 * 2^-24 relative for the root and 5 * 2^-24 for the square; REL = 2^-21
(2 REL for the square) leaves the margin tests/test_gpu_boundary.py leaves in 2-D, and the minimum over candidates cannot err by
more than its candidates do."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _vol_reference as V  # noqa: E402
from tests._guard import PATTERNS, BandSet  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 2.0 ** -21
RTOL = 1e-6


def dev():
    return torch.device('cuda', 0)


def _stream():
    from pacingpseudo_amd._lib import stream_ptr
    return stream_ptr()


def _ulp_ok(got32, ref64):
    """|got - ref| <= one fp32 ulp of the reference's magnitude (0 must be met exactly, +inf by +inf)."""
    got = np.asarray(got32, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    inf = np.isinf(ref)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    ok = np.where(inf, got == ref, np.abs(got - np.where(inf, 0.0, ref)) <= np.where(inf, 0.0, ulp))
    return bool(ok.all())


# ---------------------------------------------------------------- the raw entry points between sentinel bands
def _raw_labels(cm, connectivity, pattern=0xFF):
    from pacingpseudo_amd._vol import vol
    D, H, W = cm.shape
    bs = BandSet(pattern, dev())
    x = bs.tensor(torch.from_numpy(np.array(cm, np.int64)).to(dev()), label='cls')
    out = bs.banded((D, H, W), torch.int32, label='labels')
    ws = bs.ws(vol.pvol_label_workspace(D, H, W), label='workspace')
    vol.pvol_label_components(x.data_ptr(), D, H, W, connectivity, out.ptr(), ws.ptr(), ws.n, _stream())
    assert bs.damaged() == []
    return out.t.cpu().numpy()


def _raw_keep(cm, K, connectivity, pattern=0xFF):
    from pacingpseudo_amd._vol import vol
    D, H, W = cm.shape
    bs = BandSet(pattern, dev())
    x = bs.tensor(torch.from_numpy(np.array(cm, np.int64)).to(dev()), label='cls')
    out = bs.banded((D, H, W), torch.int64, label='out')
    stats = bs.banded((K, 2), torch.int32, label='stats')
    ws = bs.ws(vol.pvol_keep_largest_workspace(K, D, H, W), label='workspace')
    vol.pvol_keep_largest_components(x.data_ptr(), K, D, H, W, connectivity, out.ptr(), stats.ptr(), ws.ptr(), ws.n, _stream())
    assert bs.damaged() == []
    return out.t.cpu().numpy(), stats.t.cpu().numpy()


def _raw_edt(mask, spacing=(1., 1., 1.), squared=False, pattern=0xFF):
    from pacingpseudo_amd._vol import vol
    D, H, W = mask.shape
    bs = BandSet(pattern, dev())
    m = bs.tensor(torch.from_numpy(np.ascontiguousarray(mask != 0).astype(np.uint8)).to(dev()), label='mask')
    out = bs.banded((D, H, W), torch.float32, label='out')
    ws = bs.ws(vol.pvol_edt_workspace(D, H, W), label='workspace')
    vol.pvol_edt(m.data_ptr(), D, H, W, *[float(s) for s in spacing], int(squared), out.ptr(), ws.ptr(), ws.n, _stream())
    assert bs.damaged() == []
    return out.t.cpu().numpy()


def _raw_surface(pred, label, K, spacing, pattern=0xFF):
    """-> (dist (K, 2, n) fp32, counts (K, 4)) as numpy."""
    from pacingpseudo_amd._vol import vol
    D, H, W = pred.shape
    bs = BandSet(pattern, dev())
    p = bs.tensor(torch.from_numpy(np.array(pred, np.int64)).to(dev()), label='pred')
    t = bs.tensor(torch.from_numpy(np.array(label, np.int64)).to(dev()), label='label')
    dist = bs.banded((K, 2, D * H * W), torch.float32, label='dist')
    counts = bs.banded((K, 4), torch.int32, label='counts')
    ws = bs.ws(vol.pvol_surface_workspace(K, D, H, W), label='workspace')
    vol.pvol_surface_distances(p.data_ptr(), t.data_ptr(), K, D, H, W, *[float(s) for s in spacing], dist.ptr(), counts.ptr(), ws.ptr(),
                               ws.n, _stream())
    assert bs.damaged() == []
    return dist.t.cpu().numpy(), counts.t.cpu().numpy()


# ---------------------------------------------------------------- labels
def _label_cases():
    from pacingpseudo_amd._vol import BRICK
    rng = np.random.RandomState(7)
    cases = {}
    cases['1x1x1'] = np.array([[[3]]], np.int64)
    cases['2x1x1'] = np.array([[[1]], [[1]]], np.int64)
    cases['1x33x65'] = rng.randint(0, 3, size=(1, 33, 65)).astype(np.int64)
    cases['5x33x65'] = (rng.rand(5, 33, 65) < 0.55).astype(np.int64)          # no multiple of a brick edge; near the percolation threshold
    cases['brick depth + 1'] = (rng.rand(BRICK[0] + 1, BRICK[1] + 1, BRICK[2] + 1) < 0.6).astype(np.int64)
    zz, yy, xx = np.indices((6, 18, 34))
    cases['checkerboard'] = ((zz + yy + xx) % 2).astype(np.int64)
    cases['serpentine'] = V.serpentine_3d(9, 35, 67)
    touch = np.zeros((6, 20, 40), np.int64)                                      # pairs of solids around the brick corner (4, 16, 32):
    touch[0:2, 12:16, 28:32] = 1
    touch[0:2, 16:19, 32:36] = 1                                                 # class 1 touches along an edge, across two brick faces
    touch[0:2, 2:5, 2:5] = 2
    touch[2:5, 5:9, 5:9] = 2                                                     # class 2 touches at a corner only, inside one brick
    touch[2:4, 13:16, 29:32] = 3
    touch[4:6, 16:18, 32:35] = 3                                                 # class 3 touches at the brick corner itself
    cases['edge and corner'] = touch
    cases['noise 9x70x70'] = rng.randint(0, 5, size=(9, 70, 70)).astype(np.int64)
    for v in cases.values():
        v.setflags(write=False)
    return cases


_LABELS = {}


def _label_case(name, connectivity):
    """(class map, reference labels); made once and never modified."""
    if not _LABELS:
        for k, cm in _label_cases().items():
            for c in (1, 2, 3):
                ref = V.canonical_labels(cm, c)
                ref.setflags(write=False)
                _LABELS[k, c] = (cm, ref)
    return _LABELS[name, connectivity]


@pytest.mark.parametrize('connectivity', [1, 2, 3])
@pytest.mark.parametrize('name', ['1x1x1', '2x1x1', '1x33x65', '5x33x65', 'brick depth + 1', 'checkerboard', 'serpentine', 'edge and corner',
                                  'noise 9x70x70'])
def test_labels_equal_scipy(name, connectivity):
    cm, ref = _label_case(name, connectivity)
    got = _raw_labels(cm, connectivity)
    bad = int((got != ref).sum())
    print(f'labels {name} connectivity {connectivity}: {cm.shape}, {len(np.unique(ref))} components, {bad} labels differ')
    assert got.dtype == np.int32 and got.shape == cm.shape
    assert bad == 0
    if name == 'checkerboard':
        n = len(np.unique(ref))
        assert n == cm.size if connectivity == 1 else n == 2               # singletons; one component per parity class
    if name == 'serpentine':
        assert (ref[cm == 1] == 0).all()
    if name == 'edge and corner':
        n = tuple(len(np.unique(ref[cm == k])) for k in (1, 2, 3))
        assert n == {1: (2, 2, 2), 2: (1, 2, 2), 3: (1, 1, 1)}[connectivity]


@pytest.mark.parametrize('connectivity', [1, 2])
def test_labels_of_one_slice_equal_the_2d_labels(connectivity):
    from pacingpseudo_amd.utils import label_components, label_components_3d
    cm, _ = _label_case('1x33x65', connectivity)
    x = torch.from_numpy(cm.copy()).to(dev())
    assert torch.equal(label_components_3d(x, connectivity), label_components(x, connectivity))


@pytest.mark.parametrize('connectivity', [1, 3])
def test_labels_do_not_depend_on_the_workspace(connectivity):
    cm, ref = _label_case('noise 9x70x70', connectivity)
    a, b = (_raw_labels(cm, connectivity, pattern) for pattern in PATTERNS)
    assert np.array_equal(a, b) and np.array_equal(a, ref)
    ka, kb = (_raw_keep(cm, 5, connectivity, pattern) for pattern in PATTERNS)
    assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[1], kb[1])


# ---------------------------------------------------------------- keep largest
def _keep_cases():
    rng = np.random.RandomState(9)
    cases = {}
    ties = np.zeros((5, 20, 36), np.int64)
    ties[0:2, 1:3, 1:3] = 1
    ties[3:5, 10:12, 30:32] = 1                                                  # two components of 8 voxels: the first stays
    ties[1, 8, 8] = 1
    ties[0:3, 15:18, 20:23] = 2
    ties[4, 0, 0] = 2
    ties[2, 2, 30] = 7                                                           # a value >= K passes through
    ties[2, 3, 30] = -1
    cases['ties'] = (ties, 4)                                                    # class 3 is absent
    cases['k1'] = ((rng.rand(3, 9, 11) < 0.3).astype(np.int64), 1)
    cases['k32'] = (rng.randint(0, 34, size=(5, 18, 34)).astype(np.int64), 32)
    cases['blobs'] = (V.blobs_3d(6, 40, 48, 5, 3), 5)
    for cm, _ in cases.values():
        cm.setflags(write=False)
    return cases


@pytest.mark.parametrize('connectivity', [1, 2, 3])
@pytest.mark.parametrize('name', ['ties', 'k1', 'k32', 'blobs'])
def test_keep_largest_equals_scipy(name, connectivity):
    cm, K = _keep_cases()[name]
    ref, ref_stats = V.keep_largest(cm, K, connectivity)
    got, stats = _raw_keep(cm, K, connectivity)
    print(f'keep largest {name} connectivity {connectivity}: {int((cm != ref).sum())} voxels removed, stats {ref_stats[1:4].tolist()}')
    assert np.array_equal(got, ref)
    assert np.array_equal(stats, ref_stats)
    if name == 'ties':
        assert (got[0:2, 1:3, 1:3] == 1).all() and not (got[3:5, 10:12, 30:32] == 1).any()
        assert got[2, 2, 30] == 7 and got[2, 3, 30] == -1 and stats[3].tolist() == [0, 0]
    if name == 'k1':
        assert np.array_equal(got, cm) and stats.tolist() == [[0, 0]]


def test_keep_largest_3d_against_the_2d_filter_of_the_same_slices():
    """A class whose two blobs of one slice join through the next slice keeps both in 3-D (the 2-D filter removes one); an island
    that is the only blob of its class in its slice goes in 3-D and stays in 2-D."""
    from pacingpseudo_amd.utils import keep_largest_components, keep_largest_components_3d
    cm = np.zeros((4, 24, 40), np.int64)
    cm[0, 4:9, 4:9] = 1
    cm[0, 4:8, 20:24] = 1                                # slice 0: a fork, two cross-sections ...
    cm[1, 4:9, 4:24] = 1                                 # ... of one organ: joined in slice 1
    cm[3, 18:20, 30:33] = 1                              # an island, alone in slice 3
    x = torch.from_numpy(cm).to(dev())
    got3, stats = keep_largest_components_3d(x, 2, 1, return_stats=True)
    got2 = keep_largest_components(x, 2, 1)
    got3, got2 = got3.cpu().numpy(), got2.cpu().numpy()
    ref3, ref_stats = V.keep_largest(cm, 2, 1)
    assert np.array_equal(got3, ref3) and np.array_equal(stats.cpu().numpy(), ref_stats)
    assert (got3[0, 4:9, 4:9] == 1).all() and (got3[0, 4:8, 20:24] == 1).all()          # 3-D keeps both cross-sections
    assert (got2[0, 4:9, 4:9] == 1).all() and not got2[0, 4:8, 20:24].any()             # 2-D removes the smaller one
    assert not got3[3].any() and (got2[3, 18:20, 30:33] == 1).all()                     # the island: gone in 3-D, kept in 2-D
    assert stats.cpu().numpy()[1].tolist() == [2, 6]


# ---------------------------------------------------------------- EDT
def _edt_cases():
    rng = np.random.RandomState(11)
    cases = {}
    corner = np.ones((5, 20, 36), np.uint8)
    corner[4, 19, 0] = 0
    cases['corner'] = corner
    cases['ones'] = np.ones((3, 5, 7), np.uint8)
    cases['1x33x65'] = (rng.rand(1, 33, 65) < 0.9).astype(np.uint8)
    cases['7x33x9'] = (rng.rand(7, 33, 9) < 0.95).astype(np.uint8)
    for i, p in enumerate((0.6, 0.9, 0.995)):
        cases[f'3x67x129 density {p}'] = (np.random.RandomState(20 + i).rand(3, 67, 129) < p).astype(np.uint8)
    for v in cases.values():
        v.setflags(write=False)
    return cases


EDT_NAMES = ['corner', 'ones', '1x33x65', '7x33x9', '3x67x129 density 0.6', '3x67x129 density 0.9', '3x67x129 density 0.995']


@pytest.mark.parametrize('name', EDT_NAMES)
def test_edt_unit_spacing_against_scipy(name):
    mask = _edt_cases()[name]
    ref2 = V.edt_squared_int(mask)
    none = ref2 < 0
    want2 = np.where(none, np.inf, ref2.astype(np.float64))
    sq = _raw_edt(mask, squared=True)
    d = _raw_edt(mask, pattern=PATTERNS[1])
    bad = int((sq.astype(np.float64) != want2).sum())
    print(f'edt {name}: {mask.shape}, {bad} squared distances differ from scipy, max {np.where(none, 0, ref2).max()}')
    assert sq.dtype == np.float32 and sq.shape == mask.shape
    assert bad == 0                                                   # bit for bit: integers
    assert _ulp_ok(d, np.sqrt(want2).astype(np.float32).astype(np.float64))
    assert (d[mask == 0] == 0).all() and (sq[mask == 0] == 0).all()
    if name == 'ones':
        assert np.isinf(d).all() and np.isinf(sq).all()
    if name == 'corner':
        assert sq[0, 0, 35] == 4 * 4 + 19 * 19 + 35 * 35
    if name == '1x33x65':                                             # one slice: the 2-D transform, bit for bit
        from pacingpseudo_amd.utils import distance_transform_edt, distance_transform_edt_3d
        m = torch.from_numpy(mask.copy()).to(dev())
        assert torch.equal(distance_transform_edt_3d(m)[0], distance_transform_edt(m[0]))
        assert np.array_equal(distance_transform_edt_3d(m).cpu().numpy(), d)


@pytest.mark.parametrize('name', ['7x33x9', '3x67x129 density 0.6', '3x67x129 density 0.9', '3x67x129 density 0.995'])
def test_edt_anisotropic_spacing_against_float64(name):
    mask = _edt_cases()[name]
    spacing = (5.0, 1.5, 0.75)
    ref = V.edt(mask, spacing)
    assert np.isfinite(ref).all()
    got = _raw_edt(mask, spacing).astype(np.float64)
    got2 = _raw_edt(mask, spacing, squared=True).astype(np.float64)
    err = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    err2 = np.abs(got2 - ref * ref) / np.where(ref > 0, ref * ref, 1.0)
    print(f'edt {spacing} {name}: max relative error {err.max():.3e} (bound {REL:.3e}), squared {err2.max():.3e} (bound {2 * REL:.3e})')
    assert (np.abs(got - ref) <= REL * ref).all()
    assert (np.abs(got2 - ref * ref) <= 2 * REL * ref * ref).all()


# ---------------------------------------------------------------- surfaces
SURFACE_SPACINGS = ((1.0, 1.0, 1.0), (5.0, 1.62, 1.62))
_SURF = {}


def _surface_case():
    """(pred, label, K, {spacing: ([(d1, d2) per class], metrics)}); made once and never modified."""
    if not _SURF:
        K = 4
        label = V.blobs_3d(6, 40, 48, K, 21)
        pred = label.copy()
        rng = np.random.RandomState(22)
        hit = rng.rand(*label.shape) < 0.08
        pred[hit] = rng.randint(0, K, int(hit.sum()))
        pred[1:3] = np.roll(pred[1:3], 2, axis=2)
        pred.setflags(write=False)
        label.setflags(write=False)
        refs = {}
        for sp in SURFACE_SPACINGS:
            sets = [V.directed_sets(pred == c, label == c, sp) for c in range(K)]
            refs[sp] = (sets, V.surface_metrics(pred, label, K, sp, tolerance=2.0, check_tolerance=True))
        _SURF['case'] = (pred, label, K, refs)
    return _SURF['case']


@pytest.mark.parametrize('spacing', SURFACE_SPACINGS)
def test_surface_sets_and_metrics_against_the_reference(spacing):
    from pacingpseudo_amd.utils import volume_surface_metrics
    pred, label, K, refs = _surface_case()
    sets, ref = refs[spacing]
    for key in V.KEYS:                                                # every item is scored in the reference: nothing is skipped below
        assert np.isfinite(ref[key]).all(), (key, ref[key])
    dist, counts = _raw_surface(pred, label, K, spacing)
    worst = 0.0
    for c in range(K):
        d1, d2 = sets[c]
        assert counts[c].tolist() == [d1.size, d2.size, int((pred == c).sum()), int((label == c).sum())]
        for got, want in ((dist[c, 0, :d1.size], d1), (dist[c, 1, :d2.size], d2)):      # linear-index order: element by element
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-30) * (want > 0))))
            assert np.allclose(got, want, rtol=RTOL, atol=0.0)
    got = volume_surface_metrics(torch.from_numpy(pred.copy()).to(dev()), torch.from_numpy(label.copy()).to(dev()), K, spacing, tolerance=2.0)
    print(f'surface {spacing}: counts {counts[:, :2].tolist()}, worst relative distance error {worst:.3e} (bound {RTOL:.0e})')
    for key in V.KEYS:
        print(f'  {key}: {got[key].tolist()} reference {ref[key].tolist()}')
        assert got[key].shape == (K,) and got[key].dtype == np.float64
        assert np.allclose(got[key], ref[key], rtol=RTOL, atol=0.0, equal_nan=True)


def test_surface_sets_do_not_depend_on_the_workspace():
    pred, label, K, _ = _surface_case()
    (da, ca), (db, cb) = (_raw_surface(pred, label, K, SURFACE_SPACINGS[1], pattern) for pattern in PATTERNS)
    assert np.array_equal(ca, cb)
    for c in range(K):
        for d in range(2):
            n = ca[c, d]
            assert np.array_equal(da[c, d, :n], db[c, d, :n])


def test_surface_metrics_and_dice_of_empty_and_full_volumes():
    from pacingpseudo_amd.utils import volume_dice, volume_surface_metrics
    K = 3
    label = np.zeros((3, 10, 12), np.int64)
    label[1, 3:7, 3:8] = 1
    pred = np.zeros_like(label)                          # class 1: empty prediction; class 2: both empty; class 0: the prediction fills the volume
    p, t = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev())
    got = volume_surface_metrics(p, t, K, (2.0, 1.0, 1.0))
    for key in V.KEYS:
        assert np.isnan(got[key]).all(), (key, got[key])
    back = volume_surface_metrics(t, p, K, (2.0, 1.0, 1.0))          # class 1: empty label
    for key in V.KEYS:
        assert np.isnan(back[key]).all(), (key, back[key])
    dice = volume_dice(p, t, K)
    ref = V.dice(pred, label, K)
    assert np.isnan(dice[2]) and dice[1] == 0.0 and np.allclose(dice, ref, rtol=1e-12, atol=0.0, equal_nan=True)
    same = volume_surface_metrics(t, t, K, (2.0, 1.0, 1.0))
    assert same['hd'][1] == 0.0 and same['assd'][1] == 0.0 and same['nsd'][1] == 1.0 and np.isfinite(same['hd'][0])
    assert np.array_equal(volume_dice(t, t, K)[:2], [1.0, 1.0])


# ---------------------------------------------------------------- the driver
def _run_inference(tmp_path, session, *flags):
    ckp = tmp_path / 'fold0_fresh.pth'
    if not ckp.exists():
        from pacingpseudo_amd.models import UNet
        torch.manual_seed(3)
        model = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                     elab_end_points=False)
        torch.save(model.state_dict(), str(ckp))
    cmd = [sys.executable, os.path.join(ROOT, 'inference.py'), '--gpu', '0', '--fold', '0', '--checkpoint_file', str(ckp), '--dataset', 'chaost1',
           '--root', str(tmp_path), '--session', session, '--init_ch', '8', '--max_ch', '64', '--num_workers', '0', '--batch_size', '3',
           *flags]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r, os.path.join(str(tmp_path), session, 'chaost1', 'fold0_fresh.pth')


def _stacked_maps(ckp, K):
    """What the driver stacks, recomputed in this process: evaluate() on the same checkpoint and slices with a volume_maps list ->
    (the per-slice Dice array of that run, [(class map, label) per volume, uint8 (4, 64, 64) on the device])."""
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticVolumes, collate_by_shape
    from pacingpseudo_amd.models import UNet
    model = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                 elab_end_points=False).to(dev())
    I.load_backbone(model, torch.load(ckp, map_location=dev()))
    ds = SyntheticVolumes(8, K, depth=4, size=64, train=False, seed=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, num_workers=0, collate_fn=collate_by_shape)
    maps = []
    dicearr = I.evaluate(model, loader, K, I.SPACING['chaost1'], dev(), True, 1, 'none', {}, surface_metrics=True, nsd_tolerance=2.0,
                         volume_maps=maps)[0]
    assert len(maps) == 8 and maps[0][0].dtype == torch.uint8 and maps[0][1].dtype == torch.uint8
    for i, (_, lab) in enumerate(maps):
        assert np.array_equal(lab.cpu().numpy(), ds.raw_arrays(i)[1])
    return dicearr, [(torch.stack([maps[4 * v + s][0] for s in range(4)]), torch.stack([maps[4 * v + s][1] for s in range(4)])) for v in range(2)]


def test_inference_driver_with_volumes(tmp_path):
    from pacingpseudo_amd.inference import SPACING
    from pacingpseudo_amd.utils import keep_largest_components_3d, volume_dice, volume_surface_metrics
    common = ('--synthetic', '8', '--synthetic_depth', '4', '--image_size', '64', '--keep_largest_cc', '--surface_metrics')
    r, child = _run_inference(tmp_path, 'vol', *common, '--volumes')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'overall volume Dice' in r.stdout
    z = np.load(os.path.join(child, 'eval_data.npz'))
    K = 5
    vol_keys = {'vol_ids', 'vol_slices', 'vol_dicearr', 'vol_hd95arr', 'vol_hdarr', 'vol_assdarr', 'vol_nsdarr', 'vol_ncomp', 'vol_removed'}
    assert {k for k in z.files if k.startswith('vol_')} == vol_keys
    assert z['vol_ids'].tolist() == ['vol000', 'vol001'] and z['vol_slices'].tolist() == [4, 4]
    for key in vol_keys - {'vol_ids', 'vol_slices'}:
        assert z[key].shape == (2, K), (key, z[key].shape)
    assert z['dicearr'].shape == (8, K)

    # the vol_* arrays are the stand-alone functions applied to the stacked maps
    dicearr, volumes = _stacked_maps(str(tmp_path / 'fold0_fresh.pth'), K)
    assert dicearr.tobytes() == z['dicearr'].tobytes()                    # this process scored the slices the driver scored
    sy, sx = SPACING['chaost1']
    for v, (raw, lab) in enumerate(volumes):
        assert raw.shape == (4, 64, 64)
        pred, stats = keep_largest_components_3d(raw.to(torch.int64), K, 1, return_stats=True)
        assert np.array_equal(z['vol_ncomp'][v], stats[:, 0].cpu().numpy()) and np.array_equal(z['vol_removed'][v], stats[:, 1].cpu().numpy())
        assert np.array_equal(z['vol_dicearr'][v], volume_dice(pred, lab, K).astype(np.float32), equal_nan=True)
        sm = volume_surface_metrics(pred, lab, K, (sy, sy, sx), tolerance=2.0)          # --synthetic: the slice pitch is the in-plane one
        for key, name in (('hdp', 'vol_hd95arr'), ('hd', 'vol_hdarr'), ('assd', 'vol_assdarr'), ('nsd', 'vol_nsdarr')):
            assert np.array_equal(z[name][v], sm[key].astype(np.float32), equal_nan=True), name

    # without --volumes: the same per-slice arrays bit for bit, and no vol_* key
    r2, child2 = _run_inference(tmp_path, 'slices', *common)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    z2 = np.load(os.path.join(child2, 'eval_data.npz'))
    assert not [k for k in z2.files if k.startswith('vol_')] and 'overall volume Dice' not in r2.stdout
    assert set(z2.files) == {k for k in z.files if not k.startswith('vol_')}
    for key in z2.files:
        assert z2[key].tobytes() == z[key].tobytes() and z2[key].shape == z[key].shape, key


def test_inference_driver_needs_a_slice_spacing_on_real_data(tmp_path):
    r, _ = _run_inference(tmp_path, 'bad', '--volumes')
    assert r.returncode == 2 and '--slice_spacing' in r.stderr
