"""The size threshold and hole filling on the device (libpacingpseudo_morph.so, utils.morphology, inference.py --min_component_size /
--fill_holes) against the numpy / scipy restatement of tests/_morph_reference.py.  Integer work with an exact oracle: every output
and every statistic must be EQUAL, there is no tolerance.  The raw entry points run between the sentinel bands of tests/_guard.py."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _cc_reference as C2  # noqa: E402
from tests import _morph_reference as M  # noqa: E402
from tests import _vol_reference as V  # noqa: E402
from tests._guard import PATTERNS, BandSet  # noqa: E402

pytestmark = pytest.mark.gpu

MIN_SIZE = 4


def dev():
    return torch.device('cuda', 0)


def _stream():
    from pacingpseudo_amd._lib import stream_ptr
    return stream_ptr()


def _labels(cm, dims, connectivity):
    """What the existing labellers write for cm: (N, H, W) per slice, or one (D, H, W) volume."""
    from pacingpseudo_amd.utils import label_components, label_components_3d
    x = torch.from_numpy(np.ascontiguousarray(cm, np.int64)).to(dev())
    return label_components(x, connectivity) if dims == 2 else label_components_3d(x, connectivity)


def _dims_of(cm, dims):
    return (cm.shape[0], 1) + cm.shape[1:] if dims == 2 else (1,) + cm.shape


def _raw(kind, cm, K, dims, connectivity, min_size=MIN_SIZE, pattern=0xFF, labels=None, alias=False):
    """pmor_remove_small / pmor_fill_holes between sentinel bands -> (out, stats (N, K, 2)) as numpy."""
    from pacingpseudo_amd._morph import morph
    N, D, H, W = _dims_of(cm, dims)
    if labels is None:
        labels = _labels(cm, dims, connectivity)
    bs = BandSet(pattern, dev())
    x = bs.banded(torch.from_numpy(np.ascontiguousarray(cm, np.int64)).to(dev()), label='cls')
    lab = bs.banded(labels.to(torch.int32).contiguous(), label='labels')
    out = x if alias else bs.banded(tuple(cm.shape), torch.int64, label='out')
    stats = bs.banded((N, K, 2), torch.int32, label='stats')
    ws = bs.ws(morph.pmor_workspace(N, K, D, H, W, dims), label='workspace')
    if kind == 'small':
        sizes = [min_size] * K if isinstance(min_size, int) else list(min_size)
        morph.pmor_remove_small(x.ptr(), lab.ptr(), N, K, D, H, W, dims, (ctypes.c_int32 * K)(*sizes), out.ptr(), stats.ptr(), ws.ptr(), ws.n,
                                _stream())
    else:
        morph.pmor_fill_holes(x.ptr(), lab.ptr(), N, K, D, H, W, dims, connectivity, out.ptr(), stats.ptr(), ws.ptr(), ws.n, _stream())
    assert bs.damaged() == []
    if not alias:
        assert np.array_equal(x.t.cpu().numpy(), cm)                     # the input is read only
    return out.t.cpu().numpy(), stats.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, K, dims):
    return M.random_map(shape, K, seed=sum(shape) + K)


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, K, dims, connectivity):
    """The reference per item, computed once per case and shared: (out, stats (N, K, 2))."""
    cm = _case(shape, K, dims)
    items = list(cm) if dims == 2 else [cm]
    f = (lambda a: M.remove_small(a, K, MIN_SIZE, connectivity)) if kind == 'small' else (lambda a: M.fill_holes(a, K, connectivity))
    res = [f(a) for a in items]
    out = np.stack([r[0] for r in res]) if dims == 2 else res[0][0]
    out.setflags(write=False)
    stats = np.stack([r[1] for r in res])
    stats.setflags(write=False)
    return out, stats


# ---------------------------------------------------------------- 2-D
SHAPES_2D = [(1, 1, 1), (1, 1, 130), (1, 130, 1), (3, 37, 53), (2, 64, 64), (2, 200, 70)]


@pytest.mark.parametrize('ch', [1, 2])
@pytest.mark.parametrize('c', [1, 2])
@pytest.mark.parametrize('shape', SHAPES_2D, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('K', [2, 5, 32])
def test_slices_equal_the_reference(K, shape, c, ch):
    cm = _case(shape, K, 2)
    out, stats = _raw('small', cm, K, 2, c)
    want, wstats = _reference('small', shape, K, 2, c)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    out, stats = _raw('fill', cm, K, 2, ch)
    want, wstats = _reference('fill', shape, K, 2, ch)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    if shape == (2, 200, 70):                                            # the branches the case is there for
        assert wstats[:, 1:, 0].sum() > 0 and (K == 2 or wstats[:, 0, 0].sum() > 0)
        if K == 32:
            assert wstats[:, 31, 0].sum() > 0                            # bit 31 of the contact mask decided a fill


# ---------------------------------------------------------------- 3-D
@pytest.mark.parametrize('connectivity', [1, 2, 3])
@pytest.mark.parametrize('shape', [(1, 40, 40), (5, 19, 33), (9, 16, 70)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('K', [2, 5, 32])
def test_volumes_equal_the_reference(K, shape, connectivity):
    cm = _case(shape, K, 3)
    out, stats = _raw('small', cm, K, 3, connectivity)
    want, wstats = _reference('small', shape, K, 3, connectivity)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    out, stats = _raw('fill', cm, K, 3, connectivity)
    want, wstats = _reference('fill', shape, K, 3, connectivity)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    if shape[0] == 1:
        assert np.array_equal(out, cm) and not stats.any()              # every voxel lies on a z face: no cavities
    elif connectivity == 1:
        assert wstats[0, 1:, 0].sum() > 0


def test_binary_fill_holes_is_scipys():
    from scipy import ndimage
    from pacingpseudo_amd.utils import binary_fill_holes
    for shape in ((37, 53), (9, 16, 70)):
        mask = np.random.RandomState(5).rand(*shape) < 0.6
        for ch in range(1, len(shape) + 1):
            got = binary_fill_holes(torch.from_numpy(mask).to(dev()), ch)
            assert got.dtype == torch.bool
            assert np.array_equal(got.cpu().numpy(), ndimage.binary_fill_holes(mask, M.structure(len(shape), ch)))


# ---------------------------------------------------------------- hand-drawn cases
@pytest.mark.parametrize('name', list(M.hand_drawn()))
def test_hand_drawn_cavities(name):
    from pacingpseudo_amd.utils import fill_holes
    case = M.hand_drawn()[name]
    cm, K, ch = case['cm'], case['K'], case['ch']
    want = cm.copy()
    for (y, x), k in case['filled'].items():
        want[y, x] = k
    out, stats = _raw('fill', cm[None], K, 2, ch)
    assert np.array_equal(out[0], want)
    assert np.array_equal(stats[0], M.fill_holes(cm, K, ch)[1]) and stats[0, 0, 0] == case['mixed']
    got, gstats = fill_holes(torch.from_numpy(cm).to(dev(), torch.uint8), K, ch, return_stats=True)       # the (H, W) form, dtype kept
    assert got.dtype == torch.uint8 and got.shape == cm.shape and gstats.shape == (K, 2)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(gstats.cpu().numpy(), stats[0])


def test_exactly_min_size_stays_and_one_less_goes():
    from pacingpseudo_amd.utils import remove_small_components, remove_small_components_3d
    cm, want = M.size_case(5)
    out, stats = _raw('small', cm[None], 3, 2, 1, min_size=5)
    assert np.array_equal(out[0], want) and stats[0].tolist() == [[0, 0], [1, 4], [1, 4]]
    x = torch.from_numpy(cm).to(dev())
    got, gstats = remove_small_components(x.to(torch.int16), 3, 5, return_stats=True)
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want) and gstats.cpu().numpy().tolist() == [[0, 0], [1, 4], [1, 4]]
    for sizes in ([0, 6, 1], (9, 5, 0), [0, 0, 0], [0, 1, 1]):           # per class; entry 0 is never read; <= 1 is a no-op
        want_k, wstats = M.remove_small(cm, 3, sizes)
        got, gstats = remove_small_components(x, 3, sizes, return_stats=True)
        assert np.array_equal(got.cpu().numpy(), want_k) and np.array_equal(gstats.cpu().numpy(), wstats), sizes
        vol = np.stack([cm, cm])                                         # as a volume: the two copies join, every size doubles
        want_v, wstats = M.remove_small(vol, 3, [2 * s for s in sizes])
        got, gstats = remove_small_components_3d(torch.from_numpy(vol).to(dev()), 3, [2 * s for s in sizes], return_stats=True)
        assert np.array_equal(got.cpu().numpy(), want_v) and np.array_equal(gstats.cpu().numpy(), wstats), sizes


# ---------------------------------------------------------------- values outside [0, K), K = 1
def test_values_outside_the_classes_are_copied_and_veto_a_fill():
    cm = _case((3, 37, 53), 5, 2).copy()
    rng = np.random.RandomState(11)
    cm[rng.rand(*cm.shape) < 0.05] = 255
    cm[rng.rand(*cm.shape) < 0.02] = -3
    cm[rng.rand(*cm.shape) < 0.02] = 5                                   # K itself
    for c in (1, 2):
        out, stats = _raw('small', cm, 5, 2, c)
        res = [M.remove_small(a, 5, MIN_SIZE, c) for a in cm]
        assert np.array_equal(out, np.stack([r[0] for r in res])) and np.array_equal(stats, np.stack([r[1] for r in res]))
        out, stats = _raw('fill', cm, 5, 2, c)
        res = [M.fill_holes(a, 5, c) for a in cm]
        assert np.array_equal(out, np.stack([r[0] for r in res])) and np.array_equal(stats, np.stack([r[1] for r in res]))
        strange = (cm < 0) | (cm >= 5)
        assert np.array_equal(out[strange], cm[strange])
    case = M.hand_drawn()['rim with a value outside [0, K)']
    out, stats = _raw('fill', case['cm'][None], 3, 2, 1)
    assert np.array_equal(out[0], case['cm']) and not stats.any()


@pytest.mark.parametrize('dims, shape', [(2, (3, 37, 53)), (3, (5, 19, 33))])
def test_one_class_changes_nothing(dims, shape):
    cm = _case(shape, 1, dims)
    assert (cm != 0).any() and (cm == 0).any()
    for kind in ('small', 'fill'):
        out, stats = _raw(kind, cm, 1, dims, 1)
        assert np.array_equal(out, cm) and stats.shape == (_dims_of(cm, dims)[0], 1, 2) and not stats.any()


# ---------------------------------------------------------------- aliasing, stale workspaces, repeated runs
@pytest.mark.parametrize('dims, shape', [(2, (3, 37, 53)), (3, (9, 16, 70))])
def test_out_may_alias_cls_and_nothing_depends_on_stale_memory(dims, shape):
    K = 5
    cm = _case(shape, K, dims)
    for kind in ('small', 'fill'):
        want, wstats = _reference(kind, shape, K, dims, 1)
        runs = [_raw(kind, cm, K, dims, 1, pattern=p, alias=a) for p in PATTERNS for a in (False, True)]
        runs.append(_raw(kind, cm, K, dims, 1))                          # and once more: the same bits in every run
        for out, stats in runs:
            assert out.tobytes() == want.tobytes() and stats.tobytes() == wstats.tobytes()


# ---------------------------------------------------------------- garbage labels
@pytest.mark.parametrize('dims, shape', [(2, (2, 64, 64)), (3, (5, 19, 33))])
def test_labels_no_labeller_writes_are_never_an_index(dims, shape):
    """Labels that are negative, >= n or greater than the voxel's own index: the call returns, the bands are intact, and those voxels
    are copied.  The expected output restates the header on the damaged labels themselves: such a voxel adds nothing to any root."""
    K = 5
    cm = _case(shape, K, dims)
    N, D, H, W = _dims_of(cm, dims)
    n = D * H * W
    labels = _labels(cm, dims, 1).cpu().numpy().reshape(N, n).copy()
    idx = np.arange(n)[None].repeat(N, 0)
    rng = np.random.RandomState(2)
    pick = rng.rand(N, n) < 0.1
    kind_of = rng.randint(0, 4, size=(N, n))
    labels[pick & (kind_of == 0)] = -1
    labels[pick & (kind_of == 1)] = -2 ** 31
    labels[pick & (kind_of == 2)] = n + 7
    labels[pick & (kind_of == 3)] = 2 ** 31 - 1
    above = rng.rand(N, n) < 0.05                                        # in range, but past the voxel itself
    above[:, -1] = False
    labels[above] = np.minimum(idx[above] + 1 + rng.randint(0, 50, size=int(above.sum())), n - 1)
    bad = (labels < 0) | (labels > idx)
    assert bad.sum() > 0.1 * N * n and (labels[bad] >= n).any() and ((labels[bad] > idx[bad]) & (labels[bad] < n)).any()
    flat = cm.reshape(N, n)
    dev_labels = torch.from_numpy(labels.astype(np.int32).reshape(cm.shape)).to(dev())

    out, stats = _raw('small', cm, K, dims, 1, labels=dev_labels)
    want = flat.copy()
    for i in range(N):
        counted = ~bad[i] & (flat[i] >= 1) & (flat[i] < K)
        sizes = np.bincount(labels[i][counted], minlength=n)
        gone = counted & (sizes[np.where(bad[i], 0, labels[i])] < MIN_SIZE)
        want[i][gone] = 0
    assert np.array_equal(out.reshape(N, n), want)
    assert np.array_equal(out.reshape(N, n)[bad], flat[bad])
    assert np.array_equal(stats[..., 1], np.stack([np.bincount(flat[i][want[i] != flat[i]], minlength=K)[:K] for i in range(N)]))

    out, stats = _raw('fill', cm, K, dims, 1, labels=dev_labels)
    assert np.array_equal(out.reshape(N, n)[bad], flat[bad])
    assert np.array_equal(out[cm != 0], cm[cm != 0])                     # whatever the labels say, nothing non-zero is overwritten
    changed = out != cm
    assert ((out[changed] >= 1) & (out[changed] < K)).all()
    assert np.array_equal(stats[:, 1:, 1], np.stack([np.bincount(out.reshape(N, n)[i][changed.reshape(N, n)[i]], minlength=K)[1:K]
                                                     for i in range(N)]))


# ---------------------------------------------------------------- the chain, as the driver orders it
@pytest.mark.parametrize('dims, shape', [(2, (3, 37, 53)), (3, (9, 16, 70))])
def test_threshold_keep_largest_fill_in_that_order(dims, shape):
    from pacingpseudo_amd.utils import (fill_holes, fill_holes_3d, keep_largest_components, keep_largest_components_3d,
                                        remove_small_components, remove_small_components_3d)
    K = 5
    cm = _case(shape, K, dims)
    x = torch.from_numpy(cm).to(dev())
    if dims == 2:
        got = fill_holes(keep_largest_components(remove_small_components(x, K, MIN_SIZE, 2), K, 2), K, 1)
        want = np.stack([M.chain(a, K, MIN_SIZE, 2, C2.keep_largest, 1) for a in cm])
    else:
        got = fill_holes_3d(keep_largest_components_3d(remove_small_components_3d(x, K, MIN_SIZE, 2), K, 2), K, 1)
        want = M.chain(cm, K, MIN_SIZE, 2, V.keep_largest, 1)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, cm)


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
           '--image_size', '64', *flags]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r, os.path.join(str(tmp_path), session, 'chaost1', 'fold0_fresh.pth')


def _evaluate_here(ckp, K, dataset, **kwargs):
    """evaluate() in this process on the checkpoint and slices of the driver run -> (returned arrays, extra, volume maps)."""
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import collate_by_shape
    from pacingpseudo_amd.models import UNet
    model = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                 elab_end_points=False).to(dev())
    I.load_backbone(model, torch.load(ckp, map_location=dev()))
    loader = torch.utils.data.DataLoader(dataset, batch_size=3, shuffle=False, num_workers=0, collate_fn=collate_by_shape)
    extra, maps = {}, []
    res = I.evaluate(model, loader, K, I.SPACING['chaost1'], dev(), extra=extra, volume_maps=maps, **kwargs)
    return res, extra, maps


def test_inference_driver_with_the_slice_stages(tmp_path):
    from pacingpseudo_amd.data import SyntheticPhantoms
    K = 5
    r0, child0 = _run_inference(tmp_path, 'plain', '--synthetic', '8')
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-3000:]
    z0 = np.load(os.path.join(child0, 'eval_data.npz'))
    assert set(z0.files) == {'dicearr', 'hd95arr'}
    assert 'Hole filling' not in r0.stdout and 'Size threshold' not in r0.stdout
    for flag in ('min_component_size', 'fill_holes'):
        assert flag not in r0.stdout                                     # the argument dump of a run without the flags

    r, child = _run_inference(tmp_path, 'morph', '--synthetic', '8', '--fill_holes', '--min_component_size', '20')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Size threshold (20 pixels, connectivity 1)' in r.stdout and 'Hole filling (connectivity 1)' in r.stdout
    assert 'min_component_size=20' in r.stdout and 'fill_holes=True' in r.stdout
    z = np.load(os.path.join(child, 'eval_data.npz'))
    assert set(z.files) == {'dicearr', 'hd95arr', 'small_removed', 'holes_filled', 'holes_mixed'}
    assert z['small_removed'].shape == (8, K) and z['holes_filled'].shape == (8, K) and z['holes_mixed'].shape == (8,)
    assert z['small_removed'].dtype == np.int32 and z['holes_filled'].dtype == np.int32
    assert z['dicearr'].shape == (8, K) and z['hd95arr'].shape == (8, K)
    assert not z['small_removed'][:, 0].any() and not z['holes_filled'][:, 0].any()

    # this process: the flag-less run is what evaluate gives without the stages, the other one what it gives with them, and the
    # stages are the stand-alone functions in the stated order on the map the driver filters
    ds = SyntheticPhantoms(8, K, size=64, train=False, seed=1, native=True, compact=True)
    ckp = str(tmp_path / 'fold0_fresh.pth')
    (dice0, hd0), extra0, maps = _evaluate_here(ckp, K, ds)
    assert dice0.tobytes() == z0['dicearr'].tobytes() and hd0.tobytes() == z0['hd95arr'].tobytes() and extra0 == {}
    (dice1, hd1), extra1, _ = _evaluate_here(ckp, K, ds, min_component_size=20, fill_holes=True)
    assert dice1.tobytes() == z['dicearr'].tobytes() and hd1.tobytes() == z['hd95arr'].tobytes()
    for key in ('small_removed', 'holes_filled', 'holes_mixed'):
        assert np.array_equal(extra1[key], z[key]), key
    for i, (raw, _) in enumerate(maps):
        a = raw.cpu().numpy().astype(np.int64)
        small, sstats = M.remove_small(a, K, 20, 1)
        _, fstats = M.fill_holes(small, K, 1)
        assert np.array_equal(z['small_removed'][i], sstats[:, 1]) and np.array_equal(z['holes_filled'][i][1:], fstats[1:, 1])
        assert z['holes_mixed'][i] == fstats[0, 0]
    untouched = (z['small_removed'].sum(1) == 0) & (z['holes_filled'].sum(1) == 0)
    assert np.array_equal(z['dicearr'][untouched], z0['dicearr'][untouched], equal_nan=True)
    # (what a fresh network predicts decides whether anything is removed here: test_evaluate_runs_the_stages_in_order plants the work)


class _Replay(torch.nn.Module):
    """Stands in for the network: answers the k-th batch with the one-hot planes of the next class maps of a list."""

    def __init__(self, maps, K):
        super().__init__()
        self.maps, self.K, self.at = maps, K, 0

    def forward(self, x):
        m = self.maps[self.at:self.at + x.shape[0]]
        self.at += x.shape[0]
        return {'segmentation/logits': torch.nn.functional.one_hot(m, self.K).permute(0, 3, 1, 2).float()}


def test_evaluate_runs_the_stages_in_order():
    """evaluate() on planted predictions: labels with specks, pin-holes and islands.  Its counters are the reference's, stage by
    stage, and its scores are bit for bit those of a stage-less evaluate() that is handed the reference chain's result."""
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms, collate_by_shape
    K, n = 5, 6
    ds = SyntheticPhantoms(n, K, size=64, train=False, seed=1, native=True, compact=True)
    rng = np.random.RandomState(4)
    maps = np.stack([ds.raw_arrays(i)[1] for i in range(n)]).astype(np.int64)
    hit = rng.rand(*maps.shape) < 0.03
    maps[hit] = rng.randint(1, K, size=int(hit.sum()))
    maps[rng.rand(*maps.shape) < 0.03] = 0
    maps[:, 2:6, 2:9] = 1                                                # an island of 28 pixels: past the threshold, not the largest

    def run(planted, **kwargs):
        loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, num_workers=0, collate_fn=collate_by_shape)
        extra = {}
        res = I.evaluate(_Replay(torch.from_numpy(planted).to(dev()), K), loader, K, I.SPACING['chaost1'], dev(), extra=extra, **kwargs)
        return res, extra

    small = [M.remove_small(a, K, 20, 2) for a in maps]
    kept = [C2.keep_largest(s[0], K, 2) for s in small]
    filled = [M.fill_holes(k[0], K, 1) for k in kept]
    final = np.stack([f[0] for f in filled])
    res, extra = run(maps, keep_largest_cc=True, cc_connectivity=2, min_component_size=20, fill_holes=True, fill_holes_connectivity=1)
    assert len(res) == 4 and set(extra) == {'small_removed', 'holes_filled', 'holes_mixed'}
    assert np.array_equal(extra['small_removed'], np.stack([s[1][:, 1] for s in small])) and extra['small_removed'].sum() > 0
    assert np.array_equal(extra['holes_filled'][:, 1:], np.stack([f[1][1:, 1] for f in filled])) and extra['holes_filled'].sum() > 0
    assert np.array_equal(extra['holes_mixed'], np.array([f[1][0, 0] for f in filled]))
    assert np.array_equal(res[2], np.stack([k[1][:, 0] for k in kept]))                              # ncomp: after the threshold
    assert np.array_equal(res[3], np.array([(k[0] != s[0]).sum() for k, s in zip(kept, small)])) and res[3].sum() > 0
    ref, ref_extra = run(final)
    assert len(ref) == 2 and ref_extra == {}
    assert res[0].tobytes() == ref[0].tobytes() and res[1].tobytes() == ref[1].tobytes()
    plain, _ = run(maps)
    assert plain[0].tobytes() != res[0].tobytes()
    # one stage alone: the number of returned values follows keep_largest_cc only
    only, extra = run(maps, fill_holes=True, fill_holes_connectivity=2)
    assert len(only) == 2 and set(extra) == {'holes_filled', 'holes_mixed'}
    assert np.array_equal(extra['holes_filled'][:, 1:], np.stack([M.fill_holes(a, K, 2)[1][1:, 1] for a in maps]))


def test_inference_driver_with_the_volume_stages(tmp_path):
    from pacingpseudo_amd.data import SyntheticVolumes
    K = 5
    common = ('--synthetic', '8', '--synthetic_depth', '4', '--volumes')
    r, child = _run_inference(tmp_path, 'volmorph', *common, '--fill_holes', '--min_component_size', '20', '--min_component_size_3d', '30',
                              '--fill_holes_connectivity_3d', '2')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'Size threshold in 3-D (30 voxels, connectivity 1)' in r.stdout and 'Hole filling in 3-D (connectivity 2)' in r.stdout
    z = np.load(os.path.join(child, 'eval_data.npz'))
    assert {'vol_small_removed', 'vol_holes_filled', 'vol_holes_mixed', 'small_removed', 'holes_filled', 'holes_mixed'} <= set(z.files)
    assert z['vol_small_removed'].shape == (2, K) and z['vol_holes_filled'].shape == (2, K) and z['vol_holes_mixed'].shape == (2,)
    ds = SyntheticVolumes(8, K, depth=4, size=64, train=False, seed=1)
    _, _, maps = _evaluate_here(str(tmp_path / 'fold0_fresh.pth'), K, ds)
    for v in range(2):                                                   # 3-D stages on the stacked, unfiltered slice maps
        raw = np.stack([maps[4 * v + s][0].cpu().numpy() for s in range(4)]).astype(np.int64)
        small, sstats = M.remove_small(raw, K, 30, 1)
        _, fstats = M.fill_holes(small, K, 2)
        assert np.array_equal(z['vol_small_removed'][v], sstats[:, 1])
        assert np.array_equal(z['vol_holes_filled'][v][1:], fstats[1:, 1]) and z['vol_holes_mixed'][v] == fstats[0, 0]
