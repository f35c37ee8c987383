"""Geodesic scribbles on the MI355X (libpacingpseudo_geo.so, utils/geodesic.py, --geo_scribbles) against the float32 Dijkstra of
tests/_geo_reference.py.  The guide is always taken from the device (``return_guide=True``, or ``normalize=False`` with a given
guide), so every comparison of `dist` and of the labels is EXACT EQUALITY of bits: the definition's fixed point is unique whatever
order the kernel relaxes pixels in.  No pixel is excluded anywhere.

The kernel's tile is 64 x 64: the shapes of test 1 lie below a tile, on exactly one tile and one pixel past a tile edge in each axis.
Recorded from the reference: the farthest finite distance is 593.34 on the 67 x 67 spiral and 2575.84 on the 33 x 130 comb (walls of
100, lam = 5), against 3 (H + W) = 402 and 489: the walls bind."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _geo_reference as R
from tests._guard import BandSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
INF = np.float32(np.inf)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _device_dist(g, scb, K, lam, sizes=None, **kw):
    """(dist, stats) as numpy from guides (N, H, W) given as they are (normalize=False)."""
    from pacingpseudo_amd.utils import geodesic_distance
    d, st = geodesic_distance(_t(g, torch.float32), _t(scb, torch.int64), K, sizes, lam=lam, normalize=False, return_stats=True, **kw)
    return d.cpu().numpy(), st.cpu().numpy()


def _seeded(rng, shape, K, per_class=2):
    scb = np.full(shape, K, dtype=np.int64)
    where = rng.choice(shape[0] * shape[1], K * per_class, replace=False)
    for i, p in enumerate(where):
        scb.flat[p] = i % K
    return scb


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 40), (40, 1), (7, 5), (64, 64), (65, 129), (130, 67)])
def test_random_guides_bit_for_bit(shape):
    K = 3
    rng = np.random.RandomState(shape[0] * 1000 + shape[1])
    g = rng.randn(*shape).astype(np.float32)
    scb = _seeded(rng, shape, K)
    for lam in (0.0, 3.0, 20.0):
        d, st = _device_dist(g[None], scb[None], K, lam)
        ref = R.distances(g, scb, K, lam)
        bad = int((_bits(d[0]) != _bits(ref)).sum())
        print(f'{shape} lam {lam}: passes {st[0, :, 0].tolist()}, {bad} pixels differ')
        assert bad == 0 and (st[0, :, 1] == 1).all() and (st[0, :, 0] >= 2).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maze', ['spiral', 'comb'])
def test_mazes(maze):
    g, seeds = R.spiral_maze(67, 100.0) if maze == 'spiral' else R.comb_maze(33, 130, 100.0)
    ref = R.dijkstra(g, seeds, 5.0)
    far = float(ref[np.isfinite(ref)].max())
    print(f'{maze}: farthest distance {far:.2f}, 3 (H + W) = {3 * sum(g.shape)}')
    assert np.isfinite(ref).all() and far > 3 * sum(g.shape)                  # the walls bind
    d, st = _device_dist(g[None], np.where(seeds, 0, 1)[None], 1, 5.0)
    print(f'{maze}: passes {st[0, 0, 0]}')
    assert _same(d[0, 0], ref) and st[0, 0, 1] == 1


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_nan_wall():
    rng = np.random.RandomState(3)
    g = rng.randn(9, 9).astype(np.float32)
    g[4] = np.nan
    scb = np.full((9, 9), 2)
    scb[1, 2], scb[3, 7] = 0, 1
    d, st = _device_dist(g[None], scb[None], 2, 3.0)
    assert np.isinf(d[0, :, 4:]).all() and np.isfinite(d[0, :, :4]).all() and (st[0, :, 1] == 1).all()
    assert _same(d[0], R.distances(g, scb, 2, 3.0))


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_batches_with_sizes_and_padding():
    from pacingpseudo_amd.utils import geodesic_distance, geodesic_expand_scribbles
    K, H, W = 3, 70, 72
    sizes = [(70, 72), (33, 65), (64, 17)]
    rng = np.random.RandomState(4)
    img = (rng.randn(3, H, W) * 40 + 100).astype(np.float32)
    scb = np.full((3, H, W), K, dtype=np.int64)
    for n, (h, w) in enumerate(sizes):
        scb[n, :h, :w] = _seeded(rng, (h, w), K)
    got = {}
    for pad in (0.0, 1e30):
        im = img.copy()
        for n, (h, w) in enumerate(sizes):
            im[n, h:, :], im[n, :, w:] = pad, pad
        d, st, g = geodesic_distance(_t(im), _t(scb), K, sizes, lam=20.0, return_stats=True, return_guide=True)
        lab = geodesic_expand_scribbles(_t(im), _t(scb), K, sizes, ratio=1.0)
        gp = g.clone()                                    # ... and the guide itself padded, taken as given
        for n, (h, w) in enumerate(sizes):
            gp[n, h:, :], gp[n, :, w:] = pad, pad
        d2 = geodesic_distance(gp, _t(scb), K, sizes, lam=20.0, normalize=False)
        assert torch.equal(d.view(torch.int32), d2.view(torch.int32))
        got[pad] = (d.cpu().numpy(), st.cpu().numpy(), g.cpu().numpy(), lab.cpu().numpy())
    for a, b in zip(got[0.0], got[1e30]):
        assert np.array_equal(a, b) if a.dtype.kind == 'i' else _same(a, b)
    d, st, g, lab = got[0.0]
    for n, (h, w) in enumerate(sizes):
        assert np.isinf(d[n, :, h:, :]).all() and np.isinf(d[n, :, :, w:]).all() and (d[n, :, h:, :] > 0).all()
        assert (lab[n, h:, :] == K).all() and (lab[n, :, w:] == K).all()
        assert not g[n, h:, :].any() and not g[n, :, w:].any()
        ref = R.distances(g[n, :h, :w], scb[n, :h, :w], K, 20.0)
        assert _same(d[n, :, :h, :w], ref), n
        assert np.array_equal(lab[n, :h, :w], R.labels(ref, scb[n, :h, :w], K, ratio=1.0))
        alone, st1 = geodesic_distance(_t(np.ascontiguousarray(img[n, :h, :w])[None]), _t(np.ascontiguousarray(scb[n, :h, :w])[None]), K,
                                       lam=20.0, return_stats=True)
        assert _same(alone.cpu().numpy()[0], d[n, :, :h, :w]) and (st[n, :, 1] == 1).all()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_slices_beside_a_normal_one():
    from pacingpseudo_amd.utils import geodesic_expand_scribbles
    K, S = 3, 20
    rng = np.random.RandomState(5)
    g = rng.randn(3, S, S).astype(np.float32)
    scb = np.full((3, S, S), K, dtype=np.int64)
    scb[0] = _seeded(rng, (S, S), K)                      # class 2 is seeded in this slice only
    scb[2] = 1                                            # every pixel a seed of class 1; slice 1 has no seed at all
    d, st = _device_dist(g, scb, K, 3.0)
    assert _same(d[0], R.distances(g[0], scb[0], K, 3.0)) and (st[0, :, 1] == 1).all() and (st[0, :, 0] >= 2).all()
    assert np.isinf(d[1]).all() and (d[1] > 0).all() and st[1].tolist() == [[0, 1]] * K
    assert not d[2, 1].any() and st[2].tolist() == [[0, 1], [1, 1], [0, 1]] and np.isinf(d[2, [0, 2]]).all()
    lab = geodesic_expand_scribbles(_t(g), _t(scb), K, lam=3.0, ratio=1.0, normalize=False).cpu().numpy()
    assert (lab[1] == K).all() and (lab[2] == 1).all() and np.array_equal(lab[0], R.labels(d[0], scb[0], K, ratio=1.0))


@pytest.mark.parametrize('K', [1, 2, 32])
def test_class_counts(K):
    rng = np.random.RandomState(50 + K)
    g = rng.randn(12, 13).astype(np.float32)
    scb = _seeded(rng, (12, 13), K, per_class=1)
    d, st = _device_dist(g[None], scb[None], K, 3.0)
    assert _same(d[0], R.distances(g, scb, K, 3.0)) and (st[0, :, 1] == 1).all()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_labels():
    from pacingpseudo_amd.utils import geodesic_expand_scribbles
    K = 3
    rng = np.random.RandomState(6)
    g = rng.randn(2, 37, 70).astype(np.float32)
    scb = np.stack([_seeded(rng, (37, 70), K), _seeded(rng, (37, 70), K)])
    ref = [R.distances(g[n], scb[n], K, 3.0) for n in range(2)]
    for ratio in (0.25, 1.0):
        for max_dist in (np.inf, 10.0):
            lab, dist = geodesic_expand_scribbles(_t(g), _t(scb, torch.uint8), K, lam=3.0, ratio=ratio, max_dist=max_dist, normalize=False,
                                                  return_dist=True)
            assert lab.dtype == torch.uint8
            lab, dist = lab.cpu().numpy(), dist.cpu().numpy()
            for n in range(2):
                assert np.array_equal(lab[n], R.labels(dist[n], scb[n], K, ratio, max_dist))          # the rule on the device's field
                assert np.array_equal(lab[n], R.labels(ref[n], scb[n], K, ratio, max_dist))           # ... and the whole chain
            print(f'ratio {ratio} max_dist {max_dist}: labelled share {(lab != K).mean():.4f}')
    # a tie goes to the first class
    tie = geodesic_expand_scribbles(_t(np.zeros((1, 1, 5), np.float32)), _t(np.array([[[0, 2, 2, 2, 1]]])), 2, lam=0.0, ratio=1.0,
                                    normalize=False)
    assert tie.cpu().tolist() == [[[0, 0, 0, 1, 1]]]
    # one seeded class labels everything within max_dist
    one = np.full((37, 70), K)
    one[5, 9] = 1
    lab, dist = geodesic_expand_scribbles(_t(g[:1]), _t(one[None]), K, lam=0.5, ratio=0.25, max_dist=10.0, normalize=False, return_dist=True)
    lab, dist = lab.cpu().numpy()[0], dist.cpu().numpy()[0]
    assert np.array_equal(lab == 1, dist[1] <= 10.0) and ((lab == 1) | (lab == K)).all() and 50 < (lab == 1).sum() < 37 * 70


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_normalisation():
    from pacingpseudo_amd.utils import geodesic_distance
    H, W = 37, 70
    sizes = [(37, 70), (20, 33), (37, 1)]
    rng = np.random.RandomState(7)
    img = (rng.rand(3, H, W) * 900 + rng.randn(3, 1, 1) * 50).astype(np.float32)
    scb = np.full((3, H, W), 2, dtype=np.int64)
    scb[:, 0, 0] = 0
    _, g = geodesic_distance(_t(img), _t(scb), 2, sizes, return_guide=True)
    g = g.cpu().numpy()
    differ = 0
    for n, (h, w) in enumerate(sizes):
        want = R.normalise(img[n, :h, :w])
        err = np.abs(g[n, :h, :w].astype(np.float64) - want.astype(np.float64))
        differ += int((g[n, :h, :w] != want).sum())
        assert (err <= np.spacing(np.abs(want))).all(), (n, float(err.max()))
    print(f'normalisation: {differ} of {sum(h * w for h, w in sizes)} pixels are not the float64 formula rounded once (all within 1 ulp)')
    flat = np.full((1, 9, 11), 37.25, dtype=np.float32)
    _, g = geodesic_distance(_t(flat), _t(scb[:1, :9, :11]), 2, return_guide=True)
    assert not g.cpu().numpy().any()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_sweep_cap():
    g, seeds = R.comb_maze(33, 130, 100.0)
    ref = R.dijkstra(g, seeds, 5.0)
    gg = np.stack([g, np.zeros_like(g)])
    scb = np.stack([np.where(seeds, 0, 2), np.zeros(g.shape, dtype=np.int64)])          # slice 1: every pixel a seed of class 0
    d, st = _device_dist(gg, scb, 2, 5.0, max_sweeps=1)
    assert st[0, 0].tolist() == [1, 0] and (d[0, 0] >= ref).all() and d[0, 0][seeds].tolist() == [0.0] and not _same(d[0, 0], ref)
    assert st[0, 1].tolist() == [0, 1] and np.isinf(d[0, 1]).all()
    assert st[1].tolist() == [[1, 1], [0, 1]] and not d[1, 0].any() and np.isinf(d[1, 1]).all()
    d, st = _device_dist(gg, scb, 2, 5.0)                  # without the cap: the same call converges
    assert _same(d[0, 0], ref) and st[0, 0, 1] == 1 and st[0, 0, 0] > 2


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_same_bits_everywhere_and_sentinel_bands():
    from pacingpseudo_amd._geo import geo
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd.utils import geodesic_expand_scribbles
    N, K, H, W = 3, 3, 70, 72
    sizes = [(70, 72), (33, 65), (64, 17)]
    rng = np.random.RandomState(9)
    img = _t(rng.randn(N, H, W).astype(np.float32))
    scb_h = np.full((N, H, W), K, dtype=np.int64)
    for n, (h, w) in enumerate(sizes):
        scb_h[n, :h, :w] = _seeded(rng, (h, w), K)
    scb = _t(scb_h)
    kw = dict(lam=20.0, ratio=1.0, return_stats=True, return_dist=True)
    want = geodesic_expand_scribbles(img, scb, K, sizes, **kw)
    again = geodesic_expand_scribbles(img, scb, K, sizes, **kw)
    alone = geodesic_expand_scribbles(img[1:2].contiguous(), scb[1:2].contiguous(), K, sizes[1:2], **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = geodesic_expand_scribbles(img, scb, K, sizes, **kw)
    side.synchronize()
    for x, y, z, one in zip(want, again, other, alone):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x[1:2], one)
    host = np.ascontiguousarray(np.asarray(sizes, np.int32))
    hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for pattern in (0xFF, 0xA5):
        bs = BandSet(pattern, DEV)
        g_img, g_scb = bs.tensor(img, label='img'), bs.tensor(scb.to(torch.int32), label='scb')
        g = bs.banded((N, H, W), torch.float32, 'guide')
        dist, stats = bs.banded((N, K, H, W), torch.float32, 'dist'), bs.banded((N, K, 2), torch.int32, 'stats')
        out = bs.banded((N, H, W), torch.int32, 'labels')
        nbytes = geo.pgeo_distance_workspace(N, K, H, W)
        ws = bs.ws(nbytes, 'workspace')
        geo.pgeo_normalize(g_img.data_ptr(), hp, N, H, W, g.ptr(), stream_ptr())
        geo.pgeo_distance(g.ptr(), g_scb.data_ptr(), hp, N, K, H, W, 20.0, 100000, dist.ptr(), stats.ptr(), ws.ptr(), nbytes, stream_ptr())
        geo.pgeo_labels(dist.ptr(), g_scb.data_ptr(), hp, N, K, H, W, float('inf'), 1.0, out.ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert bs.damaged() == []
        for x, w_ in zip((out.t, stats.t, dist.t), want):          # nothing stale read, nothing left unwritten
            assert torch.equal(x.to(w_.dtype), w_)


# 10 --------------------------------------------------------------------------------------------------------------------------
DRIVER = ['--synthetic', '8', '--image_size', '32', '--batch_size', '4', '--num_workers', '0', '--init_ch', '8', '--max_ch', '64']


def test_driver_expands_once(tmp_path):
    from tests.test_gpu_resume import _run
    run = _run('train_chaos.py', DRIVER + ['--epoch', '1', '--geo_scribbles'], tmp_path / 'geo', 'g', session='Control')
    log = open(os.path.join(run, 'log.txt')).read()
    line = [ln for ln in log.splitlines() if 'geodesic scribbles: 8 slices' in ln]
    assert len(line) == 1 and 'coverage' in line[0] and 'agreement' in line[0] and '0 unconverged planes' in line[0], log[-2000:]
    z = np.load(os.path.join(run, 'geo_scribbles.npz'))
    assert z['sweeps'].shape == (8, 5) and z['converged'].all() and (z['coverage_after'] > z['coverage_before']).all()
    assert float(z['param_lam']) == 20.0 and float(z['param_ratio']) == 0.25 and np.isinf(z['param_max_dist']) and int(z['param_max_sweeps']) == 100000
    assert not os.path.exists(os.path.join(run, 'rw_scribbles.npz'))


def test_driver_resumes_bit_for_bit(tmp_path):
    """Two epochs, so that there is an epoch to resume into; the resumed process recomputes the expansion: the same bits."""
    from tests.test_gpu_resume import _resume_case
    full, resumed, _ = _resume_case(tmp_path, 'train_chaos.py', DRIVER + ['--epoch', '2', '--geo_scribbles'], 0, 1, session='Control')
    z, z2 = np.load(os.path.join(full, 'geo_scribbles.npz')), np.load(os.path.join(resumed, 'geo_scribbles.npz'))
    assert all(np.array_equal(z[k], z2[k], equal_nan=True) for k in z.files)


def test_expanded_planes_reach_the_model():
    """The data set the driver builds, with the override the driver computes: the scribble planes of the batches it hands to the
    model label more pixels than without the flag, on the GPU-augmentation path and on the --cpu_input path."""
    from pacingpseudo_amd.augment import AugConfig, DeviceAugmenter, collate_raw
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import check_geo_params, expand_dataset_geo
    K, S = 5, 32
    counts = {}
    for raw in (True, False):
        ds = SyntheticPhantoms(8, K, size=S, raw=raw, seed=1)
        maps, rep = expand_dataset_geo(ds, K, torch.device(DEV), check_geo_params(K=K))
        assert all(m.dtype == np.uint8 and m.shape == (S, S) for m in maps) and (rep['coverage_after'] > rep['coverage_before']).all()
        assert rep['converged'].all() and 'mindist' not in rep
        for on in (False, True):
            ds.scribble_override = maps if on else None
            items = [ds[i] for i in range(8)]
            if raw:
                batch = collate_raw(items)
                aug = DeviceAugmenter(AugConfig(num_classes=K, crop_size=(S, S)), device=DEV, seed=3)
                scribble = aug(batch['img'], batch['lab'], batch['scb'], batch['sizes'])['scribble']
            else:
                scribble = torch.stack([it['scribble'] for it in items])
            assert scribble.shape == (8, K + 1, S, S)
            counts[raw, on] = float(scribble[:, :K].sum())
    assert counts[True, True] > 2 * counts[True, False] > 0 and counts[False, True] > 2 * counts[False, False] > 0, counts


def test_tool_writes_what_geodesic_expand_scribbles_returns(tmp_path):
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import geodesic_expand_scribbles
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'expand_scribbles.py'), '--synthetic', '4', '--image_size', '32',
                        '--method', 'geo', '--out', str(tmp_path / 'geo')], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'geodesic scribbles: 4 slices' in r.stdout
    files = sorted(glob.glob(str(tmp_path / 'geo' / '*.npz')))
    assert len(files) == 4
    ds = SyntheticPhantoms(4, 5, size=32, raw=True)
    raw = [ds.raw_arrays(i) for i in range(4)]
    labels, dist = geodesic_expand_scribbles(_t(np.stack([x[0] for x in raw]).astype(np.float32)), _t(np.stack([x[2] for x in raw]), torch.int64),
                                             5, return_dist=True)
    for i, f in enumerate(files):
        z = np.load(f)
        assert set(z.files) == {'uid', 'img', 'lab', 'scb', 'scb_orig', 'geo_mindist'}
        assert np.array_equal(z['scb'], labels[i].cpu().numpy()) and np.array_equal(z['scb_orig'], raw[i][2])
        assert np.array_equal(z['img'], raw[i][0]) and np.array_equal(z['lab'], raw[i][1])
        assert z['geo_mindist'].dtype == np.float16 and np.array_equal(z['geo_mindist'], dist[i].amin(0).to(torch.float16).cpu().numpy())
