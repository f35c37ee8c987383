"""Connected components and the keep-largest-component filter on the GPU against the scipy oracle (tests/_cc_reference.py).
Everything is integer and canonical, so every comparison is an equality: no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest
import torch

from tests import _cc_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (96, 80), (130, 67)]     # one tile, one row / column of tiles, partial tiles
DENSITIES = (0.3, 0.5, 0.6, 0.9)                                              # 0.6: the 4-connected percolation threshold


def _gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _labels(maps, c):
    from pacingpseudo_amd.utils import label_components
    return label_components(_gpu(maps), c).cpu().numpy()


def _keep(maps, K, c):
    from pacingpseudo_amd.utils import keep_largest_components
    out, stats = keep_largest_components(_gpu(maps), K, c, return_stats=True)
    return out.cpu().numpy(), stats.cpu().numpy()


def _keep_raw(maps, K, c, inplace):
    """The C entry point itself on a workspace full of garbage (every word it relies on must be initialised by the call), with
    `out` aliasing `cls` when asked."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    x = _gpu(maps).to(torch.int64).contiguous()
    N, H, W = x.shape
    out = x if inplace else torch.empty_like(x)
    stats = torch.full((N, K, 2), -7, device='cuda', dtype=torch.int32)
    nws = lib.pp_components_workspace(N, K, H, W)
    ws = torch.full((nws,), 0xAB, device='cuda', dtype=torch.uint8)
    lib.pp_keep_largest_components(x.data_ptr(), N, K, H, W, c, out.data_ptr(), stats.data_ptr(), ws.data_ptr(), nws, stream_ptr())
    return out.cpu().numpy(), stats.cpu().numpy()


def _oracle_labels(maps, c):
    return np.stack([R.canonical_labels(m, c) for m in maps])


def _oracle_keep(maps, K, c):
    pairs = [R.keep_largest(m, K, c) for m in maps]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def _random_maps(shape):
    """Per shape one batch of eight maps: binary at the four densities, then K = 5 maps whose foreground fills the same share."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    maps = [(rng.random(shape) < d).astype(np.int64) for d in DENSITIES]
    maps += [np.where(rng.random(shape) < d, rng.integers(1, 5, shape), 0).astype(np.int64) for d in DENSITIES]
    m = np.stack(maps)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _big_map():
    m = (np.random.default_rng(512).random((1, 512, 512)) < 0.6).astype(np.int64)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _big_oracle():
    m = _big_map()
    return _oracle_labels(m, 1), _oracle_keep(m, 2, 1)


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=[f'{h}x{w}' for h, w in SHAPES])
def test_labels_of_random_maps(shape, connectivity):
    maps = _random_maps(shape)
    got = _labels(maps, connectivity)
    assert got.dtype == np.int32 and got.shape == maps.shape
    want = _oracle_labels(maps, connectivity)
    for i in range(len(maps)):
        assert np.array_equal(got[i], want[i]), (shape, connectivity, i, int((got[i] != want[i]).sum()))
    single = _labels(maps[5], connectivity)                      # an (H, W) map gives an (H, W) answer
    assert single.shape == tuple(shape) and np.array_equal(single, want[5])


@pytest.mark.parametrize('connectivity', [1, 2])
def test_components_do_not_leak_between_images(connectivity):
    rng = np.random.default_rng(3)
    maps = rng.integers(0, 5, (3, 37, 53))
    maps[0, -1, :] = 2
    maps[1, 0, :] = 2
    maps[1, -1, :] = 3
    maps[2, 0, :] = 3
    got = _labels(maps, connectivity)
    assert np.array_equal(got, _oracle_labels(maps, connectivity))
    assert got[1, 0, 0] == 0 and got[2, 0, 0] == 0 and got.max() < 37 * 53
    out, stats = _keep(maps, 5, connectivity)
    want, wstats = _oracle_keep(maps, 5, connectivity)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)


def _structured():
    yy, xx = np.mgrid[0:40, 0:44]
    diag = np.zeros((70, 70), np.int64)
    diag[np.arange(70), np.arange(70)] = 1
    return {
        'serpentine': (R.serpentine(67, 130), 2),
        'comb': (R.comb(45, 99), 2),
        'diagonal': (diag, 2),
        'checkerboard': ((1 + (yy + xx) % 2).astype(np.int64), 3),
        'one-class': (np.full((50, 70), 3, np.int64), 4),
        'background': (np.zeros((50, 70), np.int64), 4),
    }


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('name', ['serpentine', 'comb', 'diagonal', 'checkerboard', 'one-class', 'background'])
def test_structured_maps(name, connectivity):
    m, K = _structured()[name]
    lab = _labels(m, connectivity)
    assert np.array_equal(lab, R.canonical_labels(m, connectivity))
    out, stats = _keep(m, K, connectivity)
    want, wstats = R.keep_largest(m, K, connectivity)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    if name == 'serpentine':                                      # one component that crosses every tile border many times
        assert int(m.sum()) == 4453 and (lab[m == 1] == 0).all() and stats.tolist() == [[0, 0], [1, 4453]]
    if name == 'comb':
        assert (lab[m == 1] == 0).all() and stats[1].tolist() == [1, int(m.sum())] and np.array_equal(out, m)
    if name == 'diagonal':
        if connectivity == 1:                                     # all singletons: the tie goes to pixel 0
            assert np.array_equal(lab[m == 1], np.arange(70) * 71) and stats[1].tolist() == [70, 1] and np.flatnonzero(out).tolist() == [0]
        else:
            assert (lab[m == 1] == 0).all() and stats[1].tolist() == [1, 70] and np.array_equal(out, m)
    if name == 'checkerboard':
        if connectivity == 1:
            assert stats.tolist() == [[0, 0], [880, 1], [880, 1]]
            assert np.flatnonzero(out == 1).tolist() == [0] and np.flatnonzero(out == 2).tolist() == [1] and int((out != 0).sum()) == 2
        else:
            assert stats.tolist() == [[0, 0], [1, 880], [1, 880]] and np.array_equal(out, m)
    if name == 'one-class':
        assert (lab == 0).all() and np.array_equal(out, m) and stats.tolist() == [[0, 0], [0, 0], [0, 0], [1, 3500]]
    if name == 'background':
        assert (lab == 0).all() and (out == 0).all() and (stats == 0).all()


def _check_keep(maps, K, c):
    out, stats = _keep(maps, K, c)
    want, wstats = _oracle_keep(maps, K, c)
    assert np.array_equal(out, want), int((out != want).sum())
    assert np.array_equal(stats, wstats)
    assert (out[out != maps] == 0).all()                          # the filter only ever writes background
    again, stats2 = _keep(out, K, c)
    assert np.array_equal(again, out)                             # idempotent
    assert (stats2[..., 0] == (stats[..., 0] > 0)).all() and np.array_equal(stats2[..., 1], stats[..., 1])
    for inplace in (False, True):
        raw, rstats = _keep_raw(maps, K, c, inplace)
        assert np.array_equal(raw, want) and np.array_equal(rstats, wstats), inplace
    return out, stats


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('K', [2, 5, 32])
@pytest.mark.parametrize('shape', [(37, 53), (130, 67)], ids=['37x53', '130x67'])
def test_keep_largest_on_uniform_noise(shape, K, connectivity):
    rng = np.random.default_rng(K * 100 + shape[0])
    maps = rng.integers(0, K, (2,) + shape)
    out, stats = _check_keep(maps, K, connectivity)
    assert (stats[:, 1:, 0] >= 1).all()
    if K == 5 and shape == (37, 53) and connectivity == 1:        # hundreds of small components per class: size ties occur
        assert (stats[:, 1:, 0] > 150).all() and (stats[:, 1:, 1] < 20).all()
        ties = 0
        for n in range(2):
            lab = R.canonical_labels(maps[n], 1)
            for k in range(1, K):
                sizes = np.unique(lab[maps[n] == k], return_counts=True)[1]
                ties += (sizes == sizes.max()).sum() > 1
        assert ties >= 1


def test_keep_largest_on_a_native_size_batch():
    rng = np.random.default_rng(11)
    maps = np.where(rng.random((2, 256, 272)) < 0.62, rng.integers(1, 4, (2, 256, 272)), 0)
    maps[1] = (rng.random((256, 272)) < 0.6) * 3                  # one class at the percolation threshold
    _check_keep(maps, 4, 1)
    out, stats = _keep(maps, 4, 2)
    want, wstats = _oracle_keep(maps, 4, 2)
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)


def test_large_map_and_determinism():
    m = _big_map()
    want_lab, (want_out, want_stats) = _big_oracle()
    runs = []
    for _ in range(2):
        lab = _labels(m, 1)
        out, stats = _keep_raw(m, 2, 1, False)
        runs.append((lab, out, stats))
    assert np.array_equal(runs[0][0], want_lab) and np.array_equal(runs[0][1], want_out) and np.array_equal(runs[0][2], want_stats)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    assert want_stats[0, 1, 0] > 1000 and want_stats[0, 1, 1] > 10000          # thousands of clusters, one of them winding far


@pytest.mark.parametrize('connectivity', [1, 2])
def test_values_outside_the_class_range_are_copied(connectivity):
    rng = np.random.default_rng(5)
    K = 4
    maps = rng.integers(0, K, (2, 37, 53))
    odd = rng.random(maps.shape) < 0.1
    maps[odd] = rng.choice([K, K + 3, -1, 2 ** 40, -2 ** 40], int(odd.sum()))
    out, stats = _keep(maps, K, connectivity)
    assert np.array_equal(out[odd], maps[odd])
    want, wstats = _oracle_keep(maps, K, connectivity)            # the oracle looks at classes 1 .. K-1 only and copies the rest
    assert np.array_equal(out, want) and np.array_equal(stats, wstats)
    assert np.array_equal(_labels(maps, connectivity), _oracle_labels(maps, connectivity))     # labelled like any value
    small = _gpu(rng.integers(0, 3, (9, 11)).astype(np.uint8))    # other integer dtypes come back as they went in
    from pacingpseudo_amd.utils import keep_largest_components
    got = keep_largest_components(small, 3, connectivity)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.keep_largest(small.cpu().numpy(), 3, connectivity)[0])


def test_inference_driver_with_the_filter(tmp_path):
    """inference.py --keep_largest_cc end to end: a random-weight checkpoint (noisy predictions, many components), the rows of
    eval_data.npz against the per-sample path -- the network's arg-max, the scipy oracle, compute_95hd and the Dice formula."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.utils.metrics import compute_95hd
    from tests.test_gpu_step import build_model
    args = O.full_flags(epoch=2, num_classes=4, ignored_index=4, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    model = build_model(args, {k: v.numpy() for k, v in O.init_state(args, seed=3).items()})
    ck = tmp_path / 'run-fold0'
    (ck / 'ckps').mkdir(parents=True)
    torch.save(model.state_dict(), ck / 'ckps' / 'ckp_399.pth')
    common = ['--fold', '0', '--checkpoint_file', str(ck), '--dataset', 'acdc', '--synthetic', '6', '--image_size', '64', '--batch_size', '4',
              '--num_workers', '0', '--init_ch', '8', '--max_ch', '64']
    dicearr, hd95arr = I.main(common + ['--root', str(tmp_path / 'on'), '--keep_largest_cc'])
    out = tmp_path / 'on' / 'Inference' / 'acdc' / 'run-fold0'
    z = np.load(out / 'eval_data.npz')
    assert sorted(z.files) == ['dicearr', 'hd95arr', 'ncomp', 'removed']
    assert z['dicearr'].shape == (6, 4) and z['hd95arr'].shape == (6, 4) and z['ncomp'].shape == (6, 4) and z['removed'].shape == (6,)
    assert z['ncomp'].dtype == np.int32 and np.array_equal(z['dicearr'], dicearr, equal_nan=True)
    log = (out / 'log.txt').read_text()
    assert f'{int(z["removed"].sum())} pixels set to background, {int((z["removed"] > 0).sum())} of 6 slices changed' in log
    net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=4, output_stride=8).cuda()
    I.load_backbone(net, torch.load(ck / 'ckps' / 'ckp_399.pth'))
    net.eval()
    ds = SyntheticPhantoms(6, 4, size=64, train=False, seed=1)
    removed_ref = []
    for i in range(6):
        b = ds[i]
        with torch.no_grad():
            pred = net(b['image'][None].cuda())['segmentation/logits'].argmax(1)[0].cpu().numpy()
        filt, stats = R.keep_largest(pred, 4, 1)
        removed_ref.append(int((filt != pred).sum()))
        if i not in (0, 5):
            continue
        lab = b['label'].argmax(0).numpy()
        assert np.array_equal(z['ncomp'][i], stats[:, 0]) and int(z['removed'][i]) == removed_ref[-1]
        want = compute_95hd(filt, lab, 4, I.SPACING['acdc'])
        np.testing.assert_allclose(z['hd95arr'][i], np.array(want, np.float32), rtol=1e-6, equal_nan=True)
        for k in range(4):
            p, t = filt == k, lab == k
            d = np.nan if not p.any() and not t.any() else 2 * (p & t).sum() / max(p.sum() + t.sum(), 1e-8)
            np.testing.assert_allclose(z['dicearr'][i, k], np.float32(d), rtol=1e-6, equal_nan=True)
    assert max(removed_ref) > 0, 'the reference path removes nothing: the comparison above proves nothing'
    assert z['removed'].tolist() == removed_ref
    # the same command without the flag: exactly today's keys, and no line about the filter
    I.main(common + ['--root', str(tmp_path / 'off')])
    off = tmp_path / 'off' / 'Inference' / 'acdc' / 'run-fold0'
    assert sorted(np.load(off / 'eval_data.npz').files) == ['dicearr', 'hd95arr']
    assert 'Largest-component' not in (off / 'log.txt').read_text()
