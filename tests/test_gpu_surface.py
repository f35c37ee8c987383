"""pp_surface_reduce and the surface metrics built on it (HD, percentile distance, ASSD, surface Dice) on the GPU: the raw entry
point against numpy.sort on synthetic bit patterns (equalities), the Python layer and the inference driver against the float64
scipy oracle of tests/_surface_reference.py at the tolerance the device distances are already held to (rtol 1e-6)."""
import functools

import numpy as np
import pytest
import torch

from tests import _surface_reference as R

pytestmark = pytest.mark.gpu

CAP = 5000
PAIRS = [(1, 1), (1, 0), (0, 0), (2, 3), (255, 1), (256, 256), (257, 300), (1000, 0), (5000, 5000), (4999, 1), (21, 0), (300, 200)]
EQUAL_ITEM = 11                                                   # its 500 values are all the same


def _gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _synthetic():
    """dist [12][2][CAP] as bytes 0xFF (NaN) with live prefixes of uniformly random bit patterns from {0} + every normal
    magnitude, counts [12][4] (the last two columns are never read by the reduction), and a tolerance drawn from the data."""
    rng = np.random.default_rng(2024)
    bits = np.full((len(PAIRS), 2, CAP), 0xFFFFFFFF, np.uint32)
    for i, (na, nb) in enumerate(PAIRS):
        for s, m in enumerate((na, nb)):
            u = rng.integers(0x00800000, 0x7F7FFFFF, m, endpoint=True, dtype=np.uint32)
            u[rng.random(m) < 0.02] = 0
            if i == EQUAL_ITEM:
                u[:] = 0x40490FDB
            bits[i, s, :m] = u
    bits[4, 0, :255:7] = bits[4, 0, 3]                              # repeated values inside random sets as well
    bits[8, 1, :5000:3] = bits[8, 0, 17]
    dist = bits.view(np.float32)
    counts = np.array([[na, nb, -12345, 1 << 30] for na, nb in PAIRS], np.int32)
    tolerance = float(dist[8, 0, 2500])                           # an element: `<=` has to count it
    assert np.isnan(dist[0, 0, 1]) and np.isfinite(tolerance) and tolerance > 0
    return dist, counts, tolerance


def _reduce(dist, counts, cap, percentile, tolerance, rows_behind=1):
    from pacingpseudo_amd._lib import lib, stream_ptr
    items = counts.shape[0]
    d, c = _gpu(dist), _gpu(counts)
    out = torch.full((items + rows_behind, 8), -7.0, device='cuda', dtype=torch.float64)
    lib.pp_surface_reduce(d.data_ptr(), c.data_ptr(), items, cap, percentile, tolerance, out.data_ptr(), stream_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize('percentile', [50.0, 95.0, 100.0])
def test_entry_point_on_random_bit_patterns(percentile):
    dist, counts, tolerance = _synthetic()
    got = _reduce(dist, counts, CAP, percentile, tolerance)
    assert np.array_equal(got[len(PAIRS)], np.full(8, -7.0)), 'written behind out[items][8]'
    for i, (na, nb) in enumerate(PAIRS):
        a, b = dist[i, 0, :na], dist[i, 1, :nb]
        want = R.reduce_row(a, b, np.float32(tolerance), percentile)
        print(i, (na, nb), got[i].tolist())
        if na + nb == 0:
            assert np.array_equal(got[i], np.zeros(8)), i
            continue
        for col in (0, 3, 4, 5, 6, 7):                           # maximum, counts, order statistics, n: equalities
            assert got[i, col] == want[col], (i, col, got[i, col], want[col])
        n = na + nb
        for col in (1, 2):                                        # n non-negative terms added in double
            assert abs(got[i, col] - want[col]) <= n * 2.0 ** -52 * want[col], (i, col, got[i, col], want[col])
    assert got[8, 3] > 0 and got[8, 3] < 5000                     # the tolerance splits the largest item
    if percentile == 100.0:
        assert np.array_equal(got[:-1, 5], got[:-1, 0]) and np.array_equal(got[:-1, 6], got[:-1, 0])


def test_entry_point_reads_no_more_than_the_capacity_and_repeats_itself():
    """Counts above cap are clamped (the distance kernel writes no more than cap entries either), and a second call gives the
    same bits."""
    dist, counts, tolerance = _synthetic()
    big = counts.copy()
    big[8, :2] = (CAP + 77, 1 << 30)
    got = _reduce(dist, big, CAP, 95.0, tolerance)
    ref = _reduce(dist, counts, CAP, 95.0, tolerance)
    assert np.array_equal(got, ref) and np.array_equal(_reduce(dist, counts, CAP, 95.0, tolerance), ref)


def _metrics(pred, label, K, spacing, **kw):
    from pacingpseudo_amd.utils import batch_surface_metrics
    return batch_surface_metrics(_gpu(pred), _gpu(label), K, spacing, **kw)


def _assert_matches(got, want, where):
    for k in R.KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (where, k)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (where, k)
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, atol=0, equal_nan=True, err_msg=f'{where} {k}')


def test_duplicates():
    yy, xx = np.mgrid[0:40, 0:44]
    label = np.zeros((40, 44), np.int64)
    label[(yy - 14) ** 2 + (xx - 15) ** 2 < 100] = 1
    label[8:30, 28:40] = 2
    got = _metrics(label[None], label[None], 3, (1.51, 1.51))
    for k in ('hd', 'hdp', 'assd'):
        assert np.array_equal(got[k], np.zeros((1, 3))), k           # every distance is 0, exactly
    assert np.array_equal(got['nsd'], np.ones((1, 3)))
    pred = np.roll(label, 1, axis=1)                                # one pixel to the right: long runs of equal distances
    for spacing in R.SPACINGS:
        want = R.batch_surface_metrics(pred[None], label[None], 3, spacing)
        d1, d2 = R.directed_sets(pred == 2, label == 2, spacing)
        values, ties = np.unique(np.hstack((d1, d2)), return_counts=True)
        assert ties.max() > 20 and ties.sum() > 3 * len(values)      # a few values, each many times
        _assert_matches(_metrics(pred[None], label[None], 3, spacing), want, spacing)
    got = _metrics(pred[None], label[None], 3, (1.0, 1.0), tolerance=1.0)
    assert got['hd'][0, 2] == 1.0 and got['hdp'][0, 2] == 1.0 and got['nsd'][0, 2] == 1.0      # the exact hit counts as inside
    assert _metrics(pred[None], label[None], 3, (1.0, 1.0), tolerance=0.5)['nsd'][0, 2] < 1.0


@functools.lru_cache(maxsize=None)
def _oracle(shape, spacing):
    pred, label = R.seeded_maps(shape)
    return R.batch_surface_metrics(pred, label, 5, spacing)         # asserts that 2.0 mm is clear of every distance


def test_the_seeded_maps_are_mostly_scored():
    """The condition of the end-to-end comparison: at most one third of the (map, class) items are NaN, every shape has a finite one."""
    nan = total = 0
    for shape in R.SHAPES:
        hd = _oracle(shape, R.SPACINGS[0])['hd']
        assert np.isfinite(hd).any(), shape
        nan += int(np.isnan(hd).sum())
        total += hd.size
    assert total == 120 and 3 * nan <= total, (nan, total)


@pytest.mark.parametrize('spacing', R.SPACINGS)
@pytest.mark.parametrize('shape', R.SHAPES)
def test_against_the_oracle(shape, spacing):
    pred, label = R.seeded_maps(shape)
    _assert_matches(_metrics(pred, label, 5, spacing), _oracle(shape, spacing), (shape, spacing))


def test_single_pixel_map_is_all_nan():
    got = _metrics(np.zeros((2, 1, 1), np.int64), np.array([[[0]], [[3]]]), 5, (1.0, 1.0))
    assert all(got[k].shape == (2, 5) and np.isnan(got[k]).all() for k in R.KEYS)


def test_large_noise_pair_and_determinism():
    """256 x 256 uniform noise at K = 2: about 32,000 surface pixels per mask, so more than 6 x 10^4 distances per item, the
    order of the worst case -- every thread of the block walks hundreds of elements in each pass."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    rng = np.random.default_rng(77)
    pred, label = rng.integers(0, 2, (1, 256, 256)), rng.integers(0, 2, (1, 256, 256))
    want = R.batch_surface_metrics(pred, label, 2, (1.51, 1.51))
    _assert_matches(_metrics(pred, label, 2, (1.51, 1.51)), want, 'noise 256')
    p, t = _gpu(pred), _gpu(label)
    dist = torch.empty((2, 2, 65536), device='cuda', dtype=torch.float32)
    counts = torch.empty((2, 4), device='cuda', dtype=torch.int32)
    nws = lib.pp_hd95_workspace(1, 2, 256, 256)
    ws = torch.empty(nws, device='cuda', dtype=torch.uint8)
    lib.pp_hd95_surface_distances(p.data_ptr(), t.data_ptr(), 1, 2, 256, 256, 1.51, 1.51, dist.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                  nws, stream_ptr())
    outs = []
    for _ in range(2):
        out = torch.full((2, 8), -7.0, device='cuda', dtype=torch.float64)
        lib.pp_surface_reduce(dist.data_ptr(), counts.data_ptr(), 2, 65536, 95.0, 2.0, out.data_ptr(), stream_ptr())
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    assert (outs[0][:, 7] > 50000).all()                           # the sizes the test is about
    d, c = dist.cpu().numpy(), counts.cpu().numpy()
    for i in range(2):
        want_row = R.reduce_row(d[i, 0, :c[i, 0]], d[i, 1, :c[i, 1]], np.float32(2.0), 95.0)
        assert np.array_equal(outs[0][i, [0, 3, 4, 5, 6, 7]], want_row[[0, 3, 4, 5, 6, 7]]), i


def test_distance_sets_come_in_row_major_order():
    """pp_hd95_surface_distances lists each surface in row-major pixel order (an ordered compaction, no append through a counter):
    dist[item][d][:counts] equals, ELEMENT BY ELEMENT, the reference's sets, which scipy's boolean indexing yields in row-major
    order.  pp_surface_reduce adds the distances in storage order; its promise of the same bits in every run rests on this.
    37 x 53 = 1961 pixels: eight trips of the 256-thread block, every wave contributes."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    N, K, H, W, spacing = 4, 3, 37, 53, (1.5, 0.75)
    pred, label = R.seeded_maps((H, W), K)
    p, t = _gpu(pred), _gpu(label)
    dist = torch.zeros((N * K, 2, H * W), device='cuda', dtype=torch.float32)
    counts = torch.empty((N * K, 4), device='cuda', dtype=torch.int32)
    nws = lib.pp_hd95_workspace(N, K, H, W)
    ws = torch.empty(nws, device='cuda', dtype=torch.uint8)
    lib.pp_hd95_surface_distances(p.data_ptr(), t.data_ptr(), N, K, H, W, *spacing, dist.data_ptr(), counts.data_ptr(), ws.data_ptr(), nws,
                                  stream_ptr())
    d, c = dist.cpu().numpy(), counts.cpu().numpy()
    compared = telling = 0
    for n in range(N):
        for k in range(K):
            a, b = np.asarray(pred[n]) == k, np.asarray(label[n]) == k
            if not (a.any() and b.any()):
                continue
            d1, d2 = R.directed_sets(a, b, spacing)
            i = n * K + k
            assert c[i, 0] == len(d1) and c[i, 1] == len(d2), (n, k)
            np.testing.assert_allclose(d[i, 0, :len(d1)], d1, rtol=1e-6, atol=0, err_msg=f'image {n} class {k}: pred -> label')
            np.testing.assert_allclose(d[i, 1, :len(d2)], d2, rtol=1e-6, atol=0, err_msg=f'image {n} class {k}: label -> pred')
            compared += len(d1) + len(d2)
            telling += len(np.unique(d1)) > 3 and len(np.unique(d2)) > 3          # (a set of equal distances does not tell the order)
    assert compared > 500 and telling >= 4


def test_compute_hd_equals_the_oracle():
    from pacingpseudo_amd.utils import compute_hd
    pred, label = R.seeded_maps((37, 53))
    pred, label = pred[1].copy(), label[1].copy()
    pred[pred == 3] = 0                                             # a class the prediction lacks: NaN
    got = compute_hd(pred, label, 5, (1.51, 1.51))
    want = R.surface_metrics(pred, label, 5, (1.51, 1.51))['hd']
    assert isinstance(got, list) and len(got) == 5 and np.isnan(got[3]) and np.isfinite(want[[0, 1, 2, 4]]).all()
    np.testing.assert_allclose(np.array(got), want, rtol=1e-6, atol=0, equal_nan=True)


def test_inference_driver_with_surface_metrics(tmp_path):
    """inference.py --surface_metrics end to end on a random-weight checkpoint: the rows of eval_data.npz against the oracle on the
    network's own arg-max; without the flag exactly the keys and the Dice values there were before."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.models import UNet
    from tests.test_gpu_step import build_model
    args = O.full_flags(epoch=2, num_classes=4, ignored_index=4, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    model = build_model(args, {k: v.numpy() for k, v in O.init_state(args, seed=3).items()})
    ck = tmp_path / 'run-fold0'
    (ck / 'ckps').mkdir(parents=True)
    torch.save(model.state_dict(), ck / 'ckps' / 'ckp_399.pth')
    common = ['--fold', '0', '--checkpoint_file', str(ck), '--dataset', 'acdc', '--synthetic', '6', '--image_size', '64', '--batch_size', '4',
              '--num_workers', '0', '--init_ch', '8', '--max_ch', '64']
    dicearr, hd95arr = I.main(common + ['--root', str(tmp_path / 'on'), '--surface_metrics', '--nsd_tolerance', '2.0'])
    out = tmp_path / 'on' / 'Inference' / 'acdc' / 'run-fold0'
    z = np.load(out / 'eval_data.npz')
    keys = ['assdarr', 'dicearr', 'hd95arr', 'hdarr', 'nsdarr']
    assert sorted(z.files) == keys
    assert all(z[k].shape == (6, 4) and z[k].dtype == np.float32 for k in keys)
    assert np.array_equal(z['hd95arr'], hd95arr, equal_nan=True)
    log = (out / 'log.txt').read_text()
    assert 'overall HD: ' in log and 'overall ASSD: ' in log and 'overall NSD at 2 mm: ' in log and 'surface_metrics=True' in log
    net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=4, output_stride=8).cuda()
    I.load_backbone(net, torch.load(ck / 'ckps' / 'ckp_399.pth'))
    net.eval()
    ds = SyntheticPhantoms(6, 4, size=64, train=False, seed=1)
    finite = 0
    for i in range(6):
        b = ds[i]
        with torch.no_grad():
            pred = net(b['image'][None].cuda())['segmentation/logits'].argmax(1)[0].cpu().numpy()
        want = R.surface_metrics(pred, b['label'].argmax(0).numpy(), 4, I.SPACING['acdc'], tolerance=2.0)
        for key, name in (('hd', 'hdarr'), ('hdp', 'hd95arr'), ('assd', 'assdarr'), ('nsd', 'nsdarr')):
            np.testing.assert_allclose(z[name][i], want[key].astype(np.float32), rtol=1e-6, atol=0, equal_nan=True, err_msg=f'{name}[{i}]')
        finite += int(np.isfinite(want['hd']).sum())
    assert finite >= 6, 'hardly any class was scored: the comparison above proves nothing'
    # the same command without the flag: exactly today's keys, the same Dice, no word of the new metrics in the log
    off_dice, off_hd95 = I.main(common + ['--root', str(tmp_path / 'off')])
    off = tmp_path / 'off' / 'Inference' / 'acdc' / 'run-fold0'
    assert sorted(np.load(off / 'eval_data.npz').files) == ['dicearr', 'hd95arr']
    assert np.array_equal(off_dice, dicearr, equal_nan=True) and np.array_equal(np.load(off / 'eval_data.npz')['dicearr'], z['dicearr'], equal_nan=True)
    np.testing.assert_allclose(off_hd95, hd95arr, rtol=1e-6, atol=0, equal_nan=True)      # batch_hd95 against the device reduction
    off_log = (off / 'log.txt').read_text()
    assert 'overall HD:' not in off_log and 'surface_metrics' not in off_log and 'nsd_tolerance' not in off_log
    # composed with the component filter and test-time augmentation
    I.main(common + ['--root', str(tmp_path / 'all'), '--surface_metrics', '--keep_largest_cc', '--tta', 'flips'])
    za = np.load(tmp_path / 'all' / 'Inference' / 'acdc' / 'run-fold0' / 'eval_data.npz')
    assert sorted(za.files) == sorted(keys + ['ncomp', 'removed', 'tta_changed'])
    assert all(za[k].shape == (6, 4) for k in keys + ['ncomp']) and za['removed'].shape == (6,) and za['tta_changed'].shape == (6,)
