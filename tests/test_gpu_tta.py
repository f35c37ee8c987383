"""Test-time augmentation on the GPU against the fp64 definition in tests/_tta_reference.py: view geometry bit for bit, the
inverse mapping of the accumulate kernel by exact counting, values, determinism, the path through a U-Net, the group property
and inference.evaluate."""
import functools

import numpy as np
import pytest
import torch

from tests import _tta_reference as R

pytestmark = pytest.mark.gpu

MODES = {'none': (0,), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}
VIEW_SHAPES = [(1, 1), (1, 130), (5, 3), (37, 53), (32, 32), (33, 64), (64, 96)]   # one element / row, partial and exact tiles, W % 4 != 0


def _gpu(a, dtype=np.float32):
    return torch.as_tensor(np.array(a, dtype=dtype, order='C', copy=True)).cuda()


def _torch_view(t, op):
    """The composition the kernel replaces."""
    if op & 4:
        t = t.transpose(-1, -2)
    if op & 2:
        t = t.flip(-2)
    if op & 1:
        t = t.flip(-1)
    return t.contiguous()


def _mean_raw(view_logits, ops, shape, poison=False, want_cls=True):
    """pp_tta_accumulate per view + pp_tta_finalize on the C entry points themselves -> (prob, cls) as numpy.  poison: acc starts
    as NaN (the first view must store, not add), cls as -7."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    N, K, H, W = shape
    acc = torch.full(shape, float('nan'), device='cuda') if poison else torch.empty(shape, device='cuda')
    cls = torch.full((N, H, W), -7, device='cuda', dtype=torch.int64)
    for v, (z, op) in enumerate(zip(view_logits, ops)):
        assert tuple(z.shape) == ((N, K, W, H) if op & 4 else (N, K, H, W)) and z.is_contiguous()
        lib.pp_tta_accumulate(z.data_ptr(), N, K, H, W, op, int(v == 0), acc.data_ptr(), stream_ptr())
    lib.pp_tta_finalize(acc.data_ptr(), N, K, H, W, len(ops), cls.data_ptr() if want_cls else None, stream_ptr())
    return acc.cpu().numpy(), cls.cpu().numpy()


# ---- 1. view geometry ----
@pytest.mark.parametrize('shape', VIEW_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_view_equals_the_torch_composition_bitwise(shape):
    from pacingpseudo_amd.utils import tta_view
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    for planes in (1, 6):
        x = _gpu(rng.standard_normal((planes, 1, H, W)))
        y = _gpu(rng.standard_normal((1, planes, H, W)))
        for op in range(8):
            for t in (x, y):                                          # planes = N * C either way
                got = tta_view(t, op)
                want = _torch_view(t, op)
                assert got.shape == want.shape, (op, planes)
                assert torch.equal(got, want), (op, planes)
                assert np.array_equal(got.cpu().numpy(), R.view(t.cpu().numpy(), op)), (op, planes)


def test_view_scalar_path_for_an_unaligned_pointer():
    """W % 4 == 0 but the planes start 4 bytes off a 16-byte boundary: the 16-byte path must not be taken."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    H, W = 6, 8
    rng = np.random.default_rng(5)
    buf = _gpu(rng.standard_normal(2 * H * W + 1))
    x = buf[1:]
    out = torch.empty(2 * H * W + 1, device='cuda')[1:]
    assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    for op in (1, 3):
        lib.pp_tta_view(x.data_ptr(), 2, H, W, op, out.data_ptr(), stream_ptr())
        assert torch.equal(out.view(2, H, W), _torch_view(x.view(2, H, W), op)), op


# ---- 2. accumulate geometry, exact ----
@pytest.mark.parametrize('shape', [(37, 53), (40, 72), (1, 130)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('mode', ['none', 'flips', 'd4'])
def test_accumulate_puts_every_view_back_exactly(mode, shape):
    """One random class map per view in the un-viewed frame, fed as the view of 40 * one-hot: fp32 soft-max of such logits is 1
    and ~ 4e-18, so the mean probability of class k is #{v: c_v = k} / V; a wrong inverse mapping is off by at least 1/8."""
    ops = MODES[mode]
    H, W = shape
    N = 2
    rng = np.random.default_rng(7 * H + W + len(ops))
    for K in (1, 2, 5, 17, 32):
        maps = [rng.integers(0, K, (N, H, W)) for _ in ops]
        onehot = [np.moveaxis(np.eye(K, dtype=np.float32)[c], -1, 1) for c in maps]         # (N, K, H, W)
        logits = [_gpu(R.view(40.0 * o, op)) for o, op in zip(onehot, ops)]
        prob, cls = _mean_raw(logits, ops, (N, K, H, W), poison=True)
        want = sum(o.astype(np.float64) for o in onehot) / len(ops)
        err = np.abs(prob.astype(np.float64) - want).max()
        print(f'{mode} {shape} K={K}: max |prob - count / V| = {err:.3e}')
        assert err <= 1e-12, (K, err)
        assert np.array_equal(cls, prob.argmax(1)), K


# ---- 3. values, 4. determinism ----
@functools.lru_cache(maxsize=None)
def _random_case(mode, shape, K):
    """-> (per-view logits as numpy fp32, oracle prob fp64): N(0, 3^2) clipped to +-8, N = 2."""
    ops = MODES[mode]
    H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * W + K + len(ops))
    logits = [np.clip(rng.normal(0.0, 3.0, (2, K) + ((W, H) if op & 4 else (H, W))), -8, 8).astype(np.float32) for op in ops]
    prob, _ = R.tta_mean(logits, ops)
    return logits, prob


@pytest.mark.parametrize('shape', [(37, 53), (64, 64)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('mode', ['flips', 'd4'])
def test_values_against_the_fp64_mean(mode, shape):
    """|prob - oracle| <= 1e-5: logit differences up to 16 give a relative error of about 16 * 2^-24 * 2 ~ 2e-6 through an
    exp2-based exponential on values <= 1; seven fp32 additions of values <= 1 and an exact scaling add < 1e-6."""
    ops = MODES[mode]
    H, W = shape
    for K in (2, 5, 9, 32):
        logits, oracle = _random_case(mode, shape, K)
        dev = [_gpu(z) for z in logits]
        prob, cls = _mean_raw(dev, ops, (2, K, H, W), poison=True)
        err = np.abs(prob.astype(np.float64) - oracle).max()
        print(f'{mode} {shape} K={K}: max |prob - oracle| = {err:.3e}')
        assert err <= 1e-5, (K, err)
        assert np.array_equal(cls, prob.argmax(1)), K                 # the kernel's own definition: no tie exclusions
        assert np.abs(prob.sum(1, dtype=np.float64) - 1.0).max() <= 1e-5
        again, cls2 = _mean_raw(dev, ops, (2, K, H, W))
        assert np.array_equal(again.view(np.uint32), prob.view(np.uint32)) and np.array_equal(cls2, cls), K      # the same bits
        nocls, untouched = _mean_raw(dev, ops, (2, K, H, W), want_cls=False)
        assert np.array_equal(nocls.view(np.uint32), prob.view(np.uint32)) and (untouched == -7).all(), K        # cls may be null


def test_predict_from_recorded_logits_and_its_checks():
    """tta_predict with a `forward` that replays recorded logits: the wrapper gives what the entry points give, runs the views
    in ascending order on the views of the image, and refuses a forward whose output does not fit the view."""
    from pacingpseudo_amd.utils import tta_predict, tta_view
    logits, oracle = _random_case('d4', (37, 53), 5)
    image = _gpu(np.random.default_rng(9).standard_normal((2, 3, 37, 53)))
    seen = []

    def forward(x):
        op = len(seen)
        assert torch.equal(x, _torch_view(image, op))
        seen.append(tuple(x.shape))
        return _gpu(logits[op])
    prob, cls = tta_predict(forward, image, 'd4')
    assert len(seen) == 8 and prob.dtype == torch.float32 and cls.dtype == torch.int64
    assert tuple(prob.shape) == (2, 5, 37, 53) and tuple(cls.shape) == (2, 37, 53)
    raw, raw_cls = _mean_raw([_gpu(z) for z in logits], MODES['d4'], (2, 5, 37, 53))
    assert np.array_equal(prob.cpu().numpy().view(np.uint32), raw.view(np.uint32)) and np.array_equal(cls.cpu().numpy(), raw_cls)
    assert np.abs(prob.cpu().numpy() - oracle).max() <= 1e-5
    only = tta_predict(lambda x: _gpu(logits[0]), image, 'none', return_class=False)
    assert torch.is_tensor(only) and np.abs(only.cpu().numpy() - R.softmax(logits[0])).max() <= 1e-5
    with pytest.raises(ValueError, match='forward returned'):
        tta_predict(lambda x: _gpu(logits[0]), image, 'd4')             # the transposed views must come back 53 x 37
    with pytest.raises(ValueError, match='CUDA'):
        tta_predict(lambda x: torch.zeros(2, 5, 37, 53), image, 'flips')
    with pytest.raises(ValueError, match='K = 33'):
        tta_predict(lambda x: torch.zeros(2, 33, 37, 53, device='cuda'), image, 'flips')
    assert tuple(tta_view(image, 6).shape) == (2, 3, 53, 37)


# ---- 5. through a model, 6. group property ----
@functools.lru_cache(maxsize=None)
def _net():
    """A tiny U-Net with random weights in eval mode, its input batch (3 slices of 40 x 72) and a forward that returns a copy
    of the logits (the engine may reuse its output buffer)."""
    from pacingpseudo_amd.models import UNet
    torch.manual_seed(11)
    net = UNet(input_ch=1, init_ch=4, max_ch=32, num_classes=5, output_stride=8).cuda()
    net.eval()
    x = _gpu(np.random.default_rng(12).standard_normal((3, 1, 40, 72)))

    def forward(t):
        with torch.no_grad():
            return net(t)['segmentation/logits'].clone()
    return net, x, forward


@functools.lru_cache(maxsize=None)
def _net_prediction(mode):
    from pacingpseudo_amd.utils import tta_predict
    _, x, forward = _net()
    prob, cls = tta_predict(forward, x, mode)
    return prob.cpu().numpy(), cls.cpu().numpy()


@pytest.mark.parametrize('mode', ['flips', 'd4'])
def test_through_a_model(mode):
    from pacingpseudo_amd.utils import tta_view
    _, x, forward = _net()
    ops = MODES[mode]
    per_view = [forward(x if op == 0 else tta_view(x, op)).cpu().numpy() for op in ops]     # the model's own logits: conv numerics cancel
    oracle, _ = R.tta_mean(per_view, ops)
    prob, cls = _net_prediction(mode)
    err = np.abs(prob - oracle).max()
    print(f'{mode}: max |tta_predict - tta_mean(model logits)| = {err:.3e}')
    assert err <= 1e-5
    assert np.array_equal(cls, prob.argmax(1))


def test_mode_none_is_the_softmax_of_one_forward_pass():
    _, x, forward = _net()
    z = forward(x).cpu().numpy()
    prob, cls = _net_prediction('none')
    assert np.abs(prob - R.softmax(z)).max() <= 1e-5
    assert np.array_equal(cls, z.argmax(1))                             # the model's first-maximum arg-max


@pytest.mark.parametrize('mode', ['flips', 'd4'])
def test_group_property(mode):
    """tta_predict(view_g(x)) = view_g(tta_predict(x)) for every g of the mode's group: the same eight (four) network inputs
    occur on both sides, only the order of the fp32 additions differs: 2 * 7 * 2^-24 < 2e-6."""
    from pacingpseudo_amd.utils import tta_predict, tta_view
    _, x, forward = _net()
    prob, _ = _net_prediction(mode)
    for g in MODES[mode]:
        got = tta_predict(forward, x if g == 0 else tta_view(x, g), mode, return_class=False).cpu().numpy()
        err = np.abs(got - R.view(prob, g)).max()
        print(f'{mode} g={g}: max |predict(view_g x) - view_g predict(x)| = {err:.3e}')
        assert err <= 2e-6, (g, err)


# ---- 7. evaluate ----
def test_evaluate_with_tta():
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms, collate_by_shape, expand_compact
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.utils import tta_predict
    from pacingpseudo_amd.utils.metrics import batch_dice_counts
    K = 4
    torch.manual_seed(21)
    net = UNet(input_ch=1, init_ch=4, max_ch=32, num_classes=K, output_stride=8).cuda()
    device = torch.device('cuda', 0)
    ds = SyntheticPhantoms(6, K, size=64, train=False, seed=1, native=True, compact=True)

    def loader():
        return torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate_by_shape)
    spacing = I.SPACING['acdc']
    plain = I.evaluate(net, loader(), K, spacing, device)
    none = I.evaluate(net, loader(), K, spacing, device, tta='none', extra=(extra_none := {}))
    assert len(plain) == len(none) == 2 and extra_none == {}
    for a, b in zip(plain, none):
        assert a.dtype == b.dtype and a.shape == b.shape == (6, K)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))    # bit-identical, NaN included
    extra = {}
    dice, hd = I.evaluate(net, loader(), K, spacing, device, tta='d4', extra=extra)
    assert dice.shape == hd.shape == (6, K) and dice.dtype == hd.dtype == np.float32
    assert sorted(extra) == ['tta_changed'] and extra['tta_changed'].shape == (6,) and extra['tta_changed'].dtype == np.int64
    assert (extra['tta_changed'] >= 0).all() and (extra['tta_changed'] <= 64 * 64).all()
    rows, changed = [], []
    net.eval()
    for groups in loader():
        for batch in (groups if isinstance(groups, list) else [groups]):
            batch = expand_compact(batch, K, device)
            with torch.no_grad():
                prob, cls = tta_predict(lambda t: net(t)['segmentation/logits'], batch['image'], 'd4')
                changed.extend((cls != net(batch['image'])['segmentation/logits'].argmax(1)).flatten(1).sum(1).tolist())
            c = batch_dice_counts(prob, batch['label'])
            inter, ps, ts = c[..., 0], c[..., 1], c[..., 2]
            with np.errstate(invalid='ignore', divide='ignore'):
                d = 2.0 * inter / np.maximum(ps + ts, 1e-8)
            d[(ps == 0) & (ts == 0)] = np.nan
            rows.extend(d.tolist())
    assert np.array_equal(dice, np.array(rows, np.float32), equal_nan=True)
    assert np.array_equal(extra['tta_changed'], np.array(changed, np.int64))
    extra = {}
    out = I.evaluate(net, loader(), K, spacing, device, keep_largest_cc=True, tta='flips', extra=extra)
    assert len(out) == 4
    dice, hd, ncomp, removed = out
    assert dice.shape == hd.shape == ncomp.shape == (6, K) and removed.shape == (6,) and extra['tta_changed'].shape == (6,)
    assert ncomp.dtype == np.int32 and removed.dtype == np.int64
