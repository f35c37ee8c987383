"""Mean-field CRF refinement on the GPU against the float64 definition in tests/_crf_refine_reference.py: values and class maps
at T = 1 and T = 5 on ten shapes, structure (row sums, zero weights, determinism, batch independence, ping-pong parity, a null
class map, refusals that leave the outputs untouched) and the path through inference.evaluate.

Tolerance of the values: max |prob - prob64| <= 1e-5.  A float32 restatement of the same formulas on the CPU differs from float64
by at most 7.6e-7 over the ten shapes with T up to 10 (7.0e-7 on the inputs below with T = 1 .. 5; the test recomputes it and
prints it per case), so the bound is 13 times the format's own error; the margin is for the device's exp / exp2 and the other
summation order of the window walk.  Should the restatement's error of a case exceed 1e-6, the bound of that case is 10 times that
error instead.  Measured on an MI355X: worst |prob - prob64| 7.6e-7 (1 x 8 x 40 x 72, C = 4, r = 8, T = 5), 4.9e-7 at T = 1: the
error does not grow with T.
Class map: equal to the float64 arg-max wherever the float64 top-two gap is >= 1e-3 (at most 1 % of a case's pixels may fall below
that; 0.36 % do at most), and everywhere exactly the first-maximum arg-max of the returned probabilities."""
import functools

import numpy as np
import pytest
import torch

from tests import _crf_refine_reference as R

pytestmark = pytest.mark.gpu

BOUND = 1e-5


def _raw(z, x, T, r, d, prm=None, poison=True, want_cls=True, short=0, N=None, K=None, C=None):
    """pp_crf_refine on the C entry point itself -> (rc, prob, cls) as CPU tensors.  poison: prob starts as NaN, cls as -7, the
    workspace as NaN bytes.  short: bytes taken off the workspace size that is announced."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    prm = dict(R.DEFAULTS, **(prm or {}))
    n, k, H, W = z.shape
    c = x.shape[1]
    dll = lib.load()
    prob = torch.full(z.shape, float('nan'), device='cuda') if poison else torch.empty(z.shape, device='cuda')
    cls = torch.full((n, H, W), -7, device='cuda', dtype=torch.int64)
    nws = dll.pp_crf_refine_workspace(n, k, H, W)
    assert nws == 4 * z.numel()
    ws = torch.full((nws,), 0xFF, device='cuda', dtype=torch.uint8)
    rc = dll.pp_crf_refine(z.data_ptr(), x.data_ptr(), N or n, K or k, C or c, H, W, T, r, d, prm['sigma_xy'], prm['sigma_rgb'],
                           prm['sigma_smooth'], prm['w_bilateral'], prm['w_smooth'], prob.data_ptr(), cls.data_ptr() if want_cls else None,
                           ws.data_ptr(), nws - short, stream_ptr())
    torch.cuda.synchronize()
    return rc, prob.cpu(), cls.cpu()


@functools.lru_cache(maxsize=None)
def _device_inputs(case):
    z, x = R.inputs(case)
    return z.cuda(), x.cuda()


@functools.lru_cache(maxsize=None)
def _device_result(case, T):
    z, x = _device_inputs(case)
    rc, prob, cls = _raw(z, x, T, case[5], case[6])
    assert rc == 0
    return prob, cls


# ---- values against float64 ----
@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_values_and_class_map_against_float64(case, T):
    steps, err32 = R.oracle(case)
    want = steps[T - 1]
    prob, cls = _device_result(case, T)
    bound = BOUND if err32 <= 1e-6 else 10.0 * err32
    err = float((prob.double() - want).abs().max())
    z, _ = R.inputs(case)
    changed = float((want.argmax(1) != z.argmax(1)).double().mean())
    gap = R.top_two_gap(want)
    sure = gap >= 1e-3
    left_out = 1.0 - float(sure.double().mean())
    print(f'{R.case_id(case)} T={T}: max |prob - prob64| = {err:.3e} (bound {bound:.1e}; float32 restatement {err32:.3e}), '
          f'{100 * changed:.1f} % of the classes change, {100 * left_out:.2f} % of the pixels within 1e-3 of a tie')
    assert torch.isfinite(prob).all()
    assert err <= bound, (err, bound)
    assert left_out <= 0.01, left_out
    assert torch.equal(cls[sure], want.argmax(1)[sure])
    assert torch.equal(cls, prob.argmax(1))                       # torch's arg-max of equal values is the first, as the kernel's
    assert float((prob.double().sum(1) - 1.0).abs().max()) <= 1e-6
    moved = float((want - torch.softmax(z.double(), 1)).abs().max())
    if case[1] > 1 and case[2] * case[3] > 1:
        assert moved >= 1e-2, moved                               # 1000 bounds away from Q^0: a kernel that does nothing is seen
    else:
        assert changed == 0.0 and moved <= 1e-15                  # one class / one pixel: Q^T = Q^0


# ---- structure ----
def test_zero_weights_give_the_arg_max_of_the_logits():
    for case in (R.CASES[0], R.CASES[3], R.CASES[4]):
        z, x = _device_inputs(case)
        rc, prob, cls = _raw(z, x, 3, case[5], case[6], prm=dict(w_bilateral=0.0, w_smooth=0.0))
        assert rc == 0
        assert torch.equal(cls, z.argmax(1).cpu()), case
        assert float((prob.double() - torch.softmax(R.inputs(case)[0].double(), 1)).abs().max()) <= 1e-6, case


def test_two_runs_give_the_same_bits_and_cls_may_be_null():
    for case in (R.CASES[0], R.CASES[9]):
        z, x = _device_inputs(case)
        prob, cls = _device_result(case, 5)
        rc, again, cls2 = _raw(z, x, 5, case[5], case[6], poison=False)
        assert rc == 0 and torch.equal(again.view(torch.int32), prob.view(torch.int32)) and torch.equal(cls2, cls), case
        rc, nocls, untouched = _raw(z, x, 5, case[5], case[6], want_cls=False)
        assert rc == 0 and torch.equal(nocls.view(torch.int32), prob.view(torch.int32)) and bool((untouched == -7).all()), case


@pytest.mark.parametrize('shape', [(5, 37, 53, 1), (17, 16, 70, 3)], ids=['K5', 'K17'])
def test_a_slice_is_refined_alike_alone_and_in_a_batch(shape):
    K, H, W, C = shape
    z = R.noise_logits(3, K, H, W, 77).cuda()
    x = R.smooth_image(3, C, H, W, 78).cuda()
    rc, prob, cls = _raw(z, x, 3, 3, 2)
    assert rc == 0
    for n in range(3):
        rc, p1, c1 = _raw(z[n:n + 1].contiguous(), x[n:n + 1].contiguous(), 3, 3, 2)
        assert rc == 0
        assert torch.equal(p1[0].view(torch.int32), prob[n].view(torch.int32)) and torch.equal(c1[0], cls[n]), n


def test_the_result_lands_in_prob_for_even_and_odd_iteration_counts():
    case = R.CASES[0]
    z, x = _device_inputs(case)
    steps, _ = R.oracle(case)
    for T in (4, 5, 2):
        rc, prob, cls = _raw(z, x, T, case[5], case[6], poison=True)
        assert rc == 0
        assert torch.isfinite(prob).all() and bool((cls >= 0).all()), T
        assert float((prob.double() - steps[T - 1]).abs().max()) <= BOUND, T
    assert float((steps[3] - steps[4]).abs().max()) > 1e-3        # the two parities are told apart by the values


def test_refusals_leave_the_outputs_untouched():
    from pacingpseudo_amd._lib import lib
    case = R.CASES[0]
    z, x = _device_inputs(case)
    r, d = case[5], case[6]
    refused = [dict(short=1), dict(r=17, d=1), dict(r=1, d=17), dict(K=33), dict(C=5), dict(T=0), dict(prm=dict(sigma_xy=float('nan'))),
               dict(prm=dict(sigma_rgb=float('inf'))), dict(prm=dict(sigma_smooth=float('nan'))), dict(prm=dict(w_bilateral=float('inf')))]
    for kw in refused:
        kw = dict(kw)
        rc, prob, cls = _raw(z, x, kw.pop('T', 5), kw.pop('r', r), kw.pop('d', d), **kw)
        assert rc < 0 and lib.pp_last_error(), kw
        assert bool(torch.isnan(prob).all()) and bool((cls == -7).all()), kw
    rc, _, _ = _raw(z, x, 5, r, d, short=1)
    assert rc == -3


def test_wrapper_gives_what_the_entry_point_gives():
    from pacingpseudo_amd.utils import crf_refine
    case = R.CASES[3]
    z, x = _device_inputs(case)
    prob, cls = crf_refine(z, x, 5, case[5], case[6])
    want, want_cls = _device_result(case, 5)
    assert prob.dtype == torch.float32 and cls.dtype == torch.int64 and tuple(cls.shape) == (case[0], case[2], case[3])
    assert torch.equal(prob.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(cls.cpu(), want_cls)
    p2, none = crf_refine(z, x, 5, case[5], case[6], return_class=False)
    assert none is None and torch.equal(p2, prob)
    zt = z.transpose(2, 3)                                         # not contiguous: made so
    p3, _ = crf_refine(zt, x.transpose(2, 3), 1, 2, 1)
    p4, _ = crf_refine(zt.contiguous(), x.transpose(2, 3).contiguous(), 1, 2, 1)
    assert torch.equal(p3, p4)
    with pytest.raises(ValueError, match='image must be'):
        crf_refine(z, x[:, :, :-1], 5)
    with pytest.raises(NotImplementedError):
        crf_refine(z, torch.zeros(case[0], 5, case[2], case[3], device='cuda'), 5)


# ---- inference.evaluate ----
def _dice_rows(scores, label):
    from pacingpseudo_amd.utils.metrics import batch_dice_counts
    c = batch_dice_counts(scores, label)
    inter, ps, ts = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        d = 2.0 * inter / np.maximum(ps + ts, 1e-8)
    d[(ps == 0) & (ts == 0)] = np.nan
    return d.tolist()


def test_evaluate_with_crf_refinement():
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms, collate_by_shape, expand_compact
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.utils import crf_refine, keep_largest_components, tta_predict
    from pacingpseudo_amd.utils.metrics import batch_hd95
    K = 4
    torch.manual_seed(21)
    net = UNet(input_ch=1, init_ch=4, max_ch=32, num_classes=K, output_stride=8).cuda()
    with torch.no_grad():                                              # a random head's bias decides every pixel alike: without it, and
        net.final_conv.bias.zero_()                                    # with logits of the size of the weights, the arg-max varies over
        net.final_conv.weight.mul_(8.0)                                # a slice and the refinement has classes to change
    device = torch.device('cuda', 0)
    ds = SyntheticPhantoms(6, K, size=64, train=False, seed=1, native=True, compact=True)

    def loader():
        return torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate_by_shape)

    def batches():
        for groups in loader():
            for batch in (groups if isinstance(groups, list) else [groups]):
                yield expand_compact(batch, K, device)
    spacing = I.SPACING['acdc']
    crf = dict(iterations=3, radius=3, dilation=2, sigma_rgb=0.5, w_bilateral=3.0)
    plain = I.evaluate(net, loader(), K, spacing, device)
    off = I.evaluate(net, loader(), K, spacing, device, crf=None, extra=(extra_off := {}))
    assert len(plain) == len(off) == 2 and extra_off == {}
    for a, b in zip(plain, off):
        assert a.dtype == b.dtype and a.shape == b.shape == (6, K)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))    # bit-identical, NaN included
    # CRF alone
    extra = {}
    dice, hd = I.evaluate(net, loader(), K, spacing, device, crf=crf, extra=extra)
    assert sorted(extra) == ['crf_changed'] and extra['crf_changed'].shape == (6,) and extra['crf_changed'].dtype == np.int64
    rows, hds, changed = [], [], []
    net.eval()
    for batch in batches():
        with torch.no_grad():
            z = net(batch['image'])['segmentation/logits'].clone()
            prob, cls = crf_refine(z, batch['image'], **crf)
        changed.extend((cls != z.argmax(1)).flatten(1).sum(1).tolist())
        rows.extend(_dice_rows(prob, batch['label']))
        hds.extend(batch_hd95(cls, batch['label'].argmax(1), K, spacing).tolist())
    assert dice.shape == hd.shape == (6, K) and dice.dtype == hd.dtype == np.float32
    assert np.array_equal(dice, np.array(rows, np.float32), equal_nan=True)
    assert np.array_equal(hd, np.array(hds, np.float32), equal_nan=True)
    assert np.array_equal(extra['crf_changed'], np.array(changed, np.int64))
    print(f'crf_changed = {extra["crf_changed"].tolist()}')
    assert extra['crf_changed'].sum() > 0                               # the refinement is seen by the scores' inputs
    # TTA -> CRF -> CC
    extra = {}
    out = I.evaluate(net, loader(), K, spacing, device, keep_largest_cc=True, tta='flips', extra=extra, crf=crf)
    assert len(out) == 4 and sorted(extra) == ['crf_changed', 'tta_changed']
    dice, hd, ncomp, removed = out
    rows, hds, changed, ncomps, removeds = [], [], [], [], []
    for batch in batches():
        with torch.no_grad():
            mean, tta_cls = tta_predict(lambda t: net(t)['segmentation/logits'], batch['image'], 'flips')
            prob, cls = crf_refine(mean.clamp_min(1e-30).log(), batch['image'], **crf)
        changed.extend((cls != tta_cls).flatten(1).sum(1).tolist())
        pred, stats = keep_largest_components(cls, K, 1, return_stats=True)
        ncomps.extend(stats[..., 0].tolist())
        removeds.extend((pred != cls).flatten(1).sum(1).tolist())
        rows.extend(_dice_rows(torch.nn.functional.one_hot(pred, K).permute(0, 3, 1, 2), batch['label']))
        hds.extend(batch_hd95(pred, batch['label'].argmax(1), K, spacing).tolist())
    assert np.array_equal(dice, np.array(rows, np.float32), equal_nan=True)
    assert np.array_equal(hd, np.array(hds, np.float32), equal_nan=True)
    assert np.array_equal(extra['crf_changed'], np.array(changed, np.int64))
    assert np.array_equal(ncomp, np.array(ncomps, np.int32).reshape(-1, K)) and np.array_equal(removed, np.array(removeds, np.int64))


def test_inference_driver_with_the_refinement(tmp_path):
    """inference.py --crf_refine end to end on a random-weight checkpoint: eval_data.npz gains crf_changed and the log one line;
    without the flag exactly the keys, the values and the argument dump there were before."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd import inference as I
    from tests.test_gpu_step import build_model
    args = O.full_flags(epoch=2, num_classes=4, ignored_index=4, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    model = build_model(args, {k: v.numpy() for k, v in O.init_state(args, seed=3).items()})
    ck = tmp_path / 'run-fold0'
    (ck / 'ckps').mkdir(parents=True)
    torch.save(model.state_dict(), ck / 'ckps' / 'ckp_399.pth')
    common = ['--fold', '0', '--checkpoint_file', str(ck), '--dataset', 'acdc', '--synthetic', '6', '--image_size', '64', '--batch_size', '4',
              '--num_workers', '0', '--init_ch', '8', '--max_ch', '64']
    off_dice, off_hd = I.main(common + ['--root', str(tmp_path / 'off')])
    off = tmp_path / 'off' / 'Inference' / 'acdc' / 'run-fold0'
    assert sorted(np.load(off / 'eval_data.npz').files) == ['dicearr', 'hd95arr']
    off_log = (off / 'log.txt').read_text()
    assert 'crf_' not in off_log and 'CRF' not in off_log           # (the test's own name, part of every path in the log, has neither)
    dice, hd = I.main(common + ['--root', str(tmp_path / 'on'), '--crf_refine', '2', '--crf_radius', '3', '--crf_sigma_rgb', '0.5'])
    on = tmp_path / 'on' / 'Inference' / 'acdc' / 'run-fold0'
    z = np.load(on / 'eval_data.npz')
    assert sorted(z.files) == ['crf_changed', 'dicearr', 'hd95arr']
    assert z['crf_changed'].shape == (6,) and z['crf_changed'].dtype == np.int64 and (z['crf_changed'] >= 0).all()
    assert dice.shape == off_dice.shape == (6, 4) and np.array_equal(z['dicearr'], dice, equal_nan=True)
    log = (on / 'log.txt').read_text()
    assert 'CRF refinement (2 iterations, radius 3 x dilation 1): {} pixels differ'.format(int(z['crf_changed'].sum())) in log
    assert 'crf_refine=2' in log and 'crf_w_smooth=1.0' in log
    I.main(common + ['--root', str(tmp_path / 'all'), '--crf_refine', '1', '--keep_largest_cc', '--tta', 'flips', '--surface_metrics'])
    za = np.load(tmp_path / 'all' / 'Inference' / 'acdc' / 'run-fold0' / 'eval_data.npz')
    assert sorted(za.files) == sorted(['dicearr', 'hd95arr', 'hdarr', 'assdarr', 'nsdarr', 'ncomp', 'removed', 'tta_changed', 'crf_changed'])
    with pytest.raises(SystemExit):
        I.main(common + ['--root', str(tmp_path / 'bad'), '--crf_refine', '2', '--crf_radius', '9'])
    assert not (tmp_path / 'bad').exists()                              # refused before anything was created or built
