"""cr_variant 5 bikl_loss, 6 js_loss, 7 hard_ce_loss of pp_seg_losses_fwd / pp_seg_losses_bwd on the device: the kernels entry by entry
against the float64 reference of tests/_cr_reference.py (criteria of tests/test_gpu_ops.py::test_seg_losses: loss within
1e-5 * max(1, |ref|), rel(dz, ref) < 1e-4 for both gradients, all gradients finite), the functional API, and the whole step.

Shapes: K = 5, 24x20 takes the four-pixel kernels; the same from a pointer one float off 16-byte alignment and 5x7 take the
one-pixel MK = 8 kernels; K = 3 / 9 / 17 / 32 the MK = 8 / 16 / 32 ones; K = 2, N = 5, 256x256 has more pixels (327 680) than one pass
of the 1024 x 256 partial grid.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _cr_reference as R  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests.test_gpu_step import TOL_OUT, build_model, check_grads, iteration, oracle_with_device_branches  # noqa: E402

TOL = 1e-4
GW = dict(pce=0.7, ent=0.3, cr=1.9)
NEW = ['bikl_loss', 'js_loss', 'hard_ce_loss']
OLD_CODE = {'ce_loss': 1, 'l1_loss': 2, 'l2_loss': 3, 'kl_loss': 4}


def dev():
    return torch.device('cuda', 0)


def _lib():
    from pacingpseudo_amd._lib import lib, stream_ptr
    return lib, stream_ptr()


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


_INPUTS = {}


def _inputs(N, K, H, W, seed):
    """(weak logits, strong logits, class map with K = ignored, mask), fp32 on the CPU; made once per shape and never modified."""
    key = (N, K, H, W, seed)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(seed)
        zw = torch.randn(N, K, H, W, generator=g) * 2
        zs = torch.randn(N, K, H, W, generator=g) * 2
        t = torch.randint(0, K + 1, (N, H, W), generator=g)
        mask = (torch.rand(N, 1, H, W, generator=g) > 0.3).float()
        _INPUTS[key] = (zw, zs, t, mask)
    return _INPUTS[key]


def _misaligned(x):
    """A copy of x on the device whose first element lies one element past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 4, dtype=x.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _device(zw, zs, t, mask, vcode, detach, gw=GW, shift=False, do_ent=1):
    """pp_seg_losses_fwd -> pp_losses_finalize -> pp_seg_losses_bwd, as tests/test_gpu_ops.py::test_seg_losses calls them."""
    lib, st = _lib()
    N, K, H, W = zw.shape
    put = _misaligned if shift else (lambda x: x.to(dev()))
    zwd, td = put(zw), t.to(dev())
    zsd = put(zs) if vcode else None
    md = mask.to(dev()) if mask is not None else None
    sums = torch.zeros(6, dtype=torch.float64, device=dev())
    nws = lib.pp_seg_losses_workspace(N, H * W)
    ws = torch.empty(nws + 64, dtype=torch.uint8, device=dev())
    lib.pp_seg_losses_fwd(zwd.data_ptr(), zsd.data_ptr() if vcode else None, td.data_ptr(), md.data_ptr() if md is not None else None,
                          N, K, H * W, K, do_ent, vcode, sums.data_ptr(), ws.data_ptr(), nws, st)
    lp, le, lc = (torch.zeros((), device=dev()) for _ in range(3))
    lib.pp_losses_finalize(sums.data_ptr(), 1 if md is not None else 0, lp.data_ptr(), le.data_ptr(), lc.data_ptr() if vcode else None, st)
    dzw = put(torch.full_like(zw, float('nan')))
    dzs = put(torch.full_like(zw, float('nan'))) if vcode else None
    gs = {k: torch.tensor(v, device=dev()) for k, v in gw.items()}
    lib.pp_seg_losses_bwd(zwd.data_ptr(), zsd.data_ptr() if vcode else None, td.data_ptr(), md.data_ptr() if md is not None else None,
                          N, K, H * W, K, do_ent, vcode, 1 if detach else 0, sums.data_ptr(), gs['pce'].data_ptr(), gs['ent'].data_ptr(),
                          gs['cr'].data_ptr(), 1.0, dzw.data_ptr(), dzs.data_ptr() if vcode else None, st)
    torch.cuda.synchronize()
    return dict(pce=lp.cpu(), ent=le.cpu(), cr=lc.cpu(), dzw=dzw.cpu(), dzs=dzs.cpu() if vcode else None, sums=sums.cpu())


def _reference(zw, zs, t, mask, cr_fn, gw=GW):
    """The three losses and d(sum_i g_i loss_i) / d logits in float64; cr_fn(zs, zw, mask) -> the consistency loss."""
    K = zw.shape[1]
    zwr, zsr = zw.double().requires_grad_(True), zs.double().requires_grad_(True)
    m = mask.double() if mask is not None else None
    pce = O.partial_cross_entropy_loss(zwr, t, K)
    ent = O.entropy_minimization_loss(zwr, m)
    cr = cr_fn(zsr, zwr, m)
    (gw['pce'] * pce + gw['ent'] * ent + gw['cr'] * cr).backward()
    return dict(pce=float(pce.detach()), ent=float(ent.detach()), cr=float(cr.detach()), dzw=zwr.grad, dzs=zsr.grad if zsr.grad is not None else torch.zeros_like(zsr))


def _check(got, ref, tag=''):
    print(f'{tag} loss errors pce {abs(float(got["pce"]) - ref["pce"]):.2e} ent {abs(float(got["ent"]) - ref["ent"]):.2e} '
          f'cr {abs(float(got["cr"]) - ref["cr"]):.2e} (cr {ref["cr"]:.4e}); rel dzw {rel(got["dzw"], ref["dzw"]):.2e} '
          f'dzs {rel(got["dzs"], ref["dzs"]):.2e}')
    for k in ('pce', 'ent', 'cr'):
        assert abs(float(got[k]) - ref[k]) < 1e-5 * max(1, abs(ref[k])), (k, float(got[k]), ref[k])
    assert torch.isfinite(got['dzw']).all() and torch.isfinite(got['dzs']).all()
    assert rel(got['dzw'], ref['dzw']) < TOL
    assert rel(got['dzs'], ref['dzs']) < TOL


def _new_case(name, zw, zs, t, mask, detach, shift=False):
    got = _device(zw, zs, t, mask, R.CODE[name], detach, shift=shift)
    ref = _reference(zw, zs, t, mask, lambda a, b, m: R.consistency(name, a, b, m, detach))
    _check(got, ref, f'{name} {tuple(zw.shape)}')
    return got


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('detach', [False, True])
@pytest.mark.parametrize('spread', [1.0, 60.0])
def test_four_pixel_form(name, use_mask, detach, spread):
    """K = 5, 24x20: the v4 kernels.  Spread 60: logit gaps beyond 87, probabilities that are exact zeros in fp32."""
    zw, zs, t, mask = _inputs(2, 5, 24, 20, 3)
    _new_case(name, zw * spread, zs * spread, t, mask if use_mask else None, detach)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('geom', ['one float off', '5x7'])
@pytest.mark.parametrize('use_mask,detach,spread', [(True, False, 1.0), (False, True, 60.0), (True, False, 60.0)])
def test_one_pixel_form_at_5_classes(name, geom, use_mask, detach, spread):
    """The MK = 8 one-pixel kernels at K = 5: the 24x20 logits from a pointer that is not 16-byte aligned, and an odd plane."""
    if geom == '5x7':
        zw, zs, t, mask = _inputs(2, 5, 5, 7, 4)
        _new_case(name, zw * spread, zs * spread, t, mask if use_mask else None, detach)
    else:
        zw, zs, t, mask = _inputs(2, 5, 24, 20, 3)
        _new_case(name, zw * spread, zs * spread, t, mask if use_mask else None, detach, shift=True)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('K', [3, 9, 17, 32])
@pytest.mark.parametrize('use_mask,detach,spread', [(True, False, 1.0), (False, True, 1.0), (True, False, 60.0), (False, False, 60.0)])
def test_class_bounds(name, K, use_mask, detach, spread):
    """K = 3, 9, 17 and 32: the MK = 8, 16 and 32 instantiations, on an odd plane (7x9) of two images."""
    zw, zs, t, mask = _inputs(2, K, 7, 9, K)
    _new_case(name, zw * spread, zs * spread, t, mask if use_mask else None, detach)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('use_mask', [False, True])
def test_one_class_is_all_zero(name, use_mask):
    """K = 1: both soft-maxes are 1, every loss and every gradient is exactly 0."""
    zw, zs, t, mask = _inputs(2, 1, 6, 5, 1)
    got = _device(zw, zs, t, mask if use_mask else None, R.CODE[name], False)
    assert float(got['pce']) == 0.0 and float(got['ent']) == 0.0 and float(got['cr']) == 0.0
    assert not got['dzw'].any() and not got['dzs'].any()


_BIG = {}


@pytest.mark.parametrize('name', NEW)
def test_more_pixels_than_one_grid_pass(name):
    """K = 2, N = 5, 256x256 (four-pixel form): 327 680 pixels against the 262 144 threads of the partial grid -- the stride loops."""
    zw, zs, t, mask = _inputs(5, 2, 256, 256, 11)
    got = _device(zw, zs, t, mask, R.CODE[name], False)
    if name not in _BIG:
        _BIG[name] = _reference(zw, zs, t, mask, lambda a, b, m: R.consistency(name, a, b, m, False))
    _check(got, _BIG[name], f'{name} big')


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('K,H,W', [(5, 24, 20), (9, 7, 9)])
def test_near_agreement(name, use_mask, K, H, W):
    """z_s = z_w + 1e-3 noise: bi-KL and JS are differences of nearly equal numbers there (their values ~1e-7, their gradients ~1e-3
    of a probability) -- the regime of late training.  Same criteria."""
    zw, noise, t, mask = _inputs(2, K, H, W, 5)
    zs = zw + 1e-3 * noise
    _new_case(name, zw, zs, t, mask if use_mask else None, False)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('K,H,W,shift', [(5, 24, 20, False), (5, 24, 20, True), (17, 7, 9, False)])
def test_detached_weak_gradient_is_that_of_pce_and_entropy_bit_for_bit(name, K, H, W, shift):
    """detach_weak = 1: dz_w is the gradient of pCE + entropy alone -- the bits of a cr_variant = 0 call with the same upstream
    scalars.  hard_ce_loss gives the weak logits no consistency gradient with detach_weak = 0 either."""
    zw, zs, t, mask = _inputs(2, K, H, W, 3)
    base = _device(zw, zs, t, mask, 0, False, shift=shift)
    got = _device(zw, zs, t, mask, R.CODE[name], True, shift=shift)
    assert torch.equal(got['dzw'], base['dzw'])
    assert float(got['pce']) == float(base['pce']) and float(got['ent']) == float(base['ent'])
    free = _device(zw, zs, t, mask, R.CODE[name], False, shift=shift)
    assert torch.equal(free['dzs'], got['dzs'])                       # the strong-view gradient does not depend on the flag
    assert torch.equal(free['dzw'], base['dzw']) == (name == 'hard_ce_loss')


@pytest.mark.parametrize('K,H,W', [(5, 24, 20), (5, 5, 7), (9, 7, 9)])
@pytest.mark.parametrize('use_mask', [False, True])
def test_hard_label_ties_go_to_the_first_maximum(K, H, W, use_mask):
    """Planted ties among the weak LOGITS: two equal maxima, three equal maxima, all K equal -- torch.argmax's rule, the first."""
    zw, zs, t, mask = _inputs(2, K, H, W, 6)
    zw = zw.clone()
    top = float(zw.abs().max()) + 1.0
    first = zw.argmax(1)
    zw[:, :, 0, :] = zw[:, :, 0, :].clamp(max=0.0)
    zw[:, 1, 0, :] = zw[:, 3, 0, :] = top;                                            first[:, 0, :] = 1     # two
    zw[:, 0, 1, :] = zw[:, 2, 1, :] = zw[:, 4, 1, :] = top;                           first[:, 1, :] = 0     # three
    zw[:, :, 2, :] = 0.25;                                                            first[:, 2, :] = 0     # all
    zw[0, :, 3, 0] = -3.0;                                                            first[0, 3, 0] = 0     # all, negative
    assert torch.equal(zw.argmax(1), first)
    m = mask if use_mask else None
    got = _device(zw, zs, t, m, 7, False)
    ref = _reference(zw, zs, t, m, lambda a, b, mm: R.hard_label_cross_entropy_loss(a, b, mm))
    _check(got, ref, 'ties')
    # and directly: dz_s = g_cr m / D (s - onehot(first)), D = pixels or max(sum(mask), 1e-8)
    s = torch.softmax(zs.double(), 1)
    mm = m.double() if use_mask else torch.ones(2, 1, H, W, dtype=torch.float64)
    want = GW['cr'] * mm / (mm.sum() if use_mask else mm.numel()) * (s - torch.nn.functional.one_hot(first, K).permute(0, 3, 1, 2))
    assert rel(got['dzs'][:, :, :4], want[:, :, :4]) < TOL


@pytest.mark.parametrize('name', NEW)
def test_all_zero_mask(name):
    """sum(mask) = 0: the denominators are the 1e-8 clamp, the masked losses are 0 and every gradient is finite."""
    zw, zs, t, mask = _inputs(2, 5, 24, 20, 3)
    zero = torch.zeros_like(mask)
    got = _new_case(name, zw * 60.0, zs * 60.0, t, zero, False)
    assert float(got['cr']) == 0.0 and float(got['ent']) == 0.0 and not got['dzs'].any()


@pytest.mark.parametrize('variant,use_mask,detach', [('ce_loss', True, False), ('l1_loss', True, False), ('l2_loss', False, True),
                                                     ('kl_loss', True, True)])
def test_the_four_earlier_variants_still_meet_the_criteria(variant, use_mask, detach):
    zw, zs, t, mask = _inputs(2, 5, 24, 20, 3)
    m = mask if use_mask else None

    def cr(zsr, zwr, mm):
        pw = torch.softmax(zwr, 1)
        pw = pw.detach() if detach else pw
        return {'ce_loss': lambda: O.soft_label_cross_entropy_loss(zsr, pw, mm), 'l1_loss': lambda: O.l1_loss(torch.softmax(zsr, 1), pw, mm),
                'l2_loss': lambda: O.l2_loss(torch.softmax(zsr, 1), pw, mm), 'kl_loss': lambda: O.kl_loss(zsr, zwr, mm)}[variant]()
    _check(_device(zw, zs, t, m, OLD_CODE[variant], detach), _reference(zw, zs, t, m, cr), variant)


def test_codes_beyond_seven_are_refused():
    from pacingpseudo_amd._lib import HipLibraryError
    lib, st = _lib()
    z = torch.zeros(1, 5, 4, 4, device=dev())
    t = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev())
    sums = torch.zeros(6, dtype=torch.float64, device=dev())
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev())
    g = torch.ones((), device=dev())
    for code in (8, -1):
        with pytest.raises(HipLibraryError, match='variant=%d' % code):
            lib.pp_seg_losses_fwd(z.data_ptr(), z.data_ptr(), t.data_ptr(), None, 1, 5, 16, 5, 0, code, sums.data_ptr(), ws.data_ptr(), 1 << 16, st)
        with pytest.raises(HipLibraryError, match='variant=%d' % code):
            lib.pp_seg_losses_bwd(z.data_ptr(), z.data_ptr(), t.data_ptr(), None, 1, 5, 16, 5, 0, code, 0, sums.data_ptr(), g.data_ptr(),
                                  g.data_ptr(), g.data_ptr(), 1.0, z.data_ptr(), z.data_ptr(), st)


# ---------------------------------------------------------------- functional API
API = {'bikl_loss': 'bidirectional_kl_loss', 'js_loss': 'js_loss', 'hard_ce_loss': 'hard_label_cross_entropy_loss'}


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('use_mask', [False, True])
def test_functional_api(name, use_mask):
    import pacingpseudo_amd.losses as L
    zw, zs, _, mask = _inputs(2, 5, 24, 20, 3)
    f = getattr(L, API[name])
    a, b = zs.to(dev()).requires_grad_(True), zw.to(dev()).requires_grad_(True)
    m = mask.to(dev()) if use_mask else None
    loss = f(a, b, m) if use_mask else f(a, b)
    (loss * 1.5).backward()
    ar, br = zs.double().requires_grad_(True), zw.double().requires_grad_(True)
    ref = R.BY_NAME[name](ar, br, mask.double() if use_mask else None)
    (ref * 1.5).backward()
    loss, ref = loss.detach(), ref.detach()
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1, abs(float(ref)))
    assert rel(a.grad, ar.grad) < TOL
    if name == 'hard_ce_loss':
        assert b.grad is None or not b.grad.any()
        assert br.grad is None
    else:
        assert rel(b.grad, br.grad) < TOL
    # the argument checks of _check
    for bad in (zs, zs.to(dev()).double(), zs.to(dev())[0]):
        with pytest.raises(TypeError, match='input must be a 4-D float32 CUDA tensor'):
            f(bad, b)
    with pytest.raises(TypeError, match='target must be a 4-D float32 CUDA tensor'):
        f(a, zw)
    with pytest.raises(TypeError, match='valid_mask must be a 4-D float32 CUDA tensor'):
        f(a, b, mask)


# ---------------------------------------------------------------- the whole step
def _small_args(name, detach):
    return O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], loss_cr_variants=name, detach_weak_cr=detach)


@pytest.mark.parametrize('name,detach', [(n, False) for n in NEW] + [(n, True) for n in NEW])
def test_step_against_the_oracle(name, detach, monkeypatch):
    """The full-flags step on the small network: logits, the five losses and every parameter gradient against the oracle.  The oracle
    has no such variant: it is given 'kl_loss' -- the form that hands both LOGIT tensors to its loss -- and its kl_loss is replaced by
    the float64-checked reference function (which detaches the weak logits for --detach_weak_cr, as the model does)."""
    from pacingpseudo_amd.optim import FusedAdam
    epoch = 100                                                    # past the ramp-up: the consistency loss has its full weight
    args = _small_args(name, detach)
    oargs = _small_args('kl_loss', detach)
    monkeypatch.setattr(O, 'kl_loss', lambda a, b, m=None: R.consistency(name, a, b, m, detach))
    torch.manual_seed(2)
    model = build_model(args)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batch = O.synthetic_batch(2, 64, 64, seed=9, keep=0.08)
    batch['valid_mask'][:, :, :, :5] = 0
    opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
    ref_out, _, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, epoch, oargs, training=True)
    rec, grads = iteration(model, opt, batch, args, epoch)
    assert {'loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'} <= set(ref_out)
    for k, v in ref_out.items():
        if k.startswith('_') or not torch.is_tensor(v):
            continue
        e = G.rel_err(rec[k].double().cpu().numpy(), v.numpy())
        print(f'{name} detach={detach} {k}: rel err {e:.3e}')
        assert e < TOL_OUT, f'{k}: rel err {e:.3e}'
    assert float(ref_out['loss_cr']) > 0
    _, og, _ = oracle_with_device_branches(model, sd, batch, epoch, oargs, True)
    check_grads(grads, {k: v.numpy() for k, v in og.items() if v is not None}, True)


def test_graph_replay_equals_eager_with_js_loss():
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    from tests.test_gpu_graph import _eager_step, _loss_fn
    args = _small_args('js_loss', False)
    f = _loss_fn(args)
    batches = [{k: v.cuda() for k, v in O.synthetic_batch(2, 64, 64, seed=s, keep=0.05).items() if k != 'label'} for s in (3, 4)]
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(1)
        model = build_model(args)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)
        gs = GraphedStep(model, opt, f, warmup=1) if tag == 'graph' else None
        model.train()
        losses = []
        for i in range(4):
            b = batches[i % 2]
            losses.append(_eager_step(model, opt, f, b, 100) if gs is None else gs(b, 100)[0].detach().clone())
        torch.cuda.synchronize()
        runs[tag] = dict(losses=torch.stack(losses).cpu(), params=model.flat.params.clone(),
                         state={k: v.detach().clone() for k, v in model.state_dict().items()})
    e, g = runs['eager'], runs['graph']
    assert torch.isfinite(e['losses']).all()
    assert torch.equal(e['losses'], g['losses']) and torch.equal(e['params'], g['params'])
    for k, v in e['state'].items():
        assert torch.equal(v, g['state'][k]), k


@pytest.mark.parametrize('name', NEW)
def test_training_driver(name, tmp_path):
    """train_chaos.py --synthetic with the new name: two epochs, finite losses and validation Dice."""
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'out')
    vd = train_main(['--tag', name, '--session', 'Experiment', '--root', root, '--synthetic', '8', '--epoch', '2', '--batch_size', '4',
                     '--image_size', '64', '--num_workers', '0', '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path',
                     '--do_memory', '--loss_cr_variants', name])
    assert np.isfinite(np.asarray(vd)).all()
    run = glob.glob(os.path.join(root, 't1', 'Experiment', f'Experiment-*-fold1-{name}'))
    assert len(run) == 1
    log = open(os.path.join(run[0], 'log.txt')).read()
    assert f'loss_cr_variants={name}\n' in log
    assert 'nan' not in log.split('val: 001')[0].lower()
