"""9 to 32 segmentation classes: the MK = 16 / 32 instantiations of the loss and head kernels against the fp64 reference, the whole
step, 16-bit storage, the graph replay, the upper-bound step and the drivers at K > 8.

The K <= 8 forms keep their own tests (test_gpu_ops.py, test_gpu_step.py); the cases here use the same tolerances.
"""
import glob
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests.test_gpu_step import TOL_OUT, build_model, check_grads, iteration, oracle_with_device_branches  # noqa: E402

TOL = 1e-4
WIDE_K = [9, 16, 17, 32]
GEOMS = [(2, 7, 9), (2, 16, 12)]          # (N, H, W): odd H * W (one-pixel forms only) and a multiple of 4


def _lib(storage='fp32'):
    from pacingpseudo_amd._lib import lib_for, stream_ptr
    return lib_for(storage), stream_ptr()


def dev():
    return torch.device('cuda', 0)


def rel(a, b):
    """max |a - b| over max |b|, with max |b| floored at 1e-20: at spread 60 the fp64 strong-view gradient of the l1 / l2 terms is
    ~1e-60 everywhere, a zero in fp32, and the device's exact zeros must pass."""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-20))


def _loss_inputs(N, K, H, W, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    zw = torch.randn(N, K, H, W, generator=g) * 2
    zs = torch.randn(N, K, H, W, generator=g) * 2
    t = torch.randint(0, K + 1, (N, H, W), generator=g)
    if all_ignored:
        t[:] = K
    mask = (torch.rand(N, 1, H, W, generator=g) > 0.3).float()
    return zw, zs, t, mask


def _seg_losses_device(zw, zs, t, mask, K, variant, detach, gw):
    lib, st = _lib()
    N, _, H, W = zw.shape
    vcode = {None: 0, 'ce_loss': 1, 'l1_loss': 2, 'l2_loss': 3, 'kl_loss': 4}[variant]
    zwd, zsd, td = zw.to(dev()), zs.to(dev()), t.to(dev())
    md = mask.to(dev()) if mask is not None else None
    sums = torch.zeros(6, dtype=torch.float64, device=dev())
    nws = lib.pp_seg_losses_workspace(N, H * W)
    ws = torch.empty(nws + 64, dtype=torch.uint8, device=dev())
    lib.pp_seg_losses_fwd(zwd.data_ptr(), zsd.data_ptr() if variant else None, td.data_ptr(), md.data_ptr() if md is not None else None,
                          N, K, H * W, K, 1, vcode, sums.data_ptr(), ws.data_ptr(), nws, st)
    lp, le, lc = (torch.zeros((), device=dev()) for _ in range(3))
    lib.pp_losses_finalize(sums.data_ptr(), 1 if md is not None else 0, lp.data_ptr(), le.data_ptr(), lc.data_ptr() if variant else None, st)
    dzw = torch.empty_like(zwd)
    dzs = torch.zeros_like(zsd)
    gs = {k: torch.tensor(v, device=dev()) for k, v in gw.items()}
    lib.pp_seg_losses_bwd(zwd.data_ptr(), zsd.data_ptr() if variant else None, td.data_ptr(), md.data_ptr() if md is not None else None,
                          N, K, H * W, K, 1, vcode, 1 if detach else 0, sums.data_ptr(), gs['pce'].data_ptr(), gs['ent'].data_ptr(),
                          gs['cr'].data_ptr(), 1.0, dzw.data_ptr(), dzs.data_ptr() if variant else None, st)
    torch.cuda.synchronize()
    return lp, le, lc, dzw, dzs


@pytest.mark.parametrize('K', WIDE_K)
@pytest.mark.parametrize('N,H,W', GEOMS)
@pytest.mark.parametrize('variant,use_mask,detach', [(None, True, False), ('ce_loss', True, False), ('ce_loss', False, True),
                                                     ('l1_loss', True, False), ('l2_loss', False, True), ('kl_loss', True, True)])
@pytest.mark.parametrize('spread', [1.0, 60.0])
def test_seg_losses_wide(K, N, H, W, variant, use_mask, detach, spread):
    zw, zs, t, mask = _loss_inputs(N, K, H, W, K + H)
    zw, zs = zw * spread, zs * spread
    gw = dict(pce=0.7, ent=0.3, cr=1.9)
    zwr, zsr = zw.double().requires_grad_(True), zs.double().requires_grad_(True)
    m = mask.double() if use_mask else None
    pce = O.partial_cross_entropy_loss(zwr, t, K)
    ent = O.entropy_minimization_loss(zwr, m)
    total = gw['pce'] * pce + gw['ent'] * ent
    cr = None
    if variant:
        pw = torch.softmax(zwr, 1)
        if detach:
            pw = pw.detach()
        cr = {'ce_loss': lambda: O.soft_label_cross_entropy_loss(zsr, pw, m),
              'l1_loss': lambda: O.l1_loss(torch.softmax(zsr, 1), pw, m),
              'l2_loss': lambda: O.l2_loss(torch.softmax(zsr, 1), pw, m),
              'kl_loss': lambda: O.kl_loss(zsr, zwr, m)}[variant]()
        total = total + gw['cr'] * cr
    total.backward()
    lp, le, lc, dzw, dzs = _seg_losses_device(zw, zs, t, mask if use_mask else None, K, variant, detach, gw)
    assert abs(float(lp) - float(pce)) < 1e-5 * max(1, abs(float(pce)))
    assert abs(float(le) - float(ent)) < 1e-5 * max(1, abs(float(ent)))
    if variant:
        assert abs(float(lc) - float(cr)) < 1e-5 * max(1, abs(float(cr)))
    assert torch.isfinite(dzw).all() and torch.isfinite(dzs).all()
    assert rel(dzw, zwr.grad) < TOL
    if variant:
        # measured against the whole logit gradient: at spread 60 the l1 term's strong-view gradient can be ~1e-7 while the weak
        # view's is ~1e-2, and there torch's own fp32 gradient is ~1 % off the fp64 one
        scale = max(float(zwr.grad.abs().max()), float(zsr.grad.abs().max()))
        assert float((dzs.double().cpu() - zsr.grad).abs().max()) < TOL * scale


@pytest.mark.parametrize('K', [17, 32])
def test_seg_losses_wide_all_ignored_is_nan(K):
    zw, zs, t, mask = _loss_inputs(1, K, 8, 8, 5, all_ignored=True)
    lp, *_ = _seg_losses_device(zw, zs, t, None, K, None, False, dict(pce=1.0, ent=0.0, cr=0.0))
    assert math.isnan(float(lp)) and math.isnan(float(O.partial_cross_entropy_loss(zw, t, K)))


@pytest.mark.parametrize('K', [17, 32])
def test_wide_forms_are_deterministic(K):
    """The same inputs twice give the same bits: losses, logit gradients and the head's parameter gradients."""
    zw, zs, t, mask = _loss_inputs(2, K, 16, 12, 1)
    gw = dict(pce=0.7, ent=0.3, cr=1.9)
    a = _seg_losses_device(zw, zs, t, mask, K, 'kl_loss', False, gw)
    b = _seg_losses_device(zw, zs, t, mask, K, 'kl_loss', False, gw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ha = _head_device('fp32', *_head_inputs(32, K, 2, 24, 20, 3))
    hb = _head_device('fp32', *_head_inputs(32, K, 2, 24, 20, 3))
    for x, y in zip(ha, hb):
        assert torch.equal(x, y)


@pytest.mark.parametrize('K', WIDE_K)
@pytest.mark.parametrize('H,W', [(63, 65), (64, 64)])
def test_aux_pce_wide(K, H, W):
    lib, st = _lib()
    N, h, w = 2, 8, 8
    g = torch.Generator().manual_seed(K)
    lo = torch.randn(N, K, h, w, generator=g)
    t = torch.randint(0, K + 1, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) > 0.1] = K
    lor = lo.double().requires_grad_(True)
    up = F.interpolate(lor, size=(H, W), mode='bilinear', align_corners=True)
    loss = O.partial_cross_entropy_loss(up, t, K)
    (0.01 * loss).backward()
    lod, td = lo.to(dev()), t.to(dev())
    upd = torch.empty(N, K, H, W, device=dev())
    sums = torch.zeros(2, dtype=torch.float64, device=dev())
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev())
    lib.pp_aux_pce_fwd(lod.data_ptr(), N, K, h, w, H, W, td.data_ptr(), K, upd.data_ptr(), sums.data_ptr(), ws.data_ptr(), 1 << 16, st)
    lv = torch.zeros((), device=dev())
    lib.pp_losses_finalize(sums.data_ptr(), 0, lv.data_ptr(), None, None, st)
    assert rel(upd, up) < 1e-5
    assert abs(float(lv) - float(loss)) < 1e-5 * abs(float(loss))
    dlo = torch.empty(N, K, h, w, device=dev())
    gg = torch.tensor(0.01, device=dev())
    lib.pp_aux_pce_bwd(upd.data_ptr(), td.data_ptr(), K, gg.data_ptr(), 1.0, sums.data_ptr(), dlo.data_ptr(), N, K, h, w, H, W, st)
    assert rel(dlo, lor.grad) < TOL


@pytest.mark.parametrize('K', WIDE_K)
def test_memory_ce_wide(K):
    lib, st = _lib()
    hid = 64
    g = torch.Generator().manual_seed(K)
    bank = torch.randn(K, hid, 1, 1, generator=g)
    wfc = torch.randn(K, hid, 1, 1, generator=g)
    wr = wfc.double().requires_grad_(True)
    loss = O.cross_entropy_loss(F.conv2d(bank.double(), wr).squeeze(-1).squeeze(-1), torch.arange(K))
    (1.5 * loss).backward()
    lv = torch.zeros((), device=dev())
    bd, wd = bank.to(dev()), wfc.to(dev())
    lib.pp_memory_ce_fwd(bd.data_ptr(), wd.data_ptr(), K, hid, lv.data_ptr(), st)
    assert abs(float(lv) - float(loss)) < 1e-5 * abs(float(loss))
    dw = torch.zeros(K, hid, device=dev())
    gg = torch.tensor(1.5, device=dev())
    lib.pp_memory_ce_bwd(bd.data_ptr(), wd.data_ptr(), K, hid, gg.data_ptr(), 1.0, dw.data_ptr(), 0, st)
    assert rel(dw, wr.grad.view(K, hid)) < TOL


@pytest.mark.parametrize('K', WIDE_K)
@pytest.mark.parametrize('H,W', [(31, 33), (32, 32)])
def test_dice_counts_wide(K, H, W):
    from pacingpseudo_amd.utils.metrics import batch_dice
    g = torch.Generator().manual_seed(K)
    N = 3
    logits = torch.randn(N, K, H, W, generator=g)
    lab = torch.randint(0, K - 1, (N, H, W), generator=g)        # class K-1 never present in the label
    logits[:, K - 1] = -50.0                                      # ... nor predicted -> NaN entry
    onehot = F.one_hot(lab, K).permute(0, 3, 1, 2).float().contiguous()
    got = batch_dice(logits.to(dev()), onehot.to(dev()))
    sm = torch.softmax(logits, 1).numpy()
    ref = np.asarray([O.compute_dice(sm[n], onehot.numpy()[n]) for n in range(N)])
    assert got.shape == (N, K)
    assert np.allclose(got, ref, atol=1e-6, equal_nan=True)
    assert np.isnan(got[:, K - 1]).all()


@pytest.mark.parametrize('K', WIDE_K)
@pytest.mark.parametrize('H,W', [(31, 33), (32, 32)])
def test_dice_loss_wide(K, H, W):
    from pacingpseudo_amd.losses.losses import dice_loss_fn
    g = torch.Generator().manual_seed(K + H)
    N = 2
    logits = torch.randn(N, K, H, W, generator=g) * 2
    lab = F.one_hot(torch.randint(0, K, (N, H, W), generator=g), K).permute(0, 3, 1, 2).float().contiguous()
    zr = logits.double().requires_grad_(True)
    ref = O.dice_loss_fn(zr, lab.double())
    (0.8 * ref).backward()
    zd = logits.to(dev()).requires_grad_(True)
    got = dice_loss_fn(zd, lab.to(dev()))
    (0.8 * got).backward()
    assert abs(float(got) - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))
    assert rel(zd.grad, zr.grad) < TOL


def _head_inputs(C, K, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 1, 1, generator=g) / math.sqrt(C)
    b = torch.randn(K, generator=g)
    dl = torch.randn(N, K, H, W, generator=g)
    return x, w, b, dl


_ACT = {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}


def _lazy_rows(C, N, seed):
    """Per-image BatchNorm coefficient rows of a lazy activation: y = LeakyReLU(x * scale + shift), slope 0.01."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    return scale, shift


def _head_device(storage, x, w, b, dl, lazy=None):
    """fwd + bwd of the 1x1 head on the device; x is stored in `storage`, everything else is fp32."""
    from pacingpseudo_amd._lib import PpLazyIn
    lib, st = _lib(storage)
    N, C, H, W = x.shape
    K = w.shape[0]
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev(), _ACT[storage])
    wd, bd = w.to(dev()).contiguous(), b.to(dev())
    logits = torch.empty(N, K, H, W, device=dev())
    nws = lib.pp_conv1x1_bwd_workspace(K, C, N, H * W)
    ws = torch.empty(nws + 64, dtype=torch.uint8, device=dev())
    dx = torch.empty(N, H, W, C, device=dev(), dtype=_ACT[storage])
    dw = torch.empty(K, C, device=dev())
    db = torch.empty(K, device=dev())
    dld = dl.to(dev())
    if lazy is None:
        lib.pp_conv1x1_nhwc_to_nchw_fwd(xd.data_ptr(), C, C, wd.data_ptr(), bd.data_ptr(), logits.data_ptr(), K, N, H * W, st)
        lib.pp_conv1x1_nchw_to_nhwc_bwd(dld.data_ptr(), xd.data_ptr(), C, C, wd.data_ptr(), dx.data_ptr(), C, dw.data_ptr(), db.data_ptr(),
                                        K, N, H * W, 0, 0, ws.data_ptr(), nws, st)
    else:
        scale, shift = lazy
        coef = torch.cat([scale, shift, torch.full((C,), 0.01)]).to(dev())      # rows (scale, shift, slope), one group
        li = PpLazyIn(coef.data_ptr(), C, 1)
        lib.pp_conv1x1_nhwc_to_nchw_fwd_lazy(xd.data_ptr(), C, C, wd.data_ptr(), bd.data_ptr(), logits.data_ptr(), K, N, H * W, li, st)
        lib.pp_conv1x1_nchw_to_nhwc_bwd_lazy(dld.data_ptr(), xd.data_ptr(), C, C, wd.data_ptr(), dx.data_ptr(), C, dw.data_ptr(),
                                             db.data_ptr(), K, N, H * W, 0, 0, ws.data_ptr(), nws, li, st)
    torch.cuda.synchronize()
    return logits, dx, dw, db


@pytest.mark.parametrize('K', WIDE_K)
@pytest.mark.parametrize('storage', ['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('C,N,H,W', [(32, 2, 24, 20), (32, 1, 9, 7), (64, 2, 16, 16), (128, 1, 8, 8), (12, 2, 5, 7)])
@pytest.mark.parametrize('lazy', [False, True])
def test_head_wide(K, storage, C, N, H, W, lazy):
    """Forward and backward of the 1x1 head (network head and auxiliary classifier) at K > 8: the LDS-tiled forms (C / 4 < K, or C / 4
    not a power of two) and, at C = 64 / 128, the streaming forward.  The reference is fp64 on the activation as stored."""
    x, w, b, dl = _head_inputs(C, K, N, H, W, K + C)
    x = x.to(_ACT[storage]).float()                                      # the operand as the device reads it
    lz = _lazy_rows(C, N, K) if lazy else None
    xr = x.double().requires_grad_(True)
    xin = F.leaky_relu(xr * lz[0].double().view(1, C, 1, 1) + lz[1].double().view(1, C, 1, 1), 0.01) if lazy else xr
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.conv2d(xin, wr, br)
    yr.backward(dl.double())
    logits, dx, dw, db = _head_device(storage, x, w, b, dl, lz)
    assert rel(logits, yr) < 1e-5
    assert rel(dw, wr.grad.view(K, C)) < 1e-5
    assert rel(db, br.grad) < 1e-5
    if not lazy:                                                         # lazy: dx is the gradient wrt the normalised activation
        ref_dx = F.conv2d(dl.double(), wr.detach().view(K, C).t().reshape(C, K, 1, 1))
        tol = 1e-5 if storage == 'fp32' else 1e-2                        # dx is rounded to the storage type on its store
        assert rel(dx.float().permute(0, 3, 1, 2), ref_dx) < tol


@pytest.mark.parametrize('K', [33, 64])
def test_over_32_classes_is_an_argument_error(K):
    from pacingpseudo_amd._lib import HipLibraryError
    lib, st = _lib()
    z = torch.zeros(1, K, 4, 4, device=dev())
    t = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev())
    sums = torch.zeros(6, dtype=torch.float64, device=dev())
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev())
    with pytest.raises(HipLibraryError, match=r'K=%d \(1\.\.32\)' % K):
        lib.pp_seg_losses_fwd(z.data_ptr(), None, t.data_ptr(), None, 1, K, 16, K, 0, 0, sums.data_ptr(), ws.data_ptr(), 1 << 16, st)
    x = torch.zeros(1, 4, 4, 32, device=dev())
    w = torch.zeros(K, 32, device=dev())
    with pytest.raises(HipLibraryError, match=r'K=%d \(1\.\.32\)' % K):
        lib.pp_conv1x1_nhwc_to_nchw_fwd(x.data_ptr(), 32, 32, w.data_ptr(), None, z.data_ptr(), K, 1, 16, st)
    with pytest.raises(HipLibraryError, match=r'K=%d \(1\.\.32\)' % K):
        lib.pp_dice_counts(z.data_ptr(), z.data_ptr(), 1, K, 16, z.data_ptr(), st)


# ---------------------------------------------------------------- the whole step
@pytest.mark.parametrize('K,H,W,bn_eval', [(17, 64, 64, False), (17, 64, 64, True), (32, 48, 40, False)])
def test_step_wide(K, H, W, bn_eval):
    """The full-flags step of test_gpu_step.py::test_other_datasets_shapes at K > 8: logits, losses and every parameter gradient
    against the oracle (LeakyReLU branch choices aligned with the device's)."""
    from pacingpseudo_amd.optim import FusedAdam
    args = O.full_flags(num_classes=K, ignored_index=K, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    torch.manual_seed(2)
    model = build_model(args)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batch = O.synthetic_batch(3, H, W, num_classes=K, seed=9, keep=0.08)
    batch['valid_mask'][:, :, :, :5] = 0
    opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
    training = not bn_eval
    if bn_eval:
        model.eval()
    ref_out, _, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 3, args, training=training)
    rec, grads = iteration(model, opt, batch, args, 3)
    assert rec['segmentation/logits'].shape[1] == K
    for k, v in ref_out.items():
        if k.startswith('_') or not torch.is_tensor(v):
            continue
        e = G.rel_err(rec[k].double().cpu().numpy(), v.numpy())
        assert e < TOL_OUT, f'{k}: rel err {e:.3e}'
    _, og, _ = oracle_with_device_branches(model, sd, batch, 3, args, training)
    check_grads(grads, {k: v.numpy() for k, v in og.items() if v is not None}, training)


def test_bf16_storage_step_at_17_classes():
    """--storage bf16 at K = 17 against the oracle rounded at the plan's storage sites (test_gpu_h16_oracle.py's check)."""
    from tests.test_gpu_h16_oracle import TOL_GRAD as TG, TOL_LOGITS, TOL_LOSS, _device_step, _errors, _oracle_step, _setup, rounding_for
    kind, bn_eval = 'bf16', False
    args, model, sd, batch = _setup(kind, 128, 17, bn_eval)
    dev_out, dev_grads = _device_step(model, batch, args)
    rounding = rounding_for(model, kind, True)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, max(threads, 8)))
    try:
        r_out, r_grads, _ = _oracle_step(model, sd, batch, args, True, rounding)
    finally:
        torch.set_num_threads(threads)
    er = _errors(dev_out, dev_grads, r_out, r_grads, True)
    m = (kind, bn_eval)
    for k in ('segmentation/logits', 'segmentation/logits_strong', 'logits_aux_cls'):
        assert er[k] < TOL_LOGITS[m], (k, er[k])
    for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'):
        assert er[k] < TOL_LOSS[m], (k, er[k])
    assert er['grad_worst'] < TG[m], (er['grad_worst'], er['grad_worst_key'])


def test_graph_replay_at_17_classes_equals_eager():
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    from tests.test_gpu_graph import _eager_step, _loss_fn
    K = 17
    args = O.full_flags(num_classes=K, ignored_index=K, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    f = _loss_fn(args)
    batches = [{k: v.cuda() for k, v in O.synthetic_batch(2, 64, 64, num_classes=K, seed=s, keep=0.05).items() if k != 'label'}
               for s in (3, 4)]
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
            losses.append(_eager_step(model, opt, f, b, 0) if gs is None else gs(b, 0)[0].detach().clone())
        torch.cuda.synchronize()
        runs[tag] = dict(losses=torch.stack(losses).cpu(), params=model.flat.params.clone(),
                         state={k: v.detach().clone() for k, v in model.state_dict().items()})
    e, g = runs['eager'], runs['graph']
    assert torch.isfinite(e['losses']).all()
    assert torch.equal(e['losses'], g['losses']) and torch.equal(e['params'], g['params'])
    for k, v in e['state'].items():
        assert torch.equal(v, g['state'][k]), k


def test_upper_bound_step_at_17_classes():
    """upper_bound_chaos.py's loss (partial CE + soft Dice) on a bare UNet at K = 17 against O.upper_bound_losses, gradients included."""
    from pacingpseudo_amd.losses.losses import dice_loss_fn, partial_cross_entropy_loss
    from pacingpseudo_amd.models import UNet
    from tests.test_gpu_step import device_masks, device_pool_winners
    K = 17
    args = O.default_args(init_ch=8, max_ch=64, num_classes=K, ignored_index=K)
    torch.manual_seed(4)
    net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, is_stride_conv=False,
               is_trans_conv=False, elab_end_points=True).cuda()
    batch = O.synthetic_batch(2, 64, 64, num_classes=K, seed=8)
    image, label = batch['image'], batch['label']
    sd = {'backbone.' + k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    logits = net(image.cuda())['segmentation/logits']
    loss_ce = partial_cross_entropy_loss(logits, label.cuda().argmax(1).long(), K)
    loss_dice = dice_loss_fn(logits, label.cuda())
    net.zero_grad()
    (loss_ce + loss_dice).backward()
    grads = {'backbone.' + k: p.grad.detach().clone() for k, p in net.named_parameters()}
    fake = type('M', (), {'engine': net._engine})()
    O.MASKS, O.POOLS = device_masks(fake), device_pool_winners(fake)
    try:
        keys = list(O.trainable_keys(sd))
        for k in keys:
            sd[k].requires_grad_(True)
        O._CALLS.clear()
        ref = O.upper_bound_losses(sd, image, label, args, True)
        (ref['loss_ce'] + ref['loss_dice']).backward()
    finally:
        O.MASKS = O.POOLS = None
    assert logits.shape[1] == K
    assert G.rel_err(logits.detach().double().cpu().numpy(), ref['segmentation/logits'].detach().numpy()) < TOL_OUT
    assert abs(float(loss_ce) - float(ref['loss_ce'])) < 1e-5 and abs(float(loss_dice) - float(ref['loss_dice'])) < 1e-5
    check_grads(grads, {k: sd[k].grad.numpy() for k in keys if sd[k].grad is not None}, True)


# ---------------------------------------------------------------- drivers, end to end on synthetic data
def test_drivers_at_17_classes(tmp_path):
    import json
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'out')
    vd = train_main(['--tag', 'k17', '--session', 'Experiment', '--root', root, '--synthetic', '16', '--num_classes', '17',
                     '--ignored_index', '17', '--epoch', '2', '--batch_size', '4', '--image_size', '64', '--num_workers', '0',
                     '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path', '--do_memory'])
    assert vd.shape == (2,) and np.isfinite(vd).all()
    run = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-k17'))
    assert len(run) == 1
    for f in ('log.txt', 'valdice.npz', 'ckps/ckp_1.pth'):
        assert os.path.exists(os.path.join(run[0], f)), f
    log = open(os.path.join(run[0], 'log.txt')).read()
    assert 'num_classes=17' in log and 'C16' in log and 'nan' not in log.split('val: 001')[0].lower()
    tags = {json.loads(x)['tag'] for x in open(os.path.join(run[0], 'tb_summary', 'scalars.jsonl'))}
    assert {'DSC/BG', 'DSC/C5', 'DSC/C16', 'DSC/All'} <= tags
    sd = torch.load(os.path.join(run[0], 'ckps', 'ckp_1.pth'), map_location='cpu')
    assert sd['backbone.final_conv.weight'].shape[0] == 17 and sd['aux_path.memory_bank'].shape[0] == 17
    ckp = os.path.join(run[0], 'ckps', 'ckp_1.pth')
    common = ['--fold', '1', '--checkpoint_file', ckp, '--root', str(tmp_path / 'inf'), '--dataset', 'chaost1', '--synthetic', '6',
              '--image_size', '64', '--batch_size', '4', '--num_workers', '0']
    dicearr, hd95arr = I.main(common + ['--num_classes', '17'])
    assert dicearr.shape == (6, 17) and hd95arr.shape == (6, 17)
    with pytest.raises(ValueError, match='--num_classes 17'):
        I.main(common + ['--num_classes', '5'])
    # the fully supervised trainer with the same class count
    from pacingpseudo_amd.upper_bound import train_main as ub_main
    ub = ub_main(['--tag', 'ub17', '--session', 'Experiment', '--root', str(tmp_path / 'ub'), '--synthetic', '16', '--num_classes', '17',
                  '--ignored_index', '17', '--epoch', '2', '--batch_size', '4', '--image_size', '64', '--num_workers', '0', '--cpu_input'])
    assert np.isfinite(np.asarray(ub)).all()
