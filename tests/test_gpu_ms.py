"""The Mumford-Shah level-set loss (--do_loss_ms, pp_ms_loss_*, losses.mumford_shah_loss) on the MI355X against the float64 comparison
functions of tests/_ms_reference.py (the direct definition, differentiated by autograd).

Bounds: the project's existing ones -- the loss within 1e-5 * max(1, |L|), S and mu within 1e-6 relative per entry (they are summed in
double; the test images are positive, so a mean has its own value as its scale), gradients rel < TOL = 1e-4 in the `rel` measure of
tests/test_gpu_ops.py.  sign() is discontinuous: a pixel that touches a neighbour pair with 0 < |dp| <= 1e-5 * max(p_i, p_j) in the
float64 reference (about 80 fp32 ulps) is left out of the GRADIENT comparison, and the share of such pixels is asserted (0.5 % per
kernel case, 1 % in a whole step); the loss value is compared on all pixels.  An fp32 evaluation of the analytic form on the CPU with
S and the means accumulated in double stays within 1e-8 (loss), 5.3e-8 (S), 8.8e-9 (mu) and 1.5e-6 (gradient) of the float64 values
on the kernel cases below, so the bounds hold with more than 18x of room; nothing here is fitted to what the kernels give.
"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _crf_reference as RC  # noqa: E402
from tests import _ms_reference as R  # noqa: E402
from tests import _nc_reference as RN  # noqa: E402
from tests.test_gpu_ops import TOL, rel  # noqa: E402
from tests.test_gpu_step import build_model  # noqa: E402

NAN = float('nan')


def _kernel(z, x, m, lam=1.0, g_up=1.0, loss_scale=1.0, prefill=None, need_grad=True):
    """pp_ms_loss_fwd (+ the device-side finalize) and pp_ms_loss_bwd on CUDA copies: (loss, dlogits, sums, stats, unit).  Workspace,
    unit gradient and stats start as NaN: an entry nobody wrote shows in what is read from them."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    z, x = z.float().cuda().contiguous(), x.float().cuda().contiguous()
    m = m.float().cuda().contiguous() if m is not None else None
    N, K, H, W = z.shape
    C = x.shape[1]
    st = stream_ptr()
    sums = torch.full((4,), NAN, device='cuda', dtype=torch.float64)
    stats = torch.full((N, K, 1 + C), NAN, device='cuda', dtype=torch.float64)
    nws = lib.pp_ms_loss_workspace(N, K, C, H, W)
    ws = torch.full(((nws + 7) // 8,), NAN, device='cuda', dtype=torch.float64)
    unit = torch.full_like(z, NAN) if need_grad else None
    has_mask = 1 if m is not None else 0
    lib.pp_ms_loss_fwd(z.data_ptr(), x.data_ptr(), m.data_ptr() if m is not None else None, N, K, C, H, W, lam,
                       unit.data_ptr() if need_grad else None, stats.data_ptr(), sums[2:].data_ptr(), ws.data_ptr(), nws, st)
    loss = torch.empty((), device='cuda')
    lib.pp_losses_finalize(sums.data_ptr(), has_mask, None, loss.data_ptr(), None, st)
    dz = None
    if need_grad:
        dz = torch.zeros_like(z) if prefill is None else prefill.float().cuda().clone()
        g = torch.tensor(g_up, device='cuda', dtype=torch.float32)
        lib.pp_ms_loss_bwd(unit.data_ptr(), sums[2:].data_ptr(), has_mask, g.data_ptr(), loss_scale, dz.data_ptr(), z.numel(), st)
    torch.cuda.synchronize()
    return loss.cpu(), (dz.cpu() if dz is not None else None), sums.cpu(), stats.cpu(), (unit.cpu() if need_grad else None)


def _inputs(N, K, C, H, W, seed, masked, scale=2.0):
    """Logits 2 N(0,1), an image whose intensity offset differs from image to image, a 70 % mask."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, K, H, W, generator=g) * scale
    x = R.offset_image(N, C, H, W, seed=seed + 1)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    return z, x, m


_REF = {}


def _reference(tag, z, x, m, lam):
    """Float64 (loss, gradient, unit gradient, S, mu, ambiguous pixels) at the fp32 inputs the kernel sees: computed once per case,
    shared, never modified."""
    if tag not in _REF:
        loss, grad = R.ms_loss_and_grad(z.float(), x.float(), m, lam)
        _, _, u, _ = R.ms_analytic_form(z.float(), x.float(), m, lam)
        S, mu, _ = R.ms_stats(z.float(), x.float(), m)
        _REF[tag] = (loss, grad, u, S, mu, R.ambiguous_pixels(z.float(), m))
    return _REF[tag]


def _keep(amb, cap, tag):
    """The pixels the gradient comparison keeps, (N,1,H,W); fails by name when the reference leaves out more than `cap` of them."""
    share = float(amb.double().mean())
    assert share <= cap, f'{tag}: {int(amb.sum())} of {amb.numel()} pixels ({share:.2%}) are sign-ambiguous in the float64 reference (cap {cap:.1%})'
    return (~amb)[:, None].double()


def _check(tag, z, x, m, lam=1.0, grad_on_all=False):
    ref_loss, ref_grad, ref_u, S, mu, amb = _reference(tag, z, x, m, lam)
    loss, dz, sums, stats, unit = _kernel(z, x, m, lam)
    N, K, H, W = z.shape
    if grad_on_all:
        assert int(amb.sum()) == 0, tag
    keep = _keep(amb, 0.005, tag)
    e_loss = abs(float(loss) - float(ref_loss))
    e_grad, e_unit = rel(dz.double() * keep, ref_grad * keep), rel(unit.double() * keep, ref_u * keep)
    assert float(S.min()) > 1e-3 and float(mu.min()) > 0.3, tag           # every entry has a scale of its own, no class near S_MIN
    e_s = float(((stats[..., 0] - S).abs() / S).max())
    e_mu = float(((stats[..., 1:] - mu).abs() / mu).max())
    print(f'{tag}: loss {float(loss)!r} ref {float(ref_loss)!r} (|diff| {e_loss:.2e}), gradient rel {e_grad:.2e}, unit rel {e_unit:.2e}, '
          f'max |grad| {float(ref_grad.abs().max()):.3e}, S rel {e_s:.2e}, mu rel {e_mu:.2e}, left out {int(amb.sum())} pixels')
    assert torch.isfinite(loss) and torch.isfinite(dz).all() and torch.isfinite(stats).all() and torch.isfinite(unit).all(), tag
    D = float(m.sum()) if m is not None else float(N * H * W)
    assert sums[3].item() == D, (tag, sums.tolist())
    assert e_loss <= 1e-5 * max(1.0, abs(float(ref_loss))), (tag, float(loss), float(ref_loss))
    assert e_s <= 1e-6 and e_mu <= 1e-6, (tag, e_s, e_mu)
    assert e_grad < TOL and e_unit < TOL, (tag, e_grad, e_unit)
    return float(ref_loss), ref_grad


# (N, K, C, H, W): ragged 32 x 8 tiles, widths that are no multiple of 4 (the scalar forms), single rows and columns, every
# class-count regime, K = 1
SHAPES = [(2, 5, 1, 24, 40), (3, 2, 1, 7, 70), (2, 17, 3, 13, 66), (1, 32, 4, 9, 65), (2, 4, 1, 1, 130), (2, 9, 2, 67, 1), (1, 1, 1, 8, 64)]


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', SHAPES, ids=['-'.join(map(str, s)) for s in SHAPES])
def test_kernel_against_float64(shape, masked):
    N, K, C, H, W = shape
    z, x, m = _inputs(N, K, C, H, W, seed=SHAPES.index(shape), masked=masked)
    ref_loss, ref_grad = _check(f'{shape}{" masked" if masked else ""}', z, x, m)
    if K > 1:
        assert ref_loss > 0.05 and float(ref_grad.abs().max()) > 0            # not a vacuous case
    else:
        assert float(ref_grad.abs().max()) == 0.0                            # one class: no TV, no gradient; the level-set term remains
        assert ref_loss > 0
    if N > 1:                                                                # the means are per image: the offsets show
        mu = _REF[f'{shape}{" masked" if masked else ""}'][4]
        assert float((mu[1] - mu[0]).min()) > 0.3


def test_other_tv_weights():
    """tv_weight 0 (the level-set term alone) and a fraction: the weight reaches both the energy and the gradient."""
    z, x, m = _inputs(2, 5, 1, 24, 40, seed=0, masked=True)
    l0, _ = _check('tv 0', z, x, m, lam=0.0)
    l3, _ = _check('tv 0.3', z, x, m, lam=0.3)
    assert l3 > 1.5 * l0 > 0


def test_flat_regions():
    """Logits constant on 4 x 4 blocks whose edges never fall on a tile edge: inside a block dp = 0 exactly and sign(0) = 0.  Every
    pixel is compared: a pixel whose probabilities depended on where it is staged (interior, halo, next tile) would grow a sign."""
    g = torch.Generator().manual_seed(25)
    zb = torch.randn(2, 5, 11, 19, generator=g) * 2
    z = zb.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, 2:39, 3:73].contiguous()       # block edges at y = 2, x = 1 (mod 4)
    x = R.offset_image(2, 1, 37, 70, seed=3)
    p = R._softmax(z)
    assert float(((p[..., 1:] - p[..., :-1]) == 0).double().mean()) > 0.7     # three of four horizontal pairs lie inside a block
    for tag, m in (('flat', None), ('flat masked', (torch.rand(2, 1, 37, 70, generator=g) < 0.7).float())):
        _check(tag, z, x, m, grad_on_all=True)


@pytest.mark.parametrize('K', [5, 17])
def test_sharp_predictions(K):
    """Logits scaled by 30: most probabilities are 0 or 1 to fp32.  The loss value holds its bound and the gradient is finite; the
    sign rule would leave out most pixels here (differences of two values next to 0), and the gradient is about 0 there anyway."""
    z, x, m = _inputs(2, K, 1, 24, 40, seed=5 + K, masked=True, scale=60.0)
    ref_loss, _ = R.ms_loss_and_grad(z, x, m)
    loss, dz, sums, stats, unit = _kernel(z, x, m)
    print(f'sharp K={K}: loss {float(loss)!r} float64 {float(ref_loss)!r}')
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    assert torch.isfinite(dz).all() and torch.isfinite(unit).all() and torch.isfinite(stats).all()


def test_edge_inputs():
    """An all-zero mask in one image: its classes are inactive (S = 0, mu = 0), loss and gradient stay finite and right; an all-zero
    mask everywhere: the loss is 0 (0 / max(0, 1e-8)) and so is the gradient."""
    z, x, m = _inputs(2, 5, 1, 24, 40, seed=4, masked=True)
    m[1] = 0
    ref_loss, ref_grad = R.ms_loss_and_grad(z, x, m)
    loss, dz, sums, stats, unit = _kernel(z, x, m)
    assert int(R.ambiguous_pixels(z, m).sum()) == 0
    assert float(stats[1].abs().max()) == 0.0 and float(stats[0, :, 0].min()) > 1.0
    assert torch.isfinite(loss) and torch.isfinite(dz).all()
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss))) and float(ref_loss) > 0.05
    assert rel(dz, ref_grad) < TOL and float(dz[1].abs().max()) == 0.0
    loss, dz, sums, stats, unit = _kernel(z, x, torch.zeros_like(m))
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and sums[2:].tolist() == [0.0, 0.0] and float(stats.abs().max()) == 0.0


def test_backward_accumulates_and_scales():
    """dlogits is pre-filled, loss_scale and the upstream gradient differ from 1: dlogits = prefill + loss_scale * g_up * dL/dz."""
    z, x, m = _inputs(2, 5, 1, 24, 40, seed=0, masked=True)
    _, ref_grad, _, _, _, amb = _reference(f'{SHAPES[0]} masked', z, x, m, 1.0)
    assert int(amb.sum()) == 0
    inc = 1024.0 * 0.37 * ref_grad
    pre = torch.randn(z.shape, generator=torch.Generator().manual_seed(1)) * float(inc.abs().max())      # of the increment's size
    _, dz, _, _, _ = _kernel(z, x, m, g_up=0.37, loss_scale=1024.0, prefill=pre)
    e = rel(dz.double() - pre.double(), inc)
    print(f'accumulate: rel {e:.2e}')
    assert e < TOL
    # forward only: no unit-gradient buffer, the same sums and stats
    a = _kernel(z, x, m)
    b = _kernel(z, x, m, need_grad=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][2:], b[2][2:]) and torch.equal(a[3], b[3]) and b[1] is None


def test_bit_reproducible():
    for K, masked in ((5, True), (17, False)):
        z, x, m = _inputs(2, K, 3, 70, 132, seed=K, masked=masked)
        a, b = _kernel(z, x, m), _kernel(z, x, m)
        assert all(torch.equal(a[i], b[i]) for i in (0, 1, 3, 4)) and torch.equal(a[2][2:], b[2][2:]), K
        assert float(a[1].abs().max()) > 0


def test_argument_checks():
    """Every bad argument is refused before a launch: an error code, and the NaN-filled outputs stay as they were."""
    from pacingpseudo_amd._lib import HipLibraryError, lib, stream_ptr
    z, x = torch.zeros(1, 5, 8, 8, device='cuda'), torch.ones(1, 1, 8, 8, device='cuda')
    nws = lib.pp_ms_loss_workspace(1, 5, 1, 8, 8)
    # 1 block x 5 classes x 2 doubles | 1 tile x 2 doubles | 5 x 5 floats
    assert nws == 5 * 2 * 8 + 2 * 8 + 25 * 4 and lib.pp_ms_loss_workspace(0, 5, 1, 8, 8) == 0
    sums = torch.full((2,), NAN, device='cuda', dtype=torch.float64)
    stats = torch.full((1, 5, 2), NAN, device='cuda', dtype=torch.float64)
    unit = torch.full((1, 5, 8, 8), NAN, device='cuda')
    ws = torch.zeros(nws + 16, device='cuda', dtype=torch.uint8)

    def call(K=5, C=1, lam=1.0, nbytes=nws, zp=z.data_ptr(), sp=stats.data_ptr(), wsp=ws.data_ptr()):
        lib.pp_ms_loss_fwd(zp, x.data_ptr(), None, 1, K, C, 8, 8, lam, unit.data_ptr(), sp, sums.data_ptr(), wsp, nbytes, stream_ptr())
    for kw in (dict(K=0), dict(K=33), dict(C=0), dict(C=5), dict(lam=-1.0), dict(lam=float('nan')), dict(lam=float('inf')), dict(zp=None),
               dict(sp=None), dict(wsp=ws.data_ptr() + 4)):
        with pytest.raises(HipLibraryError, match='ms_loss_fwd'):
            call(**kw)
    with pytest.raises(HipLibraryError, match='workspace too small'):
        call(nbytes=nws - 1)
    g = torch.ones((), device='cuda')
    for up, n in ((unit.data_ptr(), 0), (None, 320)):
        with pytest.raises(HipLibraryError, match='ms_loss_bwd'):
            lib.pp_ms_loss_bwd(up, sums.data_ptr(), 0, g.data_ptr(), 1.0, unit.data_ptr(), n, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(sums).all() and torch.isnan(stats).all() and torch.isnan(unit).all()
    call()                                                                 # and the good call goes through
    torch.cuda.synchronize()
    # constant logits and image: p = 1/5, mu = 1, no energy and no gradient at all
    assert sums.tolist() == [0.0, 64.0] and float(unit.abs().max()) == 0.0
    assert float((stats.cpu() - torch.tensor([12.8, 1.0], dtype=torch.float64)).abs().max()) <= 1e-6


def test_functional_mumford_shah_loss():
    """losses.mumford_shah_loss stand-alone: value and gradient against float64, scaled upstream gradient, argument checks."""
    from pacingpseudo_amd.losses import mumford_shah_loss
    z, x, m = _inputs(2, 4, 3, 20, 24, seed=21, masked=True)
    for mask in (None, m):
        zc = z.cuda().requires_grad_(True)
        loss = mumford_shah_loss(zc, x.cuda(), mask.cuda() if mask is not None else None, tv_weight=0.5)
        (loss * 2.5).backward()
        ref_loss, ref_grad = R.ms_loss_and_grad(z, x, mask, 0.5)
        keep = _keep(R.ambiguous_pixels(z, mask), 0.005, 'functional')
        assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
        assert float(ref_grad.abs().max()) > 0 and rel(zc.grad.cpu().double() * keep, 2.5 * ref_grad * keep) < TOL
    with torch.no_grad():
        assert float(mumford_shah_loss(z.cuda(), x.cuda())) > 0.05             # defaults; no gradient buffer without a graph
    with pytest.raises(ValueError, match='Mumford-Shah'):
        mumford_shah_loss(z.cuda(), x.cuda(), tv_weight=-1.0)
    with pytest.raises(NotImplementedError, match='Mumford-Shah'):
        mumford_shah_loss(z.cuda(), torch.zeros(2, 5, 20, 24, device='cuda'))
    with pytest.raises(NotImplementedError, match='Mumford-Shah'):
        mumford_shah_loss(torch.zeros(1, 33, 4, 4, device='cuda'), torch.zeros(1, 1, 4, 4, device='cuda'))
    with pytest.raises(ValueError):
        mumford_shah_loss(z.cuda(), x.cuda()[:, :, :10])
    with pytest.raises(ValueError):
        mumford_shah_loss(z.cuda(), x.cuda(), valid_mask=torch.ones(2, 4, 20, 24, device='cuda'))
    with pytest.raises(TypeError):
        mumford_shah_loss(z, x)                                               # CPU tensors


# ---------------------------------------------------------------------------------------------------------------- whole step
# At unit weight the gradient of this loss is u / D with |u| up to a few (four signs times p) and D = B H W: about 1e-4 per logit at
# these shapes, below the partial cross entropy's 1 / (scribble pixels) ~ 6e-4.  The tests weigh it by W_MS and ASSERT its share of
# the max-norm on the float64 gradients.
W_MS = 10.0
W_NC = 30.0
W_CRF = 3.0
PRM = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)


def _ms_flags(**over):
    return O.full_flags(do_loss_ms=True, ms_tv_weight=1.0, **over)


def _step_batch(B, size, seed=3):
    b = O.synthetic_batch(B, size, size, seed=seed, keep=0.05)
    b['image'] = R.offset_image(B, 1, size, size, seed=seed)                 # smooth + a fixed pseudo-random component: neighbours differ
    b['image_strong'] = b['image'] * 1.3 - 0.2
    b['valid_mask'][0, :, :9] = 0
    b['valid_mask'][1, :, :, -5:] = 0
    return {k: v.cuda() for k, v in b.items() if k != 'label'}


def _assembled(args, out, epoch):
    w = O.loss_weights(args, epoch)
    total = sum(out[k] * wt for k, wt in w.items()) + out['loss_ms'] * W_MS
    if getattr(args, 'do_loss_crf', False):
        total = total + out['loss_crf'] * W_CRF
    if getattr(args, 'do_loss_nc', False):
        total = total + out['loss_nc'] * W_NC
    return total, w


def _oracle_dlogits(args, batch, zw, zs, w, with_others):
    """The float64 gradients of the assembled loss with respect to the weak logits, at the device's logits, term by term:
    {'rest': pce + w_ent ent + w_cr cr, 'ms': W_MS ms, 'crf': W_CRF crf, 'nc': W_NC nc}, and the float64 loss values."""
    zw = zw.detach().double().cpu().requires_grad_(True)
    zs = zs.detach().double().cpu()
    mask = batch['valid_mask'].cpu()
    target = batch['scribble'].cpu().argmax(1).long()
    rest = O.partial_cross_entropy_loss(zw, target, args.ignored_index)
    rest = rest + w['loss_ent'] * O.entropy_minimization_loss(zw, mask.double())
    rest = rest + w['loss_cr'] * O.soft_label_cross_entropy_loss(zs, torch.softmax(zw, 1), mask.double())
    ms = R.ms_loss_direct(zw, batch['image'].cpu(), mask, args.ms_tv_weight)
    g = {'rest': torch.autograd.grad(rest, zw)[0], 'ms': W_MS * torch.autograd.grad(ms, zw)[0]}
    vals = {'ms': ms.detach()}
    if with_others:
        crf = RC.crf_loss_direct(zw, batch['image'].cpu(), mask, **PRM)
        g['crf'] = W_CRF * torch.autograd.grad(crf, zw)[0]
        nc = RN.nc_loss_direct(zw, batch['image'].cpu(), mask, **PRM)
        g['nc'] = W_NC * torch.autograd.grad(nc, zw)[0]
        vals.update(crf=crf.detach(), nc=nc.detach())
    return g, vals


def _whole_step(storage, with_others):
    over = {}
    if with_others:
        over = dict(do_loss_crf=True, do_loss_nc=True, **{f'crf_{k}': v for k, v in PRM.items()}, **{f'nc_{k}': v for k, v in PRM.items()})
    args = _ms_flags(**over)
    args.storage = storage
    torch.manual_seed(1)
    model = build_model(args)
    model.train()
    B = 2
    batch = _step_batch(B, 128)
    out = model(batch, mode='train', step=37)
    keys = list(out)
    assert keys == model._expected_keys('train') and 'loss_ms' in out
    if with_others:
        i = keys.index('segmentation/logits_strong')
        assert keys[i + 1:i + 4] == ['loss_crf', 'loss_nc', 'loss_ms']
    else:
        assert keys[keys.index('loss_ms') - 1] == 'segmentation/logits_strong'
    total, w = _assembled(args, out, 37)
    total.backward()
    torch.cuda.synchronize()
    plan = model.engine.last_plan
    scale = plan.loss_scale
    s0 = 10 if with_others else 6
    assert plan.all_sums.numel() == s0 + 4 and plan.regs['ms'].sums.data_ptr() == plan.all_sums[s0:].data_ptr()
    assert plan.aux['sums'].data_ptr() == plan.all_sums[s0 + 2:].data_ptr()
    if with_others:
        assert plan.regs['crf'].sums.data_ptr() == plan.all_sums[6:].data_ptr() and plan.regs['nc'].sums.data_ptr() == plan.all_sums[8:].data_ptr()
    zw = out['segmentation/logits']
    g, vals = _oracle_dlogits(args, batch, zw, out['segmentation/logits_strong'], w, with_others)
    tag = f'{storage}{" + crf + nc" if with_others else ""}'
    amb = R.ambiguous_pixels(zw.detach().cpu(), batch['valid_mask'].cpu())
    keep = _keep(amb, 0.01, tag)
    ref_g = sum(g.values()) * keep
    got_g = plan.dlogits[:B].detach().cpu().double() * keep
    got = float(out['loss_ms'])
    e = rel(got_g, scale * ref_g)
    share = {k: float((v * keep).abs().max() / ref_g.abs().max()) for k, v in g.items()}
    print(f'{tag}: loss_ms {got!r} float64 {float(vals["ms"])!r}; dlogits[:B] rel {e:.2e} at loss scale {scale}; left out {int(amb.sum())} of '
          f'{amb.numel()} pixels; max |gradient| of each term / of the sum {share}; max |d ms| at unit weight {float(g["ms"].abs().max()) / W_MS:.3e}')
    assert float(vals['ms']) > 0.01
    assert share['ms'] >= 0.1                                            # the term is visible in a max-norm comparison
    assert abs(got - float(vals['ms'])) <= 1e-5 * max(1.0, abs(float(vals['ms'])))
    assert e < TOL
    for k in g:                                                          # every term is IN the gradient: without it the comparison fails
        if k != 'rest':
            assert rel(got_g, scale * (ref_g - g[k] * keep)) > 10 * TOL, k
    if with_others:
        assert abs(float(out['loss_crf']) - float(vals['crf'])) <= 1e-5 * max(1.0, abs(float(vals['crf'])))
        assert abs(float(out['loss_nc']) - float(vals['nc'])) <= 1e-5 * max(1.0, abs(float(vals['nc'])))
    return model, batch, args


@pytest.mark.parametrize('storage', ['fp32', 'bf16', 'fp16'])
def test_whole_step(storage):
    model, batch, args = _whole_step(storage, with_others=False)
    if storage == 'fp16':
        assert model.engine.last_plan.loss_scale == 1024.0
    # the loss moves the weights' gradients: not a term that is computed and dropped
    g_on = model.flat.grads.clone()
    out2 = model(batch, mode='train', step=37)
    sum(out2[k] * wt for k, wt in O.loss_weights(args, 37).items()).backward()
    torch.cuda.synchronize()
    assert not torch.equal(g_on, model.flat.grads)


def test_whole_step_with_the_crf_and_nc_losses_as_well():
    """All three regularisers on: keys in order, the three sums pairs at [6:8], [8:10], [10:12], every term in the gradient."""
    _whole_step('fp32', with_others=True)


def test_mask_applies_without_entropy_or_consistency():
    """--do_loss_ms alone: the batch's valid_mask still masks this loss (the partial CE has no mask)."""
    args = O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_ms=True)
    torch.manual_seed(2)
    model = build_model(args)
    model.train()
    batch = _step_batch(2, 64)
    batch['valid_mask'][:, :, 20:50, 10:40] = 0                              # a third of the pixels: the mask matters
    out = model(batch, mode='train', step=0)
    assert list(out) == ['segmentation/logits', 'loss_pce', 'loss_ms']
    (out['loss_pce'] + out['loss_ms']).backward()
    torch.cuda.synchronize()
    z = out['segmentation/logits'].detach().cpu()
    S, mu, _ = R.ms_stats(z, batch['image'].cpu(), batch['valid_mask'].cpu())
    S1, _, _ = R.ms_stats(z, batch['image'].cpu(), None)
    ref = R.ms_loss_direct(z, batch['image'].cpu(), batch['valid_mask'].cpu())
    plan = model.engine.last_plan
    st = plan.regs['ms'].state.cpu()
    # (the block always ends with the auxiliary pair's slot: 8 doubles without a regulariser, 10 with this one)
    assert plan.all_sums.numel() == 10 and plan.regs['ms'].sums.data_ptr() == plan.all_sums[6:].data_ptr()
    assert float(((S1 - S) / S1).min()) > 0.1                               # the masked sums are not the unmasked ones ...
    assert float(((st[..., 0] - S).abs() / S).max()) <= 1e-6 and float(((st[..., 1:] - mu).abs() / mu).max()) <= 1e-6      # ... the device has the masked
    assert plan.all_sums[7].item() == float(batch['valid_mask'].sum())
    assert abs(float(out['loss_ms']) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    # train mode without a graph (no_grad): the loss is still evaluated, from a forward-only plan without a unit-gradient buffer
    with torch.no_grad():
        o = model(batch, mode='train', step=0)
    assert list(o) == ['segmentation/logits', 'loss_pce', 'loss_ms']
    assert abs(float(o['loss_ms']) - float(out['loss_ms'])) <= 1e-5 and model.engine.last_plan.regs['ms'].unit is None
    assert 'loss_ms' not in model(batch, mode='val')


def test_flag_off_is_the_parent_step():
    """do_loss_ms=False and a namespace without the attribute: the same keys, bit-identical losses, gradient slab and dlogits, and
    no buffer of this loss in the plan; the sums block keeps its 8 doubles (12 with the CRF and NC pairs)."""
    runs = {}
    for tag, args in (('absent', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])),
                      ('off', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_ms=False, ms_tv_weight=0.3))):
        torch.manual_seed(5)
        model = build_model(args)
        model.train()
        batch = _step_batch(2, 64)
        out = model(batch, mode='train', step=3)
        sum(out[k] * wt for k, wt in O.loss_weights(args, 3).items()).backward()
        torch.cuda.synchronize()
        plan = model.engine.last_plan
        assert 'ms' not in model.engine.regs and not plan.regs and plan.all_sums.numel() == 8
        assert plan.aux['sums'].data_ptr() == plan.all_sums[6:].data_ptr()
        runs[tag] = (list(out), {k: v.detach().clone() for k, v in out.items()}, model.flat.grads.clone(), plan.dlogits.clone())
    a, b = runs['absent'], runs['off']
    assert a[0] == b[0] and 'loss_ms' not in a[0]
    for k in a[0]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    both = O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_crf=True, do_loss_nc=True, do_loss_ms=False)
    model = build_model(both)
    model.train()
    out = model(_step_batch(2, 64), mode='train', step=3)
    assert 'loss_ms' not in out and model.engine.last_plan.all_sums.numel() == 12 and 'ms' not in model.engine.last_plan.regs


def test_engine_rejects_bad_parameters_before_a_launch():
    for kw, err in ((dict(ms_tv_weight=-1.0), ValueError), (dict(ms_tv_weight=float('nan')), ValueError)):
        with pytest.raises(err, match='Mumford-Shah'):
            build_model(O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_ms=True, **kw))


def test_graph_replay_equals_eager_with_the_loss_on():
    """Eager vs GraphedStep over three iterations with the loss on (full flags): loss, parameters and Adam moments bit for bit."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = _ms_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])

    def loss_fn(out, epoch):
        return _assembled(args, out, epoch)[0]
    batch = _step_batch(2, 64)
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(3)
        model = build_model(args)
        model.train()
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=3e-4)
        gs = GraphedStep(model, opt, loss_fn, warmup=10 ** 9 if tag == 'eager' else 1)
        losses, mss = [], []
        for _ in range(3):
            loss, out = gs(batch, 0)
            losses.append(loss.detach().clone())
            mss.append(out['loss_ms'].detach().clone())
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(losses=torch.stack(losses).cpu(), mss=torch.stack(mss).cpu(), params=model.flat.params.clone(), m=sd['m'], v=sd['v'],
                         captures=gs.captures, replays=gs.replays)
    e, g = runs['eager'], runs['graph']
    print('losses', e['losses'].tolist(), 'loss_ms', e['mss'].tolist())
    assert e['captures'] == 0 and g['captures'] == 1 and g['replays'] == 2
    assert float(e['mss'].min()) > 0 and len(set(e['mss'].tolist())) == 3          # the weights move, and so does the loss
    for k in ('losses', 'mss', 'params', 'm', 'v'):
        assert torch.equal(e[k], g[k]), k


def test_driver_logs_the_loss(tmp_path):
    """train.py with the flag on, alone (ramped weight) and beside the other two regularisers: the epoch line gains its column behind
    theirs, scalars.jsonl its tag, and the column holds weight x loss."""
    import glob
    import json
    import re
    from pacingpseudo_amd.train import train_main
    common = ['--session', 'Experiment', '--synthetic', '8', '--epoch', '2', '--batch_size', '4', '--image_size', '64', '--num_workers', '0',
              '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path', '--do_memory']
    for tag, extra in (('ms', ['--do_loss_ms', '--ramp_up_loss_ms', '--ms_tv_weight', '0.5']),
                       ('all', ['--do_loss_ms', '--loss_ms_weight', '0.5', '--do_loss_crf', '--do_loss_nc', '--nc_radius', '3', '--crf_radius', '3'])):
        root = str(tmp_path / tag)
        train_main(['--tag', tag, '--root', root] + common + extra)
        run = glob.glob(os.path.join(root, 't1', 'Experiment', f'Experiment-*-fold1-{tag}'))[0]
        lines = [ln for ln in open(os.path.join(run, 'log.txt')) if 'loss_ms: ' in ln and 'epoch: ' in ln]
        assert len(lines) == 2, lines
        assert all(('loss_crf: ' in ln) == (tag == 'all') and ('loss_nc: ' in ln) == (tag == 'all') for ln in lines)
        if tag == 'all':
            assert all(ln.index('loss_crf: ') < ln.index('loss_nc: ') < ln.index('loss_ms: ') < ln.index('s/epoch') for ln in lines)
        sc = [json.loads(ln) for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))]
        vals = [r['value'] for r in sc if r['tag'] == 'train/loss_ms']
        assert len(vals) == 2 and (('train/loss_nc' in {r['tag'] for r in sc}) == (tag == 'all'))
        logged = [float(re.search(r'loss_ms: ([0-9.eE+-]+)', ln).group(1)) for ln in lines]
        assert all(abs(a - b) <= 1e-6 for a, b in zip(logged, vals))
        assert all(v > 0.0 for v in vals), vals                             # the meter holds weight x loss, both positive


# ---------------------------------------------------------------------------------------------------------------- data-parallel
def _rank(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    from pacingpseudo_amd import parallel
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group('gloo')
    args = _ms_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    torch.manual_seed(1)
    model = build_model(args)
    if world > 1:
        parallel.attach(model)
    model.eval()                                    # BatchNorm in eval mode: every sample independent of how the batch is split
    full = _step_batch(4, 64, seed=11)
    full['valid_mask'][3, :, 20:40] = 0             # the halves hold different numbers of valid pixels: D must be the global one
    nloc = 4 // world
    batch = {k: v[rank * nloc:(rank + 1) * nloc].contiguous() for k, v in full.items()}
    out = model(batch, mode='train', step=37)
    _assembled(args, out, 37)[0].backward()
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(dict(loss_ms=float(out['loss_ms']), D=float(model.engine.last_plan.regs['ms'].sums[1]), valid=float(full['valid_mask'].sum()),
                        grads=model.flat.grads.cpu()), out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _launch(world, out_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(PP_DIST_BACKEND='gloo', PP_SHARE_GPU='1', PP_HANG_DUMP='240')
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        procs = [mp.get_context('spawn').Process(target=_rank, args=(r, world, port, out_path)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            if p.is_alive():
                p.kill()
                p.join()
            assert p.exitcode == 0, f'rank process exit code {p.exitcode}'
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return torch.load(out_path)


def test_two_ranks_equal_one_process(tmp_path):
    """Two ranks on the one GPU (gloo), each with half of a masked batch: the energy and sum m travel in the all-reduced sums block,
    so both reach the single process's loss_ms (1e-5) and gradient slab (rel < 1e-4), with the GLOBAL D."""
    one = _launch(1, str(tmp_path / 'one.pt'))
    two = _launch(2, str(tmp_path / 'two.pt'))
    e = rel(two['grads'], one['grads'])
    print(f'loss_ms one process {one["loss_ms"]!r}, two ranks {two["loss_ms"]!r}; D {one["D"]} / {two["D"]}; gradient slab rel {e:.2e}')
    assert one['loss_ms'] > 0.01
    assert one['D'] == two['D'] == one['valid']
    assert abs(two['loss_ms'] - one['loss_ms']) <= 1e-5 * max(1.0, abs(one['loss_ms']))
    assert e < TOL
