"""The normalised-cut loss (--do_loss_nc, pp_nc_loss_*, losses.normalized_cut_loss) on the MI355X against the float64 comparison
function of tests/_nc_reference.py (the direct double sum, differentiated by autograd).

Bounds: the project's existing ones -- the loss within 1e-5 * max(1, |L|), gradients rel < TOL = 1e-4 in the `rel` measure of
tests/test_gpu_ops.py, A and V within 1e-6 relative per entry (they are summed in double).  An fp32 evaluation of the gather form with
A / V accumulated in double stays within 1.5e-9 / 3.7e-6 of the float64 values on the CPU, so loss and gradient bounds hold with
more than 25x of room; nothing here is fitted to what the kernels give.
"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _crf_reference as RC  # noqa: E402
from tests import _nc_reference as R  # noqa: E402
from tests.test_gpu_ops import TOL, rel  # noqa: E402
from tests.test_gpu_step import build_model  # noqa: E402

NAN = float('nan')


def _kernel(z, x, m, prm, g_up=1.0, loss_scale=1.0, prefill=None, need_grad=True):
    """pp_nc_loss_fwd (+ the device-side finalize) and pp_nc_loss_bwd on CUDA copies: (loss, dlogits, sums, assoc_vol).  Workspace,
    unit gradient and assoc_vol start as NaN: an entry nobody wrote shows in what is read from them."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    z, x = z.float().cuda().contiguous(), x.float().cuda().contiguous()
    m = m.float().cuda().contiguous() if m is not None else None
    N, K, H, W = z.shape
    st = stream_ptr()
    sums = torch.full((4,), NAN, device='cuda', dtype=torch.float64)
    av = torch.full((N, K, 2), NAN, device='cuda', dtype=torch.float64)
    nws = lib.pp_nc_loss_workspace(N, K, H, W)
    ws = torch.full(((nws + 7) // 8,), NAN, device='cuda', dtype=torch.float64)
    unit = torch.full_like(z, NAN) if need_grad else None
    lib.pp_nc_loss_fwd(z.data_ptr(), x.data_ptr(), m.data_ptr() if m is not None else None, N, K, x.shape[1], H, W, prm['radius'],
                       prm['dilation'], prm['sigma_xy'], prm['sigma_rgb'], unit.data_ptr() if need_grad else None, av.data_ptr(),
                       sums[2:].data_ptr(), ws.data_ptr(), nws, st)
    loss = torch.empty((), device='cuda')
    lib.pp_losses_finalize(sums.data_ptr(), 0, None, loss.data_ptr(), None, st)
    dz = None
    if need_grad:
        dz = torch.zeros_like(z) if prefill is None else prefill.float().cuda().clone()
        g = torch.tensor(g_up, device='cuda', dtype=torch.float32)
        lib.pp_nc_loss_bwd(unit.data_ptr(), sums[2:].data_ptr(), g.data_ptr(), loss_scale, dz.data_ptr(), z.numel(), st)
    torch.cuda.synchronize()
    return loss.cpu(), (dz.cpu() if dz is not None else None), sums.cpu(), av.cpu()


def _inputs(N, K, C, H, W, seed, masked, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, K, H, W, generator=g) * scale
    x = R.smooth_image(N, C, H, W, seed=seed + 1)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    return z, x, m


_REF = {}


def _reference(tag, z, x, m, prm):
    """Float64 (loss, gradient, A, V) at the fp32 inputs the kernel sees: computed once per case, shared, never modified."""
    if tag not in _REF:
        loss, grad = R.nc_loss_and_grad(z.float(), x.float(), m, **prm)
        A, V = R.nc_assoc_vol(z.float(), x.float(), m, **prm)
        _REF[tag] = (loss, grad, A.detach(), V.detach())
    return _REF[tag]


def _check(tag, z, x, m, prm):
    ref_loss, ref_grad, A, V = _reference(tag, z, x, m, prm)
    loss, dz, sums, av = _kernel(z, x, m, prm)
    N, K = z.shape[:2]
    e_loss, e_grad = abs(float(loss) - float(ref_loss)), rel(dz, ref_grad)
    assert float(A.min()) > 0 and float(V.min()) > 0, tag               # every entry has a scale of its own
    e_a, e_v = float(((av[..., 0] - A).abs() / A).max()), float(((av[..., 1] - V).abs() / V).max())      # per entry, each by its own value
    print(f'{tag}: loss {float(loss)!r} ref {float(ref_loss)!r} (|diff| {e_loss:.2e}), gradient rel {e_grad:.2e}, max |grad| '
          f'{float(ref_grad.abs().max()):.3e}, A rel {e_a:.2e}, V rel {e_v:.2e}, min V {float(V.min()):.3e}')
    assert torch.isfinite(loss) and torch.isfinite(dz).all() and torch.isfinite(av).all(), tag
    assert sums[2:].tolist()[1] == float(N * K), (tag, sums.tolist())
    assert e_loss <= 1e-5 * max(1.0, abs(float(ref_loss))), (tag, float(loss), float(ref_loss))
    assert e_a <= 1e-6 and e_v <= 1e-6, (tag, e_a, e_v)
    assert e_grad < TOL, (tag, e_grad)
    return float(ref_loss), ref_grad, V


# (N, K, C, H, W, radius, dilation, masked): every class-count regime (one chunk, equal-width chunks, 32), sizes that are no
# multiple of the 64 x 4 tile, halo 16, the run-time channel-count form, with and without mask
CASES = [
    (2, 1, 1, 24, 20, 1, 1, False),
    (2, 2, 1, 24, 20, 2, 1, True),
    (1, 2, 3, 33, 31, 1, 3, False),
    (2, 5, 1, 33, 31, 5, 1, True),
    (1, 5, 3, 24, 20, 3, 2, False),
    (1, 5, 1, 70, 130, 4, 1, False),
    (1, 9, 1, 24, 20, 4, 2, True),
    (1, 9, 3, 33, 31, 2, 1, False),
    (1, 17, 3, 24, 20, 5, 3, True),
    (1, 17, 1, 33, 31, 3, 1, False),
    (1, 32, 1, 33, 31, 5, 1, True),
    (1, 32, 3, 24, 20, 2, 2, False),
    (1, 8, 2, 40, 64, 8, 2, True),            # the largest halo (16) and the run-time channel-count form (C = 2)
    (1, 32, 4, 20, 70, 4, 4, False),          # halo 16, C = 4, K = 32: the LDS bound shrinks the class chunks
    (1, 5, 1, 256, 256, 5, 1, True),          # the training shape: 256 blocks per image in the fixed-order sums
]


@pytest.mark.parametrize('case', CASES, ids=[f'K{c[1]}-C{c[2]}-{c[3]}x{c[4]}-r{c[5]}d{c[6]}{"-mask" if c[7] else ""}' for c in CASES])
def test_kernel_against_float64(case):
    N, K, C, H, W, r, d, masked = case
    z, x, m = _inputs(N, K, C, H, W, seed=17 * K + r + d, masked=masked)
    prm = dict(radius=r, dilation=d, sigma_xy=6.0 if r == 5 else 1.0 + r, sigma_rgb=0.1)
    ref_loss, ref_grad, V = _check(str(case), z, x, m, prm)
    assert float(V.min()) > 1e-3                                          # no case sits near V_MIN
    if K > 1:
        assert 0.3 < ref_loss < 1.0 and float(ref_grad.abs().max()) > 0      # not a vacuous case (about 1 - 1/K with these inputs)
    else:
        assert abs(ref_loss) <= 1e-6 and float(ref_grad.abs().max()) == 0.0


@pytest.mark.parametrize('K,masked', [(5, False), (5, True), (17, True)])
def test_sharp_predictions(K, masked):
    """Logits scaled by 60: the probabilities are 0 or 1 to fp32; everything stays finite and within the bounds."""
    z, x, m = _inputs(2, K, 1, 33, 31, seed=5 + K, masked=masked, scale=60.0)
    p = torch.softmax(z.float(), 1)
    assert float(((p > 1e-6) & (p < 1 - 1e-6)).float().mean()) < 0.2      # nearly every probability is 0 or 1 to fp32
    _check(f'sharp K={K}{" masked" if masked else ""}', z, x, m, dict(radius=3, dilation=1, sigma_xy=4.0, sigma_rgb=0.1))


def test_inactive_class():
    """A class no pixel of the batch predicts: V = 0 exactly, it adds nothing to the loss and its logits get exactly no gradient."""
    prm = dict(radius=4, dilation=1, sigma_xy=5.0, sigma_rgb=0.1)
    z, x, _ = _inputs(2, 5, 1, 33, 31, seed=3, masked=False)
    z[:, 3] = -1e4
    ref_loss, ref_grad = R.nc_loss_and_grad(z, x, None, **prm)
    loss, dz, sums, av = _kernel(z, x, None, prm)
    print(f'inactive class: loss {float(loss)!r} float64 {float(ref_loss)!r}, gradient rel {rel(dz, ref_grad):.2e}')
    assert 0.55 < float(ref_loss) < 0.65                                 # four active classes of five: (4/5) (1 - 1/4)
    assert av[:, 3].abs().max() == 0.0 and float(av[:, [0, 1, 2, 4], 1].min()) > 1e-3
    assert abs(float(loss) - float(ref_loss)) <= 1e-5
    assert float(dz[:, 3].abs().max()) == 0.0 and float(ref_grad[:, 3].abs().max()) == 0.0
    assert torch.isfinite(dz).all() and rel(dz, ref_grad) < TOL


def test_all_zero_mask():
    prm = dict(radius=4, dilation=1, sigma_xy=5.0, sigma_rgb=0.1)
    z, x, _ = _inputs(2, 5, 1, 33, 31, seed=3, masked=False)
    loss, dz, sums, av = _kernel(z, x, torch.zeros(2, 1, 33, 31), prm)
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and sums[2:].tolist() == [0.0, 10.0]
    assert float(av.abs().max()) == 0.0


def test_backward_accumulates_and_scales():
    """dlogits is pre-filled, loss_scale and the upstream gradient differ from 1: dlogits = prefill + loss_scale * g_up * dL/dz."""
    z, x, m = _inputs(2, 5, 1, 33, 31, seed=8, masked=True)
    prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    _, ref_grad = R.nc_loss_and_grad(z, x, m, **prm)
    inc = 1024.0 * 0.37 * ref_grad
    pre = torch.randn(z.shape, generator=torch.Generator().manual_seed(1)) * float(inc.abs().max())      # of the increment's size
    _, dz, _, _ = _kernel(z, x, m, prm, g_up=0.37, loss_scale=1024.0, prefill=pre)
    e = rel(dz.double() - pre.double(), inc)
    print(f'accumulate: rel {e:.2e}')
    assert e < TOL
    # an odd element count takes the scalar forms of both streaming kernels
    z1, x1, _ = _inputs(1, 3, 1, 5, 7, seed=2, masked=False)
    _check('tail', z1, x1, None, dict(radius=2, dilation=1, sigma_xy=2.0, sigma_rgb=0.1))
    # forward only: no unit-gradient buffer, the same sums
    a = _kernel(z, x, m, prm)
    b = _kernel(z, x, m, prm, need_grad=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][2:], b[2][2:]) and torch.equal(a[3], b[3]) and b[1] is None


def test_bit_reproducible():
    for K, masked in ((5, True), (17, False)):
        z, x, m = _inputs(2, K, 3, 70, 130, seed=K, masked=masked)
        prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
        a, b = _kernel(z, x, m, prm), _kernel(z, x, m, prm)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][2:], b[2][2:]) and torch.equal(a[3], b[3]), K
        assert float(a[1].abs().max()) > 0


def test_argument_checks():
    """Every bad argument is refused before a launch: an error code, and the NaN-filled outputs stay as they were."""
    from pacingpseudo_amd._lib import HipLibraryError, lib, stream_ptr
    z, x = torch.zeros(1, 5, 8, 8, device='cuda'), torch.zeros(1, 1, 8, 8, device='cuda')
    nws = lib.pp_nc_loss_workspace(1, 5, 8, 8)
    # 2 blocks x 5 classes x 2 doubles | 5 x 2 floats padded to 16 bytes | 64 floats
    assert nws == 2 * 5 * 2 * 8 + 48 + 64 * 4 and lib.pp_nc_loss_workspace(0, 5, 8, 8) == 0
    sums = torch.full((2,), NAN, device='cuda', dtype=torch.float64)
    av = torch.full((1, 5, 2), NAN, device='cuda', dtype=torch.float64)
    unit = torch.full((1, 5, 8, 8), NAN, device='cuda')
    ws = torch.zeros(nws, device='cuda', dtype=torch.uint8)

    def call(K=5, C=1, r=5, d=1, sxy=6.0, srgb=0.1, nbytes=nws, zp=z.data_ptr(), avp=av.data_ptr(), wsp=ws.data_ptr()):
        lib.pp_nc_loss_fwd(zp, x.data_ptr(), None, 1, K, C, 8, 8, r, d, sxy, srgb, unit.data_ptr(), avp, sums.data_ptr(), wsp, nbytes,
                           stream_ptr())
    for kw in (dict(K=0), dict(K=33), dict(C=0), dict(C=5), dict(r=0), dict(r=9), dict(d=0), dict(d=5), dict(r=5, d=4), dict(sxy=0.0),
               dict(srgb=-1.0), dict(srgb=float('nan')), dict(zp=None), dict(avp=None), dict(wsp=ws.data_ptr() + 4)):
        with pytest.raises(HipLibraryError, match='nc_loss_fwd'):
            call(**kw)
    with pytest.raises(HipLibraryError, match='workspace too small'):
        call(nbytes=nws - 1)
    g = torch.ones((), device='cuda')
    for up, n in ((unit.data_ptr(), 0), (None, 320)):
        with pytest.raises(HipLibraryError, match='nc_loss_bwd'):
            lib.pp_nc_loss_bwd(up, sums.data_ptr(), g.data_ptr(), 1.0, unit.data_ptr(), n, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(sums).all() and torch.isnan(av).all() and torch.isnan(unit).all()
    call()                                                                 # and the good call goes through
    torch.cuda.synchronize()
    # constant logits and image: p = 1/5 everywhere, A = V / 5, NC = 4/5 for each of the five classes; a symmetric point: no gradient
    assert abs(sums[0].item() - 4.0) <= 1e-5 and sums[1].item() == 5.0 and torch.isfinite(av).all()
    assert float(unit.abs().max()) <= TOL * float(1.0 / av[..., 1].min())


def test_functional_normalized_cut_loss():
    """losses.normalized_cut_loss stand-alone: value and gradient against float64, scaled upstream gradient, argument checks."""
    from pacingpseudo_amd.losses import normalized_cut_loss
    z, x, m = _inputs(2, 4, 3, 20, 24, seed=21, masked=True)
    for mask in (None, m):
        zc = z.cuda().requires_grad_(True)
        loss = normalized_cut_loss(zc, x.cuda(), mask.cuda() if mask is not None else None, radius=3, dilation=2, sigma_xy=3.0, sigma_rgb=0.2)
        (loss * 2.5).backward()
        ref_loss, ref_grad = R.nc_loss_and_grad(z, x, mask, radius=3, dilation=2, sigma_xy=3.0, sigma_rgb=0.2)
        assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
        assert float(ref_grad.abs().max()) > 0 and rel(zc.grad, 2.5 * ref_grad) < TOL
    with torch.no_grad():
        assert 0.3 < float(normalized_cut_loss(z.cuda(), x.cuda())) < 1.0      # defaults; no gradient buffer without a graph
    with pytest.raises(ValueError, match='normalised cut'):
        normalized_cut_loss(z.cuda(), x.cuda(), radius=0)
    with pytest.raises(NotImplementedError, match='normalised cut'):
        normalized_cut_loss(z.cuda(), x.cuda(), radius=6, dilation=3)
    with pytest.raises(NotImplementedError):
        normalized_cut_loss(z.cuda(), torch.zeros(2, 5, 20, 24, device='cuda'))
    with pytest.raises(ValueError):
        normalized_cut_loss(z.cuda(), x.cuda()[:, :, :10])
    with pytest.raises(ValueError):
        normalized_cut_loss(z.cuda(), x.cuda(), valid_mask=torch.ones(2, 4, 20, 24, device='cuda'))
    with pytest.raises(TypeError):
        normalized_cut_loss(z, x)                                             # CPU tensors


# ---------------------------------------------------------------------------------------------------------------- whole step
# At unit weight the gradient of this loss is of the order of 1e-5 per logit (it is a mean over N K ratios whose derivative carries
# 1 / V, V ~ H W / K; 7e-6 at this network's initial logits), below the partial cross entropy's 1 / (scribble pixels) ~ 6e-4 at these
# shapes: a max-norm comparison of dlogits would not see it.  The tests weigh it by 30 (1e-5 -> 3e-4, about a third of the sum) and
# ASSERT its share on the float64 gradients.
W_NC = 30.0
W_CRF = 3.0
PRM = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)


def _nc_flags(**over):
    return O.full_flags(do_loss_nc=True, nc_radius=5, nc_dilation=1, nc_sigma_xy=6.0, nc_sigma_rgb=0.1, **over)


def _step_batch(B, size, seed=3):
    b = O.synthetic_batch(B, size, size, seed=seed, keep=0.05)
    b['image'] = R.smooth_image(B, 1, size, size, seed=seed) * 4.0            # intensities the bilateral kernel can tell apart
    b['image_strong'] = b['image'] * 1.3 - 0.2
    b['valid_mask'][0, :, :9] = 0
    b['valid_mask'][1, :, :, -5:] = 0
    return {k: v.cuda() for k, v in b.items() if k != 'label'}


def _assembled(args, out, epoch):
    w = O.loss_weights(args, epoch)
    total = sum(out[k] * wt for k, wt in w.items()) + out['loss_nc'] * W_NC
    if getattr(args, 'do_loss_crf', False):
        total = total + out['loss_crf'] * W_CRF
    return total, w


def _oracle_dlogits(args, batch, zw, zs, w, with_crf):
    """The float64 gradients of the assembled loss with respect to the weak logits, at the device's logits, term by term:
    {'rest': pce + w_ent ent + w_cr cr, 'nc': W_NC nc, 'crf': W_CRF crf}, and the float64 loss values."""
    zw = zw.detach().double().cpu().requires_grad_(True)
    zs = zs.detach().double().cpu()
    mask = batch['valid_mask'].cpu()
    target = batch['scribble'].cpu().argmax(1).long()
    rest = O.partial_cross_entropy_loss(zw, target, args.ignored_index)
    rest = rest + w['loss_ent'] * O.entropy_minimization_loss(zw, mask.double())
    rest = rest + w['loss_cr'] * O.soft_label_cross_entropy_loss(zs, torch.softmax(zw, 1), mask.double())
    nc = R.nc_loss_direct(zw, batch['image'].cpu(), mask, **PRM)
    g = {'rest': torch.autograd.grad(rest, zw)[0], 'nc': W_NC * torch.autograd.grad(nc, zw)[0]}
    vals = {'nc': nc.detach()}
    if with_crf:
        crf = RC.crf_loss_direct(zw, batch['image'].cpu(), mask, **PRM)
        g['crf'] = W_CRF * torch.autograd.grad(crf, zw)[0]
        vals['crf'] = crf.detach()
    return g, vals


def _whole_step(storage, with_crf):
    over = dict(do_loss_crf=True, crf_radius=5, crf_dilation=1, crf_sigma_xy=6.0, crf_sigma_rgb=0.1) if with_crf else {}
    args = _nc_flags(**over)
    args.storage = storage
    torch.manual_seed(1)
    model = build_model(args)
    model.train()
    B = 2
    batch = _step_batch(B, 128)
    out = model(batch, mode='train', step=37)
    keys = list(out)
    assert keys == model._expected_keys('train') and 'loss_nc' in out
    if with_crf:
        assert keys[keys.index('loss_crf') + 1] == 'loss_nc' and keys[keys.index('loss_crf') - 1] == 'segmentation/logits_strong'
    total, w = _assembled(args, out, 37)
    total.backward()
    torch.cuda.synchronize()
    plan = model.engine.last_plan
    scale = plan.loss_scale
    assert plan.all_sums.numel() == (12 if with_crf else 10) and plan.regs['nc'].sums.data_ptr() == plan.all_sums[8 if with_crf else 6:].data_ptr()
    g, vals = _oracle_dlogits(args, batch, out['segmentation/logits'], out['segmentation/logits_strong'], w, with_crf)
    ref_g = sum(g.values())
    got = float(out['loss_nc'])
    e = rel(plan.dlogits[:B], scale * ref_g)
    share = {k: float(v.abs().max() / ref_g.abs().max()) for k, v in g.items()}
    print(f'{storage}{" + crf" if with_crf else ""}: loss_nc {got!r} float64 {float(vals["nc"])!r}; dlogits[:B] rel {e:.2e} at loss scale {scale}; '
          f'max |gradient| of each term / of the sum {share}; max |d nc| at unit weight {float(g["nc"].abs().max()) / W_NC:.3e}')
    assert 0.3 < float(vals['nc']) < 1.0
    assert share['nc'] >= 0.1                                            # the term is visible in a max-norm comparison
    assert abs(got - float(vals['nc'])) <= 1e-5 * max(1.0, abs(float(vals['nc'])))
    assert e < TOL
    for k in g:                                                          # every term is IN the gradient: without it the comparison fails
        if k != 'rest':
            assert rel(plan.dlogits[:B], scale * (ref_g - g[k])) > 10 * TOL, k
    if with_crf:
        assert abs(float(out['loss_crf']) - float(vals['crf'])) <= 1e-5 * max(1.0, abs(float(vals['crf'])))
    return model, batch, args


@pytest.mark.parametrize('storage', ['fp32', 'bf16', 'fp16'])
def test_whole_step(storage):
    model, batch, args = _whole_step(storage, with_crf=False)
    if storage == 'fp16':
        assert model.engine.last_plan.loss_scale == 1024.0
    # the loss moves the weights' gradients: not a term that is computed and dropped
    g_on = model.flat.grads.clone()
    out2 = model(batch, mode='train', step=37)
    sum(out2[k] * wt for k, wt in O.loss_weights(args, 37).items()).backward()
    torch.cuda.synchronize()
    assert not torch.equal(g_on, model.flat.grads)


def test_whole_step_with_the_crf_loss_as_well():
    """Both regularisers on: two independent walks, keys in order, both terms in the gradient."""
    _whole_step('fp32', with_crf=True)


def test_mask_applies_without_entropy_or_consistency():
    """--do_loss_nc alone: the batch's valid_mask still masks this loss (the partial CE has no mask)."""
    args = O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_nc=True)
    torch.manual_seed(2)
    model = build_model(args)
    model.train()
    batch = _step_batch(2, 64)
    batch['valid_mask'][:, :, 20:50, 10:40] = 0                              # a third of the pixels: the mask matters
    out = model(batch, mode='train', step=0)
    assert list(out) == ['segmentation/logits', 'loss_pce', 'loss_nc']
    (out['loss_pce'] + out['loss_nc']).backward()
    torch.cuda.synchronize()
    z = out['segmentation/logits'].detach().cpu()
    A, V = R.nc_assoc_vol(z, batch['image'].cpu(), batch['valid_mask'].cpu())
    A1, V1 = R.nc_assoc_vol(z, batch['image'].cpu(), None)
    ref = R.nc_terms(A, V).mean()
    av = model.engine.last_plan.regs['nc'].state.cpu()
    assert float(((V1 - V) / V1).min()) > 0.1                               # the masked volumes are not the unmasked ones ...
    assert float(A.min()) > 0
    assert float(((av[..., 1] - V).abs() / V).max()) <= 1e-6 and float(((av[..., 0] - A).abs() / A).max()) <= 1e-6      # ... and the device has the masked
    assert abs(float(out['loss_nc']) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    # train mode without a graph (no_grad): the loss is still evaluated, from a forward-only plan without a unit-gradient buffer
    with torch.no_grad():
        o = model(batch, mode='train', step=0)
    assert abs(float(o['loss_nc']) - float(out['loss_nc'])) <= 1e-5 and model.engine.last_plan.regs['nc'].unit is None
    assert 'loss_nc' not in model(batch, mode='val')


def test_flag_off_is_the_parent_step():
    """do_loss_nc=False and a namespace without the attribute: the same keys, bit-identical losses, gradient slab and dlogits, and
    no buffer of this loss in the plan."""
    runs = {}
    for tag, args in (('absent', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])),
                      ('off', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_nc=False, nc_radius=3))):
        torch.manual_seed(5)
        model = build_model(args)
        model.train()
        batch = _step_batch(2, 64)
        out = model(batch, mode='train', step=3)
        sum(out[k] * wt for k, wt in O.loss_weights(args, 3).items()).backward()
        torch.cuda.synchronize()
        plan = model.engine.last_plan
        assert 'nc' not in plan.regs and 'nc' not in model.engine.regs and 'crf' not in plan.regs and plan.all_sums.numel() == 8
        assert plan.aux['sums'].data_ptr() == plan.all_sums[6:].data_ptr()
        runs[tag] = (list(out), {k: v.detach().clone() for k, v in out.items()}, model.flat.grads.clone(), plan.dlogits.clone())
    a, b = runs['absent'], runs['off']
    assert a[0] == b[0] and 'loss_nc' not in a[0]
    for k in a[0]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_engine_rejects_bad_parameters_before_a_launch():
    for kw, err in ((dict(nc_radius=0), ValueError), (dict(nc_sigma_rgb=0.0), ValueError), (dict(nc_radius=5, nc_dilation=4), NotImplementedError)):
        with pytest.raises(err, match='normalised cut'):
            build_model(O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_nc=True, **kw))


def test_graph_replay_equals_eager_with_the_loss_on():
    """Eager vs GraphedStep over three iterations with the loss on (full flags): loss, parameters and Adam moments bit for bit."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = _nc_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])

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
        losses, ncs = [], []
        for _ in range(3):
            loss, out = gs(batch, 0)
            losses.append(loss.detach().clone())
            ncs.append(out['loss_nc'].detach().clone())
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(losses=torch.stack(losses).cpu(), ncs=torch.stack(ncs).cpu(), params=model.flat.params.clone(), m=sd['m'], v=sd['v'],
                         captures=gs.captures, replays=gs.replays)
    e, g = runs['eager'], runs['graph']
    print('losses', e['losses'].tolist(), 'loss_nc', e['ncs'].tolist())
    assert e['captures'] == 0 and g['captures'] == 1 and g['replays'] == 2
    assert float(e['ncs'].min()) > 0 and len(set(e['ncs'].tolist())) == 3          # the weights move, and so does the loss
    for k in ('losses', 'ncs', 'params', 'm', 'v'):
        assert torch.equal(e[k], g[k]), k


def test_driver_logs_the_loss(tmp_path):
    """train.py with the flag on, alone (ramped weight) and beside the CRF loss: the epoch line gains its column behind loss_crf's,
    scalars.jsonl its tag, and the column holds weight x loss."""
    import glob
    import json
    import re
    from pacingpseudo_amd.train import train_main
    common = ['--session', 'Experiment', '--synthetic', '8', '--epoch', '2', '--batch_size', '4', '--image_size', '64', '--num_workers', '0',
              '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path', '--do_memory']
    for tag, extra in (('nc', ['--do_loss_nc', '--ramp_up_loss_nc', '--nc_radius', '3']),
                       ('both', ['--do_loss_nc', '--loss_nc_weight', '0.5', '--do_loss_crf'])):
        root = str(tmp_path / tag)
        train_main(['--tag', tag, '--root', root] + common + extra)
        run = glob.glob(os.path.join(root, 't1', 'Experiment', f'Experiment-*-fold1-{tag}'))[0]
        lines = [ln for ln in open(os.path.join(run, 'log.txt')) if 'loss_nc: ' in ln and 'epoch: ' in ln]
        assert len(lines) == 2, lines
        assert all(('loss_crf: ' in ln) == (tag == 'both') for ln in lines)
        if tag == 'both':
            assert all(ln.index('loss_crf: ') < ln.index('loss_nc: ') < ln.index('s/epoch') for ln in lines)
        sc = [json.loads(ln) for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))]
        vals = [r['value'] for r in sc if r['tag'] == 'train/loss_nc']
        assert len(vals) == 2 and (('train/loss_crf' in {r['tag'] for r in sc}) == (tag == 'both'))
        logged = [float(re.search(r'loss_nc: ([0-9.eE+-]+)', ln).group(1)) for ln in lines]
        assert all(abs(a - b) <= 1e-6 for a, b in zip(logged, vals))
        # the meter holds weight x loss, 0 < loss < 1: the ramp starts at exp(-5 (1 - 0)^2 ...) of 0.1, the fixed weight is 0.5
        w_max = 0.5 if tag == 'both' else 0.1
        assert all(0.0 < v < w_max for v in vals), vals


# ---------------------------------------------------------------------------------------------------------------- data-parallel
def _rank(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    from pacingpseudo_amd import parallel
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group('gloo')
    args = _nc_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    torch.manual_seed(1)
    model = build_model(args)
    if world > 1:
        parallel.attach(model)
    model.eval()                                    # BatchNorm in eval mode: every sample independent of how the batch is split
    full = _step_batch(4, 64, seed=11)
    full['valid_mask'][3, :, 20:40] = 0
    nloc = 4 // world
    batch = {k: v[rank * nloc:(rank + 1) * nloc].contiguous() for k, v in full.items()}
    out = model(batch, mode='train', step=37)
    _assembled(args, out, 37)[0].backward()
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(dict(loss_nc=float(out['loss_nc']), grads=model.flat.grads.cpu()), out_path)
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
    """Two ranks on the one GPU (gloo), each with half of a masked batch: sum NC and the count N K travel in the all-reduced sums
    block, so both reach the single process's loss_nc (1e-5) and gradient slab (rel < 1e-4)."""
    one = _launch(1, str(tmp_path / 'one.pt'))
    two = _launch(2, str(tmp_path / 'two.pt'))
    e = rel(two['grads'], one['grads'])
    print(f'loss_nc one process {one["loss_nc"]!r}, two ranks {two["loss_nc"]!r}; gradient slab rel {e:.2e}')
    assert 0.3 < one['loss_nc'] < 1.0
    assert abs(two['loss_nc'] - one['loss_nc']) <= 1e-5
    assert e < TOL
