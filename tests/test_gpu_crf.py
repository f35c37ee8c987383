"""The gated-CRF loss (--do_loss_crf, pp_crf_loss_*, losses.gated_crf_loss) on the MI355X against the float64 comparison function
of tests/_crf_reference.py (the direct double sum, differentiated by autograd).

Bounds: the project's existing ones -- the loss within 1e-5 * max(1, |L|), gradients rel < TOL = 1e-4 in the `rel` measure of
tests/test_gpu_ops.py.  An fp32 evaluation of the gather form stays within 1.2e-6 / 1.1e-7 of the float64 values on the CPU, so
both hold with about 100x of room; nothing here is fitted to what the kernels give.
"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _crf_reference as R  # noqa: E402
from tests.test_gpu_ops import TOL, rel  # noqa: E402
from tests.test_gpu_step import build_model  # noqa: E402


def _kernel(z, x, m, prm, g_up=1.0, loss_scale=1.0, prefill=None, need_grad=True):
    """pp_crf_loss_fwd (+ the device-side finalize) and pp_crf_loss_bwd on CUDA copies: (loss, dlogits, sums)."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    z, x = z.float().cuda().contiguous(), x.float().cuda().contiguous()
    m = m.float().cuda().contiguous() if m is not None else None
    N, K, H, W = z.shape
    st = stream_ptr()
    sums = torch.full((4,), float('nan'), device='cuda', dtype=torch.float64)
    nws = lib.pp_crf_loss_workspace(N, H, W)
    ws = torch.full((nws // 8,), float('nan'), device='cuda', dtype=torch.float64)        # every partial must be written
    unit = torch.full_like(z, float('nan')) if need_grad else None
    lib.pp_crf_loss_fwd(z.data_ptr(), x.data_ptr(), m.data_ptr() if m is not None else None, N, K, x.shape[1], H, W, prm['radius'],
                        prm['dilation'], prm['sigma_xy'], prm['sigma_rgb'], unit.data_ptr() if need_grad else None,
                        sums[2:].data_ptr(), ws.data_ptr(), nws, st)
    loss = torch.empty((), device='cuda')
    lib.pp_losses_finalize(sums.data_ptr(), 1 if m is not None else 0, None, loss.data_ptr(), None, st)
    dz = None
    if need_grad:
        dz = torch.zeros_like(z) if prefill is None else prefill.float().cuda().clone()
        g = torch.tensor(g_up, device='cuda', dtype=torch.float32)
        lib.pp_crf_loss_bwd(unit.data_ptr(), sums[2:].data_ptr(), 1 if m is not None else 0, g.data_ptr(), loss_scale, dz.data_ptr(),
                            z.numel(), st)
    torch.cuda.synchronize()
    return loss.cpu(), (dz.cpu() if dz is not None else None), sums.cpu()


def _inputs(N, K, C, H, W, seed, masked, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, K, H, W, generator=g) * scale
    x = R.smooth_image(N, C, H, W, seed=seed + 1)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    return z, x, m


def _check(tag, z, x, m, prm):
    ref_loss, ref_grad = R.crf_loss_and_grad(z.float(), x.float(), m, **prm)      # (the fp32 inputs the kernel sees, in float64)
    loss, dz, _ = _kernel(z, x, m, prm)
    e_loss, e_grad = abs(float(loss) - float(ref_loss)), rel(dz, ref_grad)
    print(f'{tag}: loss {float(loss)!r} ref {float(ref_loss)!r} (|diff| {e_loss:.2e}), gradient rel {e_grad:.2e}, max |grad| {float(ref_grad.abs().max()):.3e}')
    assert torch.isfinite(loss) and torch.isfinite(dz).all(), tag
    assert e_loss <= 1e-5 * max(1.0, abs(float(ref_loss))), (tag, float(loss), float(ref_loss))
    assert e_grad < TOL, (tag, e_grad)
    return float(ref_loss), ref_grad


# (N, K, C, H, W, radius, dilation, masked): every class-count regime (one chunk, equal-width chunks, 32), sizes that are no
# multiple of the 64 x 4 tile, every radius 1..5 and dilation 1..3, both channel counts, with and without mask
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
    (1, 5, 1, 256, 256, 5, 1, True),
    (1, 5, 1, 256, 256, 5, 1, False),
    (1, 8, 2, 40, 64, 8, 2, True),            # the largest halo (16) and the run-time channel-count form (C = 2)
    (1, 32, 4, 20, 70, 4, 4, False),          # halo 16, C = 4, K = 32: the LDS bound shrinks the class chunks
]


@pytest.mark.parametrize('case', CASES, ids=[f'K{c[1]}-C{c[2]}-{c[3]}x{c[4]}-r{c[5]}d{c[6]}{"-mask" if c[7] else ""}' for c in CASES])
def test_kernel_against_float64(case):
    N, K, C, H, W, r, d, masked = case
    z, x, m = _inputs(N, K, C, H, W, seed=17 * K + r + d, masked=masked)
    prm = dict(radius=r, dilation=d, sigma_xy=6.0 if r == 5 else 1.0 + r, sigma_rgb=0.1)
    ref_loss, ref_grad = _check(str(case), z, x, m, prm)
    if K > 1:
        assert ref_loss > 1e-3 and float(ref_grad.abs().max()) > 0      # not a vacuous case
    else:
        assert ref_loss == pytest.approx(0.0, abs=1e-12)


@pytest.mark.parametrize('K,masked', [(5, False), (5, True), (17, True)])
def test_sharp_predictions(K, masked):
    """Logits scaled by 60: the probabilities are 0 or 1 to fp32; everything stays finite and within the bounds."""
    z, x, m = _inputs(2, K, 1, 33, 31, seed=5 + K, masked=masked, scale=60.0)
    p = torch.softmax(z.float(), 1)
    assert float(((p > 1e-6) & (p < 1 - 1e-6)).float().mean()) < 0.2      # nearly every probability is 0 or 1 to fp32
    _check(f'sharp K={K}', z, x, m, dict(radius=3, dilation=1, sigma_xy=4.0, sigma_rgb=0.1))


def test_all_zero_mask_and_constant_prediction():
    prm = dict(radius=4, dilation=1, sigma_xy=5.0, sigma_rgb=0.1)
    z, x, _ = _inputs(2, 5, 1, 33, 31, seed=3, masked=False)
    loss, dz, sums = _kernel(z, x, torch.zeros(2, 1, 33, 31), prm)
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0 and sums[2:].tolist() == [0.0, 0.0]
    # a constant one-hot prediction: S_i - p_i.G_i cancels.  |L| <= 1e-5 * max S_i; the gradient is 0 in float64, and on the
    # device every |dL/dz_ic| = (2/D) p_ic |G_ic - p_i.G_i| is bounded by its natural scale (2/D) max S_i times TOL
    zc = torch.zeros(2, 5, 33, 31)
    zc[:, 2] = 60.0
    ref_loss, ref_grad, S = R.crf_gather_form(zc, x, None, **prm)
    loss, dz, _ = _kernel(zc, x, None, prm)
    print(f'constant one-hot: loss {float(loss)!r} (float64 {float(ref_loss)!r}), max S {float(S.max())!r}, max |grad| {float(dz.abs().max())!r}')
    assert abs(float(ref_loss)) < 1e-20 and float(ref_grad.abs().max()) < 1e-20
    assert abs(float(loss)) <= 1e-5 * float(S.max())
    assert float(dz.abs().max()) <= TOL * 2.0 / zc[:, 0].numel() * float(S.max())


def test_backward_accumulates_and_scales():
    """dlogits is pre-filled, loss_scale and the upstream gradient differ from 1: dlogits = prefill + loss_scale * g_up * dL/dz."""
    z, x, m = _inputs(2, 5, 1, 33, 31, seed=8, masked=True)
    prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    _, ref_grad = R.crf_loss_and_grad(z, x, m, **prm)
    inc = 1024.0 * 0.37 * ref_grad
    pre = torch.randn(z.shape, generator=torch.Generator().manual_seed(1)) * float(inc.abs().max())      # of the increment's size
    _, dz, _ = _kernel(z, x, m, prm, g_up=0.37, loss_scale=1024.0, prefill=pre)
    e = rel(dz.double() - pre.double(), inc)
    print(f'accumulate: rel {e:.2e}')
    assert e < TOL
    # an odd element count and misaligned buffers take the scalar form of the streaming kernel
    z1, x1, _ = _inputs(1, 3, 1, 5, 7, seed=2, masked=False)
    _check('tail', z1, x1, None, dict(radius=2, dilation=1, sigma_xy=2.0, sigma_rgb=0.1))
    # forward only: no unit-gradient buffer, the same sums
    a = _kernel(z, x, m, prm)
    b = _kernel(z, x, m, prm, need_grad=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][2:], b[2][2:]) and b[1] is None


def test_bit_reproducible():
    for K, masked in ((5, True), (17, False)):
        z, x, m = _inputs(2, K, 3, 70, 130, seed=K, masked=masked)
        prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
        a, b = _kernel(z, x, m, prm), _kernel(z, x, m, prm)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][2:], b[2][2:]), K


def test_argument_checks():
    from pacingpseudo_amd._lib import HipLibraryError, lib, stream_ptr
    z, x = torch.zeros(1, 5, 8, 8, device='cuda'), torch.zeros(1, 1, 8, 8, device='cuda')
    sums = torch.zeros(2, device='cuda', dtype=torch.float64)
    nws = lib.pp_crf_loss_workspace(1, 8, 8)
    assert nws == 2 * 8 * 2 and lib.pp_crf_loss_workspace(32, 256, 256) == 32 * 64 * 4 * 16
    ws = torch.zeros(nws, device='cuda', dtype=torch.uint8)

    def call(K=5, C=1, r=5, d=1, sxy=6.0, srgb=0.1, nbytes=nws):
        lib.pp_crf_loss_fwd(z.data_ptr(), x.data_ptr(), None, 1, K, C, 8, 8, r, d, sxy, srgb, None, sums.data_ptr(), ws.data_ptr(), nbytes, stream_ptr())
    call()
    for kw in (dict(K=0), dict(K=33), dict(C=0), dict(C=5), dict(r=0), dict(r=9), dict(d=0), dict(d=5), dict(r=5, d=4), dict(sxy=0.0),
               dict(srgb=-1.0), dict(srgb=float('nan'))):
        with pytest.raises(HipLibraryError, match='crf_loss_fwd'):
            call(**kw)
    with pytest.raises(HipLibraryError, match='workspace too small'):
        call(nbytes=nws - 1)
    torch.cuda.synchronize()


def test_functional_gated_crf_loss():
    """losses.gated_crf_loss stand-alone: value and gradient against float64 (a gradcheck-style comparison: the analytic
    backward against the derivative of the float64 function), scaled upstream gradient, argument checks."""
    from pacingpseudo_amd.losses.losses import gated_crf_loss
    z, x, m = _inputs(2, 4, 3, 20, 24, seed=21, masked=True)
    for mask in (None, m):
        zc = z.cuda().requires_grad_(True)
        loss = gated_crf_loss(zc, x.cuda(), mask.cuda() if mask is not None else None, radius=3, dilation=2, sigma_xy=3.0, sigma_rgb=0.2)
        (loss * 2.5).backward()
        ref_loss, ref_grad = R.crf_loss_and_grad(z, x, mask, radius=3, dilation=2, sigma_xy=3.0, sigma_rgb=0.2)
        assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
        assert rel(zc.grad, 2.5 * ref_grad) < TOL
    with torch.no_grad():
        assert float(gated_crf_loss(z.cuda(), x.cuda())) > 0                 # defaults; no gradient buffer without a graph
    with pytest.raises(ValueError):
        gated_crf_loss(z.cuda(), x.cuda(), radius=0)
    with pytest.raises(NotImplementedError):
        gated_crf_loss(z.cuda(), x.cuda(), radius=6, dilation=3)
    with pytest.raises(NotImplementedError):
        gated_crf_loss(z.cuda(), torch.zeros(2, 5, 20, 24, device='cuda'))
    with pytest.raises(ValueError):
        gated_crf_loss(z.cuda(), x.cuda()[:, :, :10])
    with pytest.raises(ValueError):
        gated_crf_loss(z.cuda(), x.cuda(), valid_mask=torch.ones(2, 4, 20, 24, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------- whole step
W_CRF = 0.3


def _crf_flags(**over):
    return O.full_flags(do_loss_crf=True, crf_radius=5, crf_dilation=1, crf_sigma_xy=6.0, crf_sigma_rgb=0.1, **over)


def _step_batch(B, size, seed=3):
    b = O.synthetic_batch(B, size, size, seed=seed, keep=0.05)
    b['image'] = R.smooth_image(B, 1, size, size, seed=seed) * 4.0            # intensities the bilateral kernel can tell apart
    b['image_strong'] = b['image'] * 1.3 - 0.2
    b['valid_mask'][0, :, :9] = 0
    b['valid_mask'][1, :, :, -5:] = 0
    return {k: v.cuda() for k, v in b.items() if k != 'label'}


def _assembled(args, out, epoch):
    w = O.loss_weights(args, epoch)
    return sum(out[k] * wt for k, wt in w.items()) + out['loss_crf'] * W_CRF, w


def _oracle_dlogits(args, batch, zw, zs, w, prm):
    """d (pce + w_ent ent + w_cr cr + W_CRF crf) / d weak logits in float64 at the device's logits: the oracle's loss functions as
    consistency_forward composes them (oracle/pacing_oracle.py), plus the comparison function of this loss."""
    zw = zw.detach().double().cpu().requires_grad_(True)
    zs = zs.detach().double().cpu()
    mask = batch['valid_mask'].cpu()
    target = batch['scribble'].cpu().argmax(1).long()
    total = O.partial_cross_entropy_loss(zw, target, args.ignored_index)
    total = total + w['loss_ent'] * O.entropy_minimization_loss(zw, mask.double())
    total = total + w['loss_cr'] * O.soft_label_cross_entropy_loss(zs, torch.softmax(zw, 1), mask.double())
    crf = R.crf_loss_direct(zw, batch['image'].cpu(), mask, **prm)
    (g,) = torch.autograd.grad(total + W_CRF * crf, zw)
    return g, crf.detach()


@pytest.mark.parametrize('storage', ['fp32', 'bf16', 'fp16'])
def test_whole_step(storage):
    args = _crf_flags()
    args.storage = storage
    torch.manual_seed(1)
    model = build_model(args)
    model.train()
    B = 2
    batch = _step_batch(B, 128)
    out = model(batch, mode='train', step=37)
    assert list(out) == model._expected_keys('train') and 'loss_crf' in out
    total, w = _assembled(args, out, 37)
    total.backward()
    torch.cuda.synchronize()
    plan = model.engine.last_plan
    scale = plan.loss_scale
    if storage == 'fp16':
        assert scale == 1024.0
    prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    ref_g, ref_crf = _oracle_dlogits(args, batch, out['segmentation/logits'], out['segmentation/logits_strong'], w, prm)
    got = float(out['loss_crf'])
    e = rel(plan.dlogits[:B], scale * ref_g)
    print(f'{storage}: loss_crf {got!r} float64 {float(ref_crf)!r}; dlogits[:B] rel {e:.2e} at loss scale {scale}')
    assert float(ref_crf) > 1e-3
    assert abs(got - float(ref_crf)) <= 1e-5 * max(1.0, abs(float(ref_crf)))
    assert e < TOL
    # the loss moves the weights' gradients: not a term that is computed and dropped
    g_on = model.flat.grads.clone()
    out2 = model(batch, mode='train', step=37)
    w2 = O.loss_weights(args, 37)
    sum(out2[k] * wt for k, wt in w2.items()).backward()
    torch.cuda.synchronize()
    assert not torch.equal(g_on, model.flat.grads)


def test_mask_applies_without_entropy_or_consistency():
    """--do_loss_crf alone: the batch's valid_mask still masks this loss (the partial CE has no mask)."""
    args = O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_crf=True)
    torch.manual_seed(2)
    model = build_model(args)
    model.train()
    batch = _step_batch(2, 64)
    out = model(batch, mode='train', step=0)
    assert list(out) == ['segmentation/logits', 'loss_pce', 'loss_crf']
    (out['loss_pce'] + out['loss_crf']).backward()
    torch.cuda.synchronize()
    ref = R.crf_loss_direct(out['segmentation/logits'].detach().cpu(), batch['image'].cpu(), batch['valid_mask'].cpu())
    unmasked = R.crf_loss_direct(out['segmentation/logits'].detach().cpu(), batch['image'].cpu(), None)
    assert abs(float(ref) - float(unmasked)) > 1e-4 * abs(float(ref))            # the mask matters in this batch
    assert abs(float(out['loss_crf']) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    # train mode without a graph (no_grad): the loss is still evaluated, from a forward-only plan without a unit-gradient buffer
    with torch.no_grad():
        o = model(batch, mode='train', step=0)
    assert abs(float(o['loss_crf']) - float(out['loss_crf'])) <= 1e-5 and model.engine.last_plan.regs['crf'].unit is None
    assert 'loss_crf' not in model(batch, mode='val')


def test_flag_off_is_the_parent_step():
    """do_loss_crf=False and a namespace without the attribute: the same keys, bit-identical losses and gradient slab, and no
    buffer of this loss in the plan."""
    runs = {}
    for tag, args in (('absent', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])),
                      ('off', O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_crf=False, crf_radius=3))):
        torch.manual_seed(5)
        model = build_model(args)
        model.train()
        batch = _step_batch(2, 64)
        out = model(batch, mode='train', step=3)
        sum(out[k] * wt for k, wt in O.loss_weights(args, 3).items()).backward()
        torch.cuda.synchronize()
        plan = model.engine.last_plan
        assert 'crf' not in plan.regs and 'crf' not in model.engine.regs and plan.all_sums.numel() == 8
        runs[tag] = (list(out), {k: v.detach().clone() for k, v in out.items()}, model.flat.grads.clone(), plan.dlogits.clone())
    a, b = runs['absent'], runs['off']
    assert a[0] == b[0] and 'loss_crf' not in a[0]
    for k in a[0]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_engine_rejects_bad_parameters_before_a_launch():
    for kw, err in ((dict(crf_radius=0), ValueError), (dict(crf_sigma_rgb=0.0), ValueError), (dict(crf_radius=5, crf_dilation=4), NotImplementedError)):
        with pytest.raises(err):
            build_model(O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], do_loss_crf=True, **kw))


def test_graph_replay_equals_eager_with_the_loss_on():
    """Eager vs GraphedStep over three iterations with the loss on (full flags): loss, parameters and Adam moments bit for bit."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = _crf_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])

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
        losses, crfs = [], []
        for _ in range(3):
            loss, out = gs(batch, 0)
            losses.append(loss.detach().clone())
            crfs.append(out['loss_crf'].detach().clone())
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(losses=torch.stack(losses).cpu(), crfs=torch.stack(crfs).cpu(), params=model.flat.params.clone(), m=sd['m'], v=sd['v'],
                         captures=gs.captures, replays=gs.replays)
    e, g = runs['eager'], runs['graph']
    print('losses', e['losses'].tolist(), 'loss_crf', e['crfs'].tolist())
    assert e['captures'] == 0 and g['captures'] == 1 and g['replays'] == 2
    assert float(e['crfs'].min()) > 0 and len(set(e['crfs'].tolist())) == 3          # the weights move, and so does the loss
    for k in ('losses', 'crfs', 'params', 'm', 'v'):
        assert torch.equal(e[k], g[k]), k


# ---------------------------------------------------------------------------------------------------------------- data-parallel
def _rank(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    from pacingpseudo_amd import parallel
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group('gloo')
    args = _crf_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
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
        torch.save(dict(loss_crf=float(out['loss_crf']), grads=model.flat.grads.cpu()), out_path)
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
    """Two ranks on the one GPU (gloo), each with half of a masked batch: the numerator and sum m travel in the all-reduced sums
    block, so both reach the single process's loss_crf (1e-5) and gradient slab (rel < 1e-4)."""
    one = _launch(1, str(tmp_path / 'one.pt'))
    two = _launch(2, str(tmp_path / 'two.pt'))
    e = rel(two['grads'], one['grads'])
    print(f'loss_crf one process {one["loss_crf"]!r}, two ranks {two["loss_crf"]!r}; gradient slab rel {e:.2e}')
    assert one['loss_crf'] > 1e-3
    assert abs(two['loss_crf'] - one['loss_crf']) <= 1e-5
    assert e < TOL
