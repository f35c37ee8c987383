"""--cr_teacher ema on the device: the consistency term pulls the student's strong-view prediction towards what the optimizer's
EMA weights predict for the weak view (pacingpseudo_amd/engine.py: a forward-only pass that reads every parameter from the shadow
slab; the loss composed from two calls of the fused loss kernels).

Float64 references: tests/_teacher_reference.py.  Reference LOSSES are computed from the device's own teacher logits (fp32 values
cast to float64, so hard_ce_loss takes the same arg-max at every pixel); the teacher logits themselves are compared separately.
Shapes: the loss kernels at 8x8 (four-pixel forms at K = 2, 5) and 7x9 (one-pixel forms), K = 2 / 5 / 17; the networks at 32x32
(the smallest size every stage of the output-stride-8 U-Net exists at), the small one also at 48x32 with an odd batch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests import _teacher_reference as T  # noqa: E402
from tests.test_gpu_step import TOL_OUT, build_model, check_grads, iteration, oracle_with_device_branches  # noqa: E402

TOL = 1e-4              # tests/test_gpu_cr_variants.py::_check: loss within 1e-5 * max(1, |ref|), rel(gradient) < 1e-4
EPOCH = 100             # past the ramp-up: the consistency loss has its full weight
SMALL = dict(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])


def dev():
    return torch.device('cuda', 0)


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _args(width, **over):
    return O.full_flags(**(SMALL if width == 'small' else {}), **over)


def _cuda(batch):
    return {k: v.cuda() for k, v in batch.items() if k != 'label'}


def _adam(model, args, lr=1e-2, decay=0.9):
    from pacingpseudo_amd.optim import FusedAdam
    return FusedAdam(model.parameters(), lr=lr, weight_decay=args.wd, ema_decay=decay)


def _shadow(model, opt):
    return opt.ema_shadow(model.flat)


def _step(model, opt, b, args, epoch=EPOCH):
    out = model(b, mode='train', step=epoch)
    loss = sum(out[k] * wt for k, wt in O.loss_weights(args, epoch).items())
    opt.zero_grad()
    loss.backward()
    opt.step()
    return out


# ---------------------------------------------------------------- 1. the loss composition
_INPUTS = {}


def _inputs(K, H, W):
    """(student logits, teacher logits, mask) for N = 2, fp32 on the CPU; made once per shape and never modified."""
    key = (K, H, W)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(100 * K + H)
        _INPUTS[key] = (torch.randn(2, K, H, W, generator=g) * 2, torch.randn(2, K, H, W, generator=g) * 2,
                        (torch.rand(2, 1, H, W, generator=g) > 0.3).float())
    return _INPUTS[key]


@pytest.mark.parametrize('variant', T.VARIANTS)
@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('K', [2, 5, 17])
@pytest.mark.parametrize('H,W', [(8, 8), (7, 9)])
def test_loss_composition(variant, use_mask, K, H, W):
    """teacher_consistency_loss -- the teacher call of the step's two-call composition -- against float64: loss within
    1e-5 * max(1, |ref|), student gradient within 1e-4 (max-norm relative), finite; nothing flows into the teacher argument."""
    import pacingpseudo_amd.losses as L
    zs, zt, mask = _inputs(K, H, W)
    a = zs.to(dev()).requires_grad_(True)
    b = zt.to(dev()).requires_grad_(True)
    m = mask.to(dev()) if use_mask else None
    loss = L.teacher_consistency_loss(a, b, variant, m) if use_mask else L.teacher_consistency_loss(a, b, variant)
    assert loss.dim() == 0
    (loss * 1.9).backward()
    ar = zs.double().requires_grad_(True)
    ref = T.teacher_consistency(ar, b.detach().cpu().double(), variant, mask.double() if use_mask else None)
    (ref * 1.9).backward()
    err, g = abs(float(loss) - float(ref)), rel(a.grad, ar.grad)
    print(f'{variant} K={K} {H}x{W} mask={use_mask}: loss error {err:.2e} (loss {float(ref):.4e}), rel student gradient {g:.2e}')
    assert err < 1e-5 * max(1, abs(float(ref)))
    assert torch.isfinite(a.grad).all() and g < TOL
    assert b.grad is None


def test_loss_argument_checks():
    import pacingpseudo_amd.losses as L
    zs, zt, mask = _inputs(5, 8, 8)
    a, b = zs.to(dev()), zt.to(dev())
    for bad in (zs, a.double(), a[0]):
        with pytest.raises(TypeError, match='student_logits must be a 4-D float32 CUDA tensor'):
            L.teacher_consistency_loss(bad, b)
    with pytest.raises(TypeError, match='teacher_logits must be a 4-D float32 CUDA tensor'):
        L.teacher_consistency_loss(a, zt)
    with pytest.raises(TypeError, match='valid_mask must be a 4-D float32 CUDA tensor'):
        L.teacher_consistency_loss(a, b, 'ce_loss', mask)
    with pytest.raises(ValueError, match='variant must be one of'):
        L.teacher_consistency_loss(a, b, 'mse')
    with pytest.raises(ValueError, match='same shape'):
        L.teacher_consistency_loss(a, b[:1])


# ---------------------------------------------------------------- 2. the teacher's weights are the shadow
@pytest.mark.parametrize('width', ['small', 'full'])
def test_teacher_logits_are_those_of_the_shadow_weights_bit_for_bit(width):
    """After three optimizer steps with ema_decay 0.9: segmentation/logits_teacher == model.backbone(image) in eval mode inside
    optimizer.ema_weights() -- the same plan kind, the same kernels, the weights swapped in instead of read through the offset --
    and != the live weights' logits.  'full': Winograd and split-fp16 layers on the teacher's path."""
    args = _args(width)
    torch.manual_seed(3)
    model = build_model(args)
    opt = _adam(model, args)
    model.attach_teacher(opt)
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08))
    model.train()
    for _ in range(3):
        _step(model, opt, b, args)
    model.eval()                                  # (the student's pass of the forward below must not move the running statistics)
    out = model(b, mode='train', step=EPOCH)
    assert list(out).index('segmentation/logits_teacher') == list(out).index('segmentation/logits_strong') + 1
    zt = out['segmentation/logits_teacher'].clone()
    assert zt.shape == out['segmentation/logits'].shape and not zt.requires_grad
    kinds = {op.sel.kind for op in model.engine.last_plan.teacher_plan.conv.values()}
    assert {'f16x3', 'fp32'} <= kinds and ('wino' in kinds) == (width == 'full'), kinds
    with torch.no_grad():
        with opt.ema_weights():
            want = model.backbone(b['image'])['segmentation/logits'].clone()
        live = model.backbone(b['image'])['segmentation/logits'].clone()
    assert torch.equal(zt, want), f'max difference {float((zt - want).abs().max()):.3e}'
    assert not torch.equal(zt, live) and rel(zt, live) > 1e-4


def test_frozen_stages_and_in_place_loads_read_as_the_live_values():
    """freeze_encoder(2): the frozen parameters left the slab, the optimizer never averages them, and the teacher reads them at
    offset 0.  Weights loaded in place after the shadow was created (load_state_dict) reach the shadow wherever the average has
    not started: the teacher equals the live eval-mode backbone bit for bit before the first optimizer step."""
    args = _args('small')
    torch.manual_seed(4)
    model = build_model(args)
    model.freeze_encoder(2)
    opt = _adam(model, args)
    model.attach_teacher(opt)
    other = {k: (v + 0.01 * torch.randn_like(v) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    model.load_state_dict(other)
    assert torch.equal(_shadow(model, opt), model.flat.params)
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08))
    model.eval()
    zt = model(b, mode='train', step=EPOCH)['segmentation/logits_teacher'].clone()
    tp = model.engine.last_plan.teacher_plan
    assert tp.conv['enc_block1.conv_block.conv_layer1'].woff == 0 and tp.norm['enc_block2.conv_block.conv_layer2'].goff == 0
    assert tp.conv['enc_block3.conv_block.conv_layer1'].woff == _shadow(model, opt).data_ptr() - model.flat.params.data_ptr() != 0
    with torch.no_grad():
        live = model.backbone(b['image'])['segmentation/logits'].clone()
    assert torch.equal(zt, live)
    model.train()
    for _ in range(2):
        _step(model, opt, b, args)
    model.eval()
    zt = model(b, mode='train', step=EPOCH)['segmentation/logits_teacher'].clone()
    with torch.no_grad(), opt.ema_weights():
        want = model.backbone(b['image'])['segmentation/logits'].clone()
    assert torch.equal(zt, want)


# ---------------------------------------------------------------- 3. the teacher is read-only
def test_the_teacher_pass_writes_no_parameter_no_shadow_and_no_running_statistic():
    """Forward + backward of a teacher step.  Eval-mode student: the shadow slab, every live parameter and every buffer are
    bitwise what they were.  Train-mode student (which updates the running statistics itself): the buffers afterwards are bitwise
    those of the same step without a teacher."""
    args = _args('small')
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08))

    def fwd_bwd(model):
        out = model(b, mode='train', step=EPOCH)
        sum(out[k] * wt for k, wt in O.loss_weights(args, EPOCH).items()).backward()
        torch.cuda.synchronize()

    def buffers(model):
        return {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    torch.manual_seed(3)
    model = build_model(args)
    opt = _adam(model, args)
    model.attach_teacher(opt)
    model.train()
    _step(model, opt, b, args)                    # shadow != parameters from here on
    shadow = _shadow(model, opt)
    assert not torch.equal(shadow, model.flat.params)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    twin = build_model(args, {k: v.cpu().numpy() for k, v in state.items()})
    twin.train()
    before = (shadow.clone(), model.flat.params.clone())
    fwd_bwd(model)
    fwd_bwd(twin)
    assert torch.equal(shadow, before[0]) and torch.equal(model.flat.params, before[1])
    got, want = buffers(model), buffers(twin)
    assert any(not torch.equal(v, state[k]) for k, v in got.items())            # the student did update them
    for k in want:
        assert torch.equal(got[k], want[k]), k
    model.eval()
    state = buffers(model)
    fwd_bwd(model)
    assert torch.equal(shadow, before[0]) and torch.equal(model.flat.params, before[1])
    for k, v in buffers(model).items():
        assert torch.equal(v, state[k]), k


# ---------------------------------------------------------------- 4. the whole step against float64
@pytest.mark.parametrize('variant', ['ce_loss', 'js_loss'])
@pytest.mark.parametrize('B,H,W', [(2, 32, 32), (3, 48, 32)])
@pytest.mark.parametrize('bn_training', [True, False])
def test_step_against_float64(variant, B, H, W, bn_training, monkeypatch):
    """The full-flags step of the small network with the teacher on, after two optimizer steps (shadow != parameters): the teacher
    logits against the oracle's eval-mode U-Net under the averaged parameters, every output and loss (TOL_OUT), and every parameter
    gradient with the LeakyReLU / max-pool choices aligned (check_grads, TOL_GRAD).  The reference consistency term is the float64
    form against the DEVICE's teacher logits.  Bounds are those of the no-teacher whole-step tests, unchanged."""
    args = _args('small', loss_cr_variants=variant)
    torch.manual_seed(2)
    model = build_model(args)
    opt = _adam(model, args, lr=1e-3)
    model.attach_teacher(opt)
    batch = O.synthetic_batch(B, H, W, seed=9, keep=0.08)
    batch['valid_mask'][:, :, :, :5] = 0
    model.train()
    for _ in range(2):
        _step(model, opt, _cuda(batch), args)
    model.train(bn_training)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ema_sd = opt.ema_state_dict(model)
    rec, grads = iteration(model, opt, batch, args, EPOCH)
    zt = rec['segmentation/logits_teacher'].cpu()
    e = G.rel_err(zt.double().numpy(), T.teacher_logits(sd, ema_sd, batch['image'], args).numpy())
    print(f'{variant} B={B} {H}x{W} bn_training={bn_training} teacher logits: rel err {e:.3e}')
    assert e < TOL_OUT
    oargs = _args('small', loss_cr_variants='kl_loss')
    monkeypatch.setattr(O, 'kl_loss', lambda a, b, m=None: T.teacher_consistency(a, zt.double(), variant, m))
    ref_out, _, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, EPOCH, oargs, training=bn_training)
    assert {'loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'} <= set(ref_out) and float(ref_out['loss_cr']) > 0
    for k, v in ref_out.items():
        if k.startswith('_') or not torch.is_tensor(v):
            continue
        e = G.rel_err(rec[k].double().cpu().numpy(), v.numpy())
        print(f'  {k}: rel err {e:.3e}')
        assert e < TOL_OUT, f'{k}: rel err {e:.3e}'
    _, og, _ = oracle_with_device_branches(model, sd, batch, EPOCH, oargs, bn_training)
    worst = check_grads(grads, {k: v.numpy() for k, v in og.items() if v is not None}, bn_training)
    print(f'  worst gradient: {worst}')


# ---------------------------------------------------------------- 5. 'none' is the parent's step
def _launch_log(teacher):
    """(entry point, launch shape) of every engine launch of one step, in order; teacher: 'never' (attach_teacher never called),
    'detached' (attached, then attach_teacher(None)), 'on'."""
    from pacingpseudo_amd import engine as E
    from tests._launch_census import _Recorder
    log = []
    real, real_lib = E.lib_for, E.lib
    E.lib_for = lambda storage: _Recorder(real(storage), storage, lambda key: log.append(key[1:]))
    E.lib = _Recorder(real_lib, 'fp32', lambda key: log.append(key[1:]))
    try:
        args = _args('small')
        torch.manual_seed(3)
        model = build_model(args)
        opt = _adam(model, args)
        if teacher != 'never':
            model.attach_teacher(opt)
        if teacher == 'detached':
            model.attach_teacher(None)
        model.train()
        out = _step(model, opt, _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08)), args)
        torch.cuda.synchronize()
    finally:
        E.lib_for, E.lib = real, real_lib
    return log, list(out), model.flat.params.clone()


def test_teacher_off_is_the_step_as_it_was():
    never, detached, on = _launch_log('never'), _launch_log('detached'), _launch_log('on')
    assert len(never[0]) > 100
    assert never[0] == detached[0] and never[1] == detached[1] and torch.equal(never[2], detached[2])
    assert 'segmentation/logits_teacher' not in never[1] and 'segmentation/logits_teacher' in on[1]
    names = lambda log: [e for e, _ in log]      # noqa: E731
    count = lambda log, e: names(log).count(e)   # noqa: E731
    # on: one more forward of B images in front (its own image pack and head), the loss kernels twice each way, one more finalize
    assert len(on[0]) > len(never[0])
    for entry, extra in (('pp_seg_losses_fwd', 1), ('pp_seg_losses_bwd', 1), ('pp_losses_finalize', 1), ('pp_pack_image_nchw_to_nhwc', 1),
                         ('pp_conv1x1_nhwc_to_nchw_fwd', 1), ('pp_bn_eval_coeffs_batch', 1)):
        assert count(on[0], entry) == count(never[0], entry) + extra, entry
    # nothing of the teacher is differentiated: the backward launches are those of the step without it
    for entry in sorted({e for e in names(never[0]) if 'bwd' in e and e != 'pp_seg_losses_bwd'}):
        assert count(on[0], entry) == count(never[0], entry), entry


# ---------------------------------------------------------------- 6. hipGraph
def test_graph_replay_equals_eager_and_survives_a_validation_epoch():
    """Two eager calls, a capture, three replays against five eager steps: parameters, shadow slab and loss_cr bit for bit.  Then a
    validation epoch over nine slice shapes (more than MAX_INFER_PLANS forward-only plans: the LRU evicts) and one more replay,
    still bit-identical to the eager run's sixth step: the teacher plan, whose buffers the graph holds, is not in that cache."""
    from pacingpseudo_amd.engine import StepEngine
    from pacingpseudo_amd.graph import GraphedStep
    from tests.test_gpu_graph import _loss_fn
    args = _args('small', loss_cr_variants='js_loss')
    f = _loss_fn(args)
    batches = [_cuda(O.synthetic_batch(2, 64, 64, seed=s, keep=0.05)) for s in (3, 4)]
    shapes = [(32, 32), (32, 48), (48, 32), (48, 48), (64, 32), (32, 64), (64, 48), (48, 64), (80, 32)]
    assert len(shapes) > StepEngine.MAX_INFER_PLANS
    vals = [_cuda(O.synthetic_batch(1, h, w, seed=h + w, keep=0.05)) for h, w in shapes]
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(1)
        model = build_model(args)
        opt = _adam(model, args, lr=1e-3)
        model.attach_teacher(opt)
        gs = GraphedStep(model, opt, f, warmup=2) if tag == 'graph' else None
        model.train()
        cr = []

        def one(i):
            b = batches[i % 2]
            if gs is not None:
                cr.append(gs(b, EPOCH)[1]['loss_cr'].detach().clone())
                return
            out = model(b, mode='train', step=EPOCH)
            cr.append(out['loss_cr'].detach().clone())
            loss = f(out, EPOCH)
            opt.zero_grad()
            loss.backward()
            opt.step()
        for i in range(5):
            one(i)
        torch.cuda.synchronize()
        first = dict(params=model.flat.params.clone(), shadow=_shadow(model, opt).clone())
        train_plan = model.engine.last_plan
        teacher_plan = train_plan.teacher_plan
        assert train_plan.trainable and teacher_plan is not None
        built = model.engine.plans_built
        model.eval()
        with torch.no_grad():
            for v in vals:
                assert torch.isfinite(model(v, mode='val')['loss_pce'])
        model.train()
        assert model.engine.plans_built == built + len(shapes)
        assert len([p for p in model.engine.plans.values() if not p.trainable]) == StepEngine.MAX_INFER_PLANS
        one(5)
        torch.cuda.synchronize()
        # (a replay runs no host code: engine.last_plan is still the last validation plan there)
        assert train_plan in model.engine.plans.values() and train_plan.teacher_plan is teacher_plan
        assert teacher_plan not in model.engine.plans.values()
        if gs is not None:
            assert (gs.captures, gs.replays) == (1, 4), (gs.captures, gs.replays)
        runs[tag] = dict(first=first, cr=torch.stack(cr).cpu(), params=model.flat.params.clone(), shadow=_shadow(model, opt).clone())
    e, g = runs['eager'], runs['graph']
    assert torch.isfinite(e['cr']).all() and float(e['cr'].min()) > 0
    assert torch.equal(e['cr'], g['cr']), (e['cr'], g['cr'])
    for k in ('params', 'shadow'):
        assert torch.equal(e['first'][k], g['first'][k]), k
        assert torch.equal(e[k], g[k]), k
    assert not torch.equal(e['params'], e['shadow'])


def test_capture_key_covers_the_teacher():
    from pacingpseudo_amd.graph import GraphedStep
    from tests.test_gpu_graph import _loss_fn
    args = _args('small')
    torch.manual_seed(1)
    model = build_model(args)
    opt = _adam(model, args)
    gs = GraphedStep(model, opt, _loss_fn(args), warmup=1)
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08))
    off = gs._key(b, 0)
    model.attach_teacher(opt)
    on = gs._key(b, 0)
    assert off != on and model.engine.teacher_key()[0][2] == _shadow(model, opt).data_ptr()
    model.attach_teacher(None)
    assert gs._key(b, 0) == off


# ---------------------------------------------------------------- 7. resume
def test_resume_is_bit_identical(tmp_path):
    """Two epochs straight against one epoch + --resume + one epoch (synthetic data, the sizes of tests/test_gpu_resume.py): the
    final checkpoint, the state file (the shadow slab travels in the optimizer state), valdice and every scalar, bit for bit.  The
    train -> eval BatchNorm switch lies between the two epochs."""
    from tests.test_gpu_resume import FULL, SMALL as SIZES, _resume_case
    argv = SIZES + FULL + ['--epoch', '2', '--cpu_input', '--num_workers', '0', '--ema_decay', '0.9', '--cr_teacher', 'ema']
    full, copy, st = _resume_case(tmp_path, 'train_chaos.py', argv, 0, 1)
    assert st['args']['cr_teacher'] == 'ema' and 'ema' in st['optimizer']['slabs'][0]
    assert st['optimizer']['slabs'][0]['steps'] == {'backbone': 8, 'aux_path': 8}


# ---------------------------------------------------------------- 8. a 16-bit student
def test_bf16_student_with_an_fp32_teacher():
    """--storage bf16: the student runs its 16-bit training plan, the teacher its fp32 forward-only plan (bitwise the teacher of
    the fp32-storage run).  One step of the full-width network against fp32 storage, at the whole-step tolerances
    tests/test_gpu_h16.py states for bf16 against fp32."""
    from tests.test_gpu_h16 import MIN_COSINE, TOL_HEAD_GRAD, TOL_LOGITS, TOL_LOSS
    a32, a16 = _args('full'), _args('full')
    a16.storage = 'bf16'
    torch.manual_seed(1)
    m32 = build_model(a32)
    m16 = build_model(a16, {k: v.detach().cpu().numpy() for k, v in m32.state_dict().items()})
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=11, keep=0.08))
    rec = {}
    for name, m, a in (('fp32', m32, a32), ('bf16', m16, a16)):
        opt = _adam(m, a)
        m.attach_teacher(opt)
        _shadow(m, opt).mul_(1.0 + 2.0 ** -6)      # shadow != parameters, the same in both models
        m.train()
        out = m(b, mode='train', step=0)
        sum(out[k] for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory')).backward()
        torch.cuda.synchronize()
        plan = m.engine.last_plan
        assert plan.storage == name and plan.teacher_plan.storage == 'fp32' and plan.teacher_plan.act_dtype == torch.float32
        rec[name] = dict(out={k: v.detach().float().clone() for k, v in out.items()},
                         grads={n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None})
    x, y = rec['fp32'], rec['bf16']
    assert torch.equal(x['out']['segmentation/logits_teacher'], y['out']['segmentation/logits_teacher'])
    for k in ('segmentation/logits', 'segmentation/logits_strong', 'logits_aux_cls'):
        e = rel(y['out'][k], x['out'][k])
        print(f'{k}: rel err {e:.3e}')
        assert 1e-5 < e < TOL_LOGITS['bf16'], (k, e)
    for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'):
        d = abs(float(y['out'][k]) - float(x['out'][k]))
        print(f'{k}: abs err {d:.3e}')
        assert d < TOL_LOSS['bf16'], (k, d)
    for n, ga in x['grads'].items():
        gb = y['grads'][n]
        assert bool(torch.isfinite(gb).all()), n
        if float(ga.norm()) == 0.0:
            continue
        cos = float(torch.dot(ga.flatten().double(), gb.flatten().double()) / (ga.double().norm() * gb.double().norm() + 1e-300))
        assert cos > MIN_COSINE['bf16'], (n, cos)
    gh32, gh16 = x['grads']['backbone.final_conv.weight'], y['grads']['backbone.final_conv.weight']
    assert float((gh32 - gh16).double().norm() / gh32.double().norm()) < TOL_HEAD_GRAD['bf16']


# ---------------------------------------------------------------- 9. stream hazards
def test_no_launch_of_a_teacher_step_races_another():
    """tests/_stream_hazards.py on the recorded log of two teacher steps (full width, 128 px, clipping and EMA on): no pair of
    launches on different streams with overlapping extents, a write among them and no happens-before path.  The pairs in
    question: the teacher's weight packs and forward (main stream, reading the shadow slab) against the second stream's weight
    gradients, and the optimizer's write of the shadow against the next step's teacher pass."""
    from pacingpseudo_amd.optim import FusedAdam
    from tests import _stream_hazards as H
    args = _args('full')
    b = _cuda(O.synthetic_batch(2, 128, 128, seed=7, keep=0.05))
    with pytest.MonkeyPatch.context() as mp, H.Recording(mp) as rec:
        torch.manual_seed(1)
        model = build_model(args)
        model.train()
        opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd, max_grad_norm=1.0, ema_decay=0.99)
        model.attach_teacher(opt)
        torch.cuda.synchronize()
        for _ in range(2):
            _step(model, opt, b, args, 37)
        torch.cuda.synchronize()
        side, main = model.engine._wg_stream.cuda_stream, torch.cuda.current_stream().cuda_stream
        shadow = _shadow(model, opt)
        lo, hi = shadow.data_ptr(), shadow.data_ptr() + 4 * shadow.numel()
    log = rec.log
    launches = [it for it in log if it[0] == 'L']
    assert {it[3] for it in launches} >= {side, main} and side != main
    # the log holds the teacher: pack launches whose SOURCE lies in the shadow slab, on the main stream
    packs = [it for it in launches if it[1] == 'pp_pack_conv3x3_weights_f16x3_batch' and any(lo <= d['w_oihw'] < hi for d in it[2][0][1])]
    assert len(packs) == 2 and all(it[3] == main for it in packs), [it[3] for it in packs]
    assert len([it for it in launches if it[1] == 'pp_adam_step_ema']) >= 2
    found, total = H.check(log)
    assert total == 0, H.report(found, total)
