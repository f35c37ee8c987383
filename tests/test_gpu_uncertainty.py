"""Uncertainty mask of the mean-teacher consistency term (--cr_uncertainty) on the device: libpacingpseudo_unc.so entry by entry
against the float64 reference of tests/_unc_reference.py, the engine step against the float64 oracle, off = the parent's step,
hipGraph replay, --resume and a bf16 student.

Tolerances ("Uncertainty mask"): TOL_NOISE and TOL_UNC are twice the largest deviation measured against the
float64 reference on the device over every case of this file, rounded up to one digit; the kernel's own output on another path is
never the yardstick.  Measured: noise 1.531e-7 (sigma = 0.1, values up to 0.35: the fp32 rounding of the Box-Muller angle, up to
2.4e-7 rad, times a radius of up to 5.5 sigma), entropy 5.410e-7 (values up to 2.8)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pacing_oracle as O  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests import _teacher_reference as T  # noqa: E402
from tests import _unc_reference as R  # noqa: E402
from tests.test_gpu_step import TOL_OUT, build_model, check_grads, iteration, oracle_with_device_branches  # noqa: E402
from tests.test_gpu_teacher import _adam, _args, _cuda, _shadow, _step  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_NOISE = 4e-7          # measured 1.531e-7
TOL_UNC = 2e-6            # measured 5.410e-7
BAND_CAP = 0.005           # at most 0.5 % of a case's pixels may lie within the tolerance of the threshold
SEED = 0x1234_5678_9ABC_DEF1


def dev():
    return torch.device('cuda', 0)


# ---------------------------------------------------------------- 1. noise
_NOISE_REF = {}


def _noise_ref(n, step, p, clip):
    key = (n, step, p, clip)
    if key not in _NOISE_REF:
        _NOISE_REF[key] = R.noise(n, 0.1, clip, SEED, step, p)
    return _NOISE_REF[key]


def _device_noise(n, step, p, clip, offset=0, image=None):
    from pacingpseudo_amd.utils import add_noise
    buf = torch.zeros(n + offset, device=dev()) if image is None else image
    x = buf[offset:offset + n]
    assert x.data_ptr() % 16 == (4 * offset) % 16
    return add_noise(x, 0.1, clip, SEED, step, p)


@pytest.mark.parametrize('step', [0, 2 ** 32 + 5])
@pytest.mark.parametrize('p', [0, 3])
@pytest.mark.parametrize('n,offset', [(35, 0), (1024, 0), (1027, 1)])
def test_noise_values_against_float64(n, offset, p, step):
    """out - 0 = clamp(sigma n) against the reference, unclamped (clip 10) and with the clamp engaged on both sides (clip 0.05)."""
    for clip in (10.0, 0.05):
        got = _device_noise(n, step, p, clip, offset).double().cpu().numpy()
        ref = _noise_ref(n, step, p, clip)
        err = float(np.abs(got - ref).max())
        print(f'noise n={n} offset={offset} pass={p} step={step} clip={clip}: max |dev - f64| = {err:.3e} (max |ref| {np.abs(ref).max():.3f})')
        assert err <= TOL_NOISE
        if clip == 0.05 and n >= 1024:
            assert got.min() == np.float32(-0.05) and got.max() == np.float32(0.05) and (np.abs(got) < 0.049).any()


def test_noise_vector_and_scalar_paths_agree_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    base = torch.randn(1028, generator=g).to(dev())
    shifted = torch.empty(1029, device=dev())
    shifted[1:] = base                                  # the same values one float off a 16-byte boundary
    for p, step in ((0, 0), (3, 2 ** 32 + 5)):
        a = _device_noise(1027, step, p, 0.05, 0, base)             # float4 path + scalar tail
        b = _device_noise(1027, step, p, 0.05, 1, shifted[:1028])   # 4-byte accesses throughout
        assert torch.equal(a, b)
        assert torch.equal(a, _device_noise(1027, step, p, 0.05, 0, base))      # the same state, the same bits
        assert not torch.equal(a, base[:1027])
        # a value depends on the element index alone: the first 35 of 1027 are the 35 of a call of their own
        assert torch.equal(a[:35], _device_noise(35, step, p, 0.05, 0, base))


def test_advance_moves_to_the_noise_of_the_next_step():
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._unc import unc
    from pacingpseudo_amd.utils.uncertainty import state_tensor
    x = torch.zeros(1024, device=dev())
    for step in (0, 2 ** 32 - 1):
        state = state_tensor(SEED, step, dev())
        out = torch.empty_like(x)
        unc.punc_advance(state.data_ptr(), stream_ptr())
        unc.punc_noise_add(x.data_ptr(), 1024, 0.1, 10.0, state.data_ptr(), 1, out.data_ptr(), stream_ptr())
        assert [int(v) & (2 ** 64 - 1) for v in state.tolist()] == [SEED, step + 1]
        assert torch.equal(out, _device_noise(1024, step + 1, 1, 10.0))
        assert not torch.equal(out, _device_noise(1024, step, 1, 10.0))


# ---------------------------------------------------------------- 2. accumulate / mask
SHAPES = [(2, 2, 35), (2, 5, 256), (1, 9, 64), (1, 17, 64), (2, 32, 35)]
_ACC = {}


def _acc_case(N, K, HW, passes, saturated=False):
    """(logits list fp32 CPU, valid mask, float64 entropy, theta); made once and never modified."""
    key = (N, K, HW, passes, saturated)
    if key not in _ACC:
        g = torch.Generator().manual_seed(1000 * K + 10 * HW + passes + (7 if saturated else 0))
        zs = [3.0 * torch.randn(N, K, HW, 1, generator=g) for _ in range(passes)]
        if saturated:
            for z in zs:
                z[:, 0, ::3] = 80.0
                z[:, 1:, ::3] = -80.0
                z[:, 1, 1::7] = -80.0
        valid = (torch.rand(N, 1, HW, 1, generator=g) > 0.3).float()
        u = R.entropy(R.mean_softmax([z.double().numpy() for z in zs]))[..., 0]          # (N, HW)
        # between two neighbouring entropies at the 60 % quantile: a mixed mask, and no pixel sits on the threshold (fixed by the
        # reference alone, before any device run)
        srt = np.sort(u.reshape(-1))
        i = int(0.6 * srt.size)
        theta = float(np.float32(0.5 * (srt[i - 1] + srt[i])))
        assert R.band_fraction(u, theta, TOL_UNC) <= BAND_CAP
        _ACC[key] = (zs, valid, u, theta)
    return _ACC[key]


def _accumulate(zs, theta, valid, poison=None, want_unc=True):
    """The binding itself (so that the workspace can be poisoned): mask (N,HW), unc (N,HW), stats (3,) float64."""
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._unc import unc
    N, K, HW = zs[0].shape[:3]
    nws = unc.punc_workspace_bytes(N, K, HW)
    assert nws == (N * HW + 255) // 256 * 24
    ws = torch.full((nws // 8,), float('nan') if poison is None else poison, device=dev(), dtype=torch.float64)
    acc = torch.full((N, K, HW), float('nan'), device=dev())
    mask = torch.full((N, HW), float('nan'), device=dev())
    u = torch.full((N, HW), float('nan'), device=dev()) if want_unc else None
    stats = torch.full((3,), float('nan'), device=dev(), dtype=torch.float64)
    vd = valid.to(dev()).contiguous() if valid is not None else None
    for t, z in enumerate(zs):
        zd = z.to(dev()).contiguous()
        unc.punc_accumulate(zd.data_ptr(), N, K, HW, t, len(zs), vd.data_ptr() if vd is not None else None, theta, acc.data_ptr(),
                            mask.data_ptr(), u.data_ptr() if u is not None else None, stats.data_ptr(), ws.data_ptr(), nws, stream_ptr())
    torch.cuda.synchronize()
    return mask, u, stats


@pytest.mark.parametrize('use_valid', [False, True])
@pytest.mark.parametrize('passes', [1, 3])
@pytest.mark.parametrize('N,K,HW', SHAPES)
def test_accumulate_against_float64(N, K, HW, passes, use_valid):
    zs, valid, u64, theta = _acc_case(N, K, HW, passes)
    _check_accumulate(zs, valid if use_valid else None, u64, theta)


def _check_accumulate(zs, valid, u64, theta):
    mask, u, stats = _accumulate(zs, theta, valid)
    ud = u.double().cpu().numpy()
    err = float(np.abs(ud - u64).max())
    print(f'accumulate {tuple(zs[0].shape[:3])} T={len(zs)} valid={valid is not None}: max |u - u64| = {err:.3e} (max u {u64.max():.3f})')
    assert np.isfinite(ud).all() and err <= TOL_UNC
    v = valid.double().numpy().reshape(u64.shape) if valid is not None else None
    ref_m = R.mask(u64, theta, v)
    clear = np.abs(u64 - theta) > TOL_UNC
    assert 1.0 - clear.mean() <= BAND_CAP
    md = mask.double().cpu().numpy()
    assert np.array_equal(md[clear], ref_m[clear])
    assert set(np.unique(md)) <= {0.0, 1.0} and 0 < md.sum() < md.size            # a mixed mask: both branches taken
    st = stats.cpu().numpy()
    assert st[0] == float(mask.double().sum())                                      # the device mask's own sum, exactly
    ref_st = R.stats(u64, ref_m, v)
    assert st[2] == ref_st[2] and abs(st[1] - ref_st[1]) <= TOL_UNC * ref_st[2] and abs(st[0] - ref_st[0]) <= (~clear).sum()
    # the same bits in a second run, from a workspace with other rubbish in it, and without the optional output
    mask2, _, stats2 = _accumulate(zs, theta, valid, poison=1e300, want_unc=False)
    assert torch.equal(mask, mask2) and torch.equal(stats.view(torch.int64), stats2.view(torch.int64))


@pytest.mark.parametrize('passes', [1, 3])
def test_accumulate_saturated_softmax(passes):
    """+-80 logits: soft-max entries that are exactly 0 in fp32 (terms that contribute 0) beside ordinary pixels."""
    zs, valid, u64, theta = _acc_case(2, 5, 256, passes, saturated=True)
    assert (u64 < 1e-30).any()
    _check_accumulate(zs, valid, u64, theta)


def test_threshold_extremes_and_the_masked_loss():
    from pacingpseudo_amd.losses import losses as L
    from pacingpseudo_amd.utils import uncertainty_mask
    zs, valid, u64, _ = _acc_case(2, 5, 256, 3)
    zd = [z.reshape(2, 5, 16, 16).to(dev()) for z in zs]
    vd = valid.reshape(2, 1, 16, 16).to(dev())
    m_all, st = uncertainty_mask(zd, 1e30, vd, return_stats=True)
    assert m_all.shape == (2, 1, 16, 16) and torch.equal(m_all, vd) and float(st[0]) == float(vd.sum()) == float(st[2])
    assert torch.equal(uncertainty_mask(zd, 1e30), torch.ones_like(vd))
    m_none, u, st = uncertainty_mask((lambda t: zd[t], 3), 0.0, vd, return_uncertainty=True, return_stats=True)
    assert float(m_none.abs().sum()) == 0.0 and float(st[0]) == 0.0 and float(np.abs(u.double().cpu().numpy() - u64.reshape(2, 16, 16)).max()) <= TOL_UNC
    student = zd[0].clone().requires_grad_(True)
    for variant in ('ce_loss', 'js_loss', 'hard_ce_loss'):
        student.grad = None
        loss = L.teacher_consistency_loss(student, zd[1], variant, valid_mask=m_none)
        loss.backward()
        assert float(loss) == 0.0 and float(student.grad.abs().max()) == 0.0
        student.grad = None
        loss = L.teacher_consistency_loss(student, zd[1], variant, valid_mask=m_all)
        loss.backward()
        assert float(loss) > 0.0 and float(student.grad.abs().max()) > 0.0


# ---------------------------------------------------------------- 3. the engine step against float64
EPOCH_MID = 40             # inside the ramp: theta = (start + (1 - start) * exp(-scale / 2)) ln K, well below ln K


HEAD_GAIN = 20.0           # the 1x1 head of a freshly initialised network times this: entropies spread over (0, ln K) instead of
                           # huddling within 0.01 of ln K, where every threshold keeps nearly all pixels or nearly none


def _start_at_median(out, args, epoch):
    """`start` that puts theta(epoch) at the median entropy of the clean teacher prediction of a step's outputs: the threshold then
    cuts through the distribution."""
    p = torch.softmax(out['segmentation/logits_teacher'].detach().double(), 1)
    u = -(p * torch.log(p.clamp_min(1e-300))).sum(1)
    ramp = math.exp(-args.ramp_up_scale * (1 - epoch / 80)) if epoch < 80 else 1.0
    return min(1.0, max(0.05, (float(u.median()) / math.log(args.num_classes) - ramp) / (1 - ramp)))


def _median_start(args, batch, passes, sigma, epoch, seed_torch):
    model, opt = _unc_model(args, passes, sigma, start=1.0, seed_torch=seed_torch)
    model.train()
    return _start_at_median(_step(model, opt, batch, args, epoch), args, epoch)


def _unc_model(args, passes, sigma, start=0.9, seed_torch=2):
    torch.manual_seed(seed_torch)
    model = build_model(args)
    model.backbone.final_conv.weight.data.mul_(HEAD_GAIN)
    model.engine.invalidate_packed()
    opt = _adam(model, args, lr=1e-3)
    model.attach_teacher(opt, uncertainty=dict(passes=passes, sigma=sigma, clip=0.2, start=start, seed=SEED))
    return model, opt


@pytest.mark.parametrize('passes,sigma', [(2, 0.1), (1, 0.0)])
@pytest.mark.parametrize('variant', ['ce_loss', 'js_loss', 'hard_ce_loss'])
@pytest.mark.parametrize('bn_training', [True, False])
def test_step_against_float64(variant, bn_training, passes, sigma, monkeypatch):
    """B = 2 at 32 x 32, K = 5, the small network after two optimizer steps.  The device's mask against the reference entropy of
    the float64 teacher on the reference's noisy inputs (outside the band); loss_cr, every output and every gradient against the
    float64 oracle evaluated WITH the device's mask, at the bounds tests/test_gpu_teacher.py uses for the unmasked term; partial CE
    and entropy bit-identical to the step with the mask off; the shadow untouched.  `start` puts theta at the median entropy of the
    teacher's prediction one step earlier, so that the threshold cuts through the distribution instead of keeping every pixel."""
    from pacingpseudo_amd.utils import uncertainty_threshold
    args = _args('small', loss_cr_variants=variant)
    B, H, W, K = 2, 32, 32, args.num_classes
    model, opt = _unc_model(args, passes, sigma)
    eng = model.engine
    batch = O.synthetic_batch(B, H, W, seed=9, keep=0.08)
    batch['valid_mask'][:, :, :, :5] = 0
    model.train()
    for _ in range(2):
        out = _step(model, opt, _cuda(batch), args, EPOCH_MID)
    assert eng.uncertainty_state() == (SEED, 2 if sigma else 0)
    start = _start_at_median(out, args, EPOCH_MID)
    model.set_uncertainty(passes, sigma=sigma, clip=0.2, start=start, seed=SEED)
    assert eng.uncertainty_state() == (SEED, 0)
    theta = uncertainty_threshold(EPOCH_MID, start, K, args.ramp_up_scale)
    model.train(bn_training)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ema_sd = opt.ema_state_dict(model)
    shadow0 = _shadow(model, opt).clone()

    # partial CE / entropy with the mask on and off, from the same weights (forward + backward, no optimizer step)
    probe = {}
    for tag in ('on', 'off'):
        if tag == 'off':
            model.set_uncertainty(None)
        out = model(_cuda(batch), mode='train', step=EPOCH_MID)
        assert ('segmentation/uncertainty_mask' in out) == (tag == 'on') and list(out) == model._expected_keys('train')
        opt.zero_grad()
        (out['loss_pce'] + out['loss_ent'] + out['loss_cr']).backward()
        probe[tag] = {k: out[k].detach().clone() for k in ('loss_pce', 'loss_ent', 'loss_cr')}
        assert torch.equal(_shadow(model, opt), shadow0)          # no gradient step, no write: the teacher is a constant
        # the probe moved the memory bank and (train mode) the running statistics the teacher reads: put them back
        model.load_state_dict({k: v.clone() for k, v in sd.items()})
        model.train(bn_training)
        _shadow(model, opt).copy_(shadow0)
    assert torch.equal(probe['on']['loss_pce'], probe['off']['loss_pce']) and torch.equal(probe['on']['loss_ent'], probe['off']['loss_ent'])
    assert not torch.equal(probe['on']['loss_cr'], probe['off']['loss_cr'])
    model.set_uncertainty(passes, sigma=sigma, clip=0.2, start=start, seed=SEED)

    rec, grads = iteration(model, opt, batch, args, EPOCH_MID)
    assert eng.uncertainty_state() == (SEED, 1 if sigma else 0)
    m_dev = rec['segmentation/uncertainty_mask'].cpu()
    assert m_dev.shape == (B, 1, H, W)
    # reference: the float64 teacher on the reference's noisy inputs of step 0
    img = batch['image'].double().numpy()
    if sigma:
        zs = [T.teacher_logits(sd, ema_sd, torch.from_numpy(R.add_noise(img, sigma, 0.2, SEED, 0, t)), args).numpy() for t in range(passes)]
    else:
        zs = [T.teacher_logits(sd, ema_sd, batch['image'], args).numpy()]
    u64 = R.entropy(R.mean_softmax(zs))                                        # (B, H, W)
    v = batch['valid_mask'].double().numpy().reshape(B, H, W)
    ref_m = R.mask(u64, theta, v)
    clear = np.abs(u64 - np.float32(theta)) > TOL_UNC
    md = m_dev.double().numpy().reshape(B, H, W)
    kept = md.sum() / v.sum()
    wrong = int((md[clear] != ref_m[clear]).sum())
    print(f'{variant} bn_training={bn_training} T={passes} sigma={sigma}: theta {theta:.4f}, kept {kept:.3f}, in band {(~clear).sum()}, '
          f'mask bits off outside the band {wrong}')
    assert 1.0 - clear.mean() <= BAND_CAP
    assert 0.05 < kept < 0.95, 'the threshold does not cut through the entropy distribution'
    assert wrong == 0
    # the oracle with the device's mask on the teacher call
    zt = rec['segmentation/logits_teacher'].cpu()
    oargs = _args('small', loss_cr_variants='kl_loss')
    monkeypatch.setattr(O, 'kl_loss', lambda a, b, m=None: T.teacher_consistency(a, zt.double(), variant, m_dev.double()))
    ref_out, _, _ = O.train_step({k: v_.clone() for k, v_ in sd.items()}, batch, EPOCH_MID, oargs, training=bn_training)
    assert float(ref_out['loss_cr']) > 0
    for k, val in ref_out.items():
        if k.startswith('_') or not torch.is_tensor(val):
            continue
        e = G.rel_err(rec[k].double().cpu().numpy(), val.numpy())
        print(f'  {k}: rel err {e:.3e}')
        assert e < TOL_OUT, f'{k}: rel err {e:.3e}'
    _, og, _ = oracle_with_device_branches(model, sd, batch, EPOCH_MID, oargs, bn_training)
    worst = check_grads(grads, {k: val.numpy() for k, val in og.items() if val is not None}, bn_training)
    print(f'  worst gradient: {worst}')


# ---------------------------------------------------------------- 4. off is off
def _launch_log(mode):
    """mode: 'never' (set_uncertainty never called), 'zero' (configured, then T = 0), 'on'."""
    from pacingpseudo_amd import _unc
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
        model.attach_teacher(opt)
        if mode == 'zero':
            model.set_uncertainty(0, sigma=0.1, clip=0.2, start=0.75, seed=1)
        if mode == 'on':
            model.set_uncertainty(2, sigma=0.1, clip=0.2, start=0.75, seed=1)
        model.train()
        out = _step(model, opt, _cuda(O.synthetic_batch(2, 32, 32, seed=5, keep=0.08)), args)
        torch.cuda.synchronize()
        loaded = _unc.unc._dll is not None
    finally:
        E.lib_for, E.lib = real, real_lib
    return log, list(out), model.flat.params.clone(), loaded


def test_off_is_the_step_as_it_was(monkeypatch):
    from pacingpseudo_amd import _unc
    monkeypatch.setattr(_unc.unc, '_dll', None)              # whatever earlier tests loaded: this step must not need it
    for k in [k for k, v in vars(_unc.unc).items() if callable(v)]:
        monkeypatch.delattr(_unc.unc, k)                     # (cached wrappers)
    never, zero = _launch_log('never'), _launch_log('zero')
    assert len(never[0]) > 100 and not never[3] and not zero[3]
    assert never[0] == zero[0] and never[1] == zero[1] and torch.equal(never[2], zero[2])
    assert 'segmentation/uncertainty_mask' not in never[1]
    on = _launch_log('on')
    assert on[3] and on[1].index('segmentation/uncertainty_mask') == on[1].index('segmentation/logits_teacher') + 1
    assert [k for k in on[1] if k != 'segmentation/uncertainty_mask'] == never[1]
    names = lambda log: [e for e, _ in log]      # noqa: E731
    count = lambda log, e: names(log).count(e)   # noqa: E731
    # on, T = 2: two more teacher forwards (image pack, head), the weight packs once per step as before, the same backward
    for entry, extra in (('pp_pack_image_nchw_to_nhwc', 2), ('pp_conv1x1_nhwc_to_nchw_fwd', 2), ('pp_seg_losses_fwd', 0), ('pp_seg_losses_bwd', 0),
                         ('pp_losses_finalize', 0), ('pp_pack_conv3x3_weights_f16x3_batch', 0), ('pp_wino_pack_weights_f16x3_batch', 0)):
        assert count(on[0], entry) == count(never[0], entry) + extra, entry
    for entry in sorted({e for e in names(never[0]) if 'bwd' in e}):
        assert count(on[0], entry) == count(never[0], entry), entry


# ---------------------------------------------------------------- 5. replay and resume
def test_graph_replay_equals_eager_and_draws_new_noise():
    """Two eager calls, a capture, three replays against five eager steps: losses, masks, parameters, shadow and the step counter bit
    for bit; the masks of consecutive replays of the SAME batch differ, so the noise advanced inside the graph."""
    from pacingpseudo_amd.graph import GraphedStep
    from tests.test_gpu_graph import _loss_fn
    args = _args('small', loss_cr_variants='js_loss')
    f = _loss_fn(args)
    b = _cuda(O.synthetic_batch(2, 64, 64, seed=3, keep=0.05))
    runs = {}
    start = _median_start(args, b, 2, 0.1, EPOCH_MID, 1)
    for tag in ('eager', 'graph'):
        model, opt = _unc_model(args, 2, 0.1, start=start, seed_torch=1)
        gs = GraphedStep(model, opt, f, warmup=2) if tag == 'graph' else None
        model.train()
        cr, masks = [], []
        for i in range(5):
            if gs is not None:
                out = gs(b, EPOCH_MID)[1]
            else:
                out = _step_fn(model, opt, b, f)
            cr.append(out['loss_cr'].detach().clone())
            masks.append(out['segmentation/uncertainty_mask'].detach().clone())
        torch.cuda.synchronize()
        assert model.engine.uncertainty_state() == (SEED, 5)          # the replays advanced the step on the device
        runs[tag] = dict(cr=torch.stack(cr).cpu(), masks=torch.stack(masks).cpu(), params=model.flat.params.clone(),
                         shadow=_shadow(model, opt).clone())
        if gs is not None:
            assert (gs.captures, gs.replays) == (1, 3), (gs.captures, gs.replays)
            key = gs._key(b, EPOCH_MID)
            assert key == gs.key and model.engine.uncertainty_key() in key
            model.set_uncertainty(2, sigma=0.2, clip=0.2, start=start, seed=SEED)
            assert gs._key(b, EPOCH_MID) != key
    e, g = runs['eager'], runs['graph']
    assert torch.equal(e['cr'], g['cr']) and torch.equal(e['masks'], g['masks'])
    assert torch.equal(e['params'], g['params']) and torch.equal(e['shadow'], g['shadow'])
    for i in (2, 3):           # replays: calls 3, 4, 5 (indices 2 .. 4)
        assert not torch.equal(g['masks'][i], g['masks'][i + 1])
    assert 0 < float(g['masks'].mean()) < 1


def _step_fn(model, opt, b, f):
    out = model(b, mode='train', step=EPOCH_MID)
    loss = f(out, EPOCH_MID)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return out


def test_resume_is_bit_identical_and_refuses_a_changed_flag(tmp_path):
    """Three epochs straight against two epochs + --resume from state_1 + one epoch: weights, shadow (optimizer state), scalars and
    the saved (seed, step) bit for bit; CR/uncertainty_kept in [0, 1]; a changed --cr_uncertainty is refused by name."""
    from tests.test_gpu_resume import FULL, _driver, _resume_case, _scalars
    argv = (['--synthetic', '8', '--image_size', '32', '--epoch', '3', '--batch_size', '4', '--num_workers', '0'] + FULL
            + ['--ema_decay', '0.9', '--cr_teacher', 'ema', '--cr_uncertainty', '2'])
    full, copy, st = _resume_case(tmp_path, 'train_chaos.py', argv, 1, 2)
    assert st['args']['cr_uncertainty'] == 2
    seed, step = st['uncertainty_state']
    assert step == 3 * 2 and seed == 1                               # 8 images / batch 4 = two steps per epoch; --seed 1
    from tests.test_gpu_resume import _load
    resumed = _load(os.path.join(copy, 'ckps', 'state_2.pth'))
    assert resumed['uncertainty_state'] == st['uncertainty_state']
    assert _load(os.path.join(copy, 'ckps', 'state_1.pth'))['uncertainty_state'] == [1, 4]
    sc = _scalars(full)
    for e in range(3):
        assert 0.0 <= sc[('CR/uncertainty_kept', e)] <= 1.0 and 0.0 <= sc[('CR/uncertainty_mean', e)] <= math.log(5)
    assert 'uncertainty threshold theta' in open(os.path.join(full, 'log.txt')).read()
    changed = [('4' if a == '2' and argv[i - 1] == '--cr_uncertainty' else a) for i, a in enumerate(argv)]
    r = _driver('train_chaos.py', changed + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'resumed'),
                                             '--resume', os.path.join(copy, 'ckps', 'state_1.pth')])
    assert r.returncode == 2 and '--cr_uncertainty (saved 2, now 4)' in r.stderr


def test_state_file_without_the_feature_has_no_new_key():
    """resume.capture adds `uncertainty_state` only while the mask is on."""
    from pacingpseudo_amd import resume
    args = _args('small')
    model, opt = _unc_model(args, 2, 0.1)
    rng = [resume.rng_states(dev())]
    on = resume.capture(args, 0, model, opt, (0.0, 0, []), np.zeros(1), rng, 1)
    model.set_uncertainty(None)
    off = resume.capture(args, 0, model, opt, (0.0, 0, []), np.zeros(1), rng, 1)
    assert set(on) - set(off) == {'uncertainty_state'} and on['uncertainty_state'] == [SEED, 0]


# ---------------------------------------------------------------- 6. a bf16 student
def test_bf16_student_has_the_mask_of_the_fp32_student():
    """--storage bf16: one step runs; the teacher plan -- the noisy passes included -- is fp32 either way, so the mask is bitwise
    the fp32 student's."""
    a32, a16 = _args('full'), _args('full')
    a16.storage = 'bf16'
    torch.manual_seed(1)
    m32 = build_model(a32)
    m32.backbone.final_conv.weight.data.mul_(HEAD_GAIN)
    m16 = build_model(a16, {k: v.detach().cpu().numpy() for k, v in m32.state_dict().items()})
    b = _cuda(O.synthetic_batch(2, 32, 32, seed=11, keep=0.08))
    masks = {}
    start = None
    state = {k: v.detach().cpu().numpy() for k, v in m32.state_dict().items()}
    for name, m, a in (('probe', build_model(_args('full'), state), _args('full')), ('fp32', m32, a32), ('bf16', m16, a16)):
        opt = _adam(m, a)
        m.attach_teacher(opt, uncertainty=dict(passes=2, sigma=0.1, clip=0.2, start=start or 1.0, seed=SEED))
        _shadow(m, opt).mul_(1.0 + 2.0 ** -6)
        m.train()
        if name == 'probe':      # a third model with the same weights, only to place the threshold at its median entropy
            start = _start_at_median(m(b, mode='train', step=0), a, 0)
            continue
        out = m(b, mode='train', step=0)
        sum(out[k] for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory')).backward()
        torch.cuda.synchronize()
        plan = m.engine.last_plan
        assert plan.storage == name and plan.teacher_plan.storage == 'fp32'
        assert bool(torch.isfinite(out['loss_cr']))
        masks[name] = out['segmentation/uncertainty_mask'].detach().clone()
    assert torch.equal(masks['fp32'], masks['bf16'])
    assert 0 < float(masks['fp32'].sum()) < masks['fp32'].numel()
