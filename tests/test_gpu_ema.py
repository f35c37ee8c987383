"""Device-side EMA weight averaging (FusedAdam / FusedSGD ``ema_decay``, ``--ema_decay``) on the MI355X.

The rule is three separately rounded fp32 operations, ``e + fl32(w * fl32(p - e))`` with ``w = (float)(1 - min(D, (1 + t) /
(10 + t)))``, so the kernels are compared BIT FOR BIT with the torch CPU fp32 chain and with each other (fused against unfused,
graph replay against eager, resumed against uninterrupted).  Against float64 the parameters keep the bound of
tests/test_gpu_clip.py:225 (rtol 2e-6, atol 1e-8) and the shadow gets that bound plus 20 * 2^-23 * max|e|: twenty updates of at
most one ulp each -- a derived bound, not a measured one.
"""
import glob
import json
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests.test_gpu_step import build_model, iteration  # noqa: E402


def _small_args():
    return O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])


def _small_batch():
    return O.synthetic_batch(2, 64, 64, seed=4, keep=0.05)


def _w(t, decay):
    """The weight of the update after t earlier ones, restated: double arithmetic, one rounding to fp32."""
    return struct.unpack('f', struct.pack('f', 1.0 - min(decay, (1.0 + t) / (10.0 + t))))[0]


def _chain(e, p, t, decay):
    """torch CPU fp32: e + w * (p - e), every operation rounded on its own."""
    e, p = e.cpu(), p.cpu()
    assert e.dtype == p.dtype == torch.float32
    return e + torch.tensor(_w(t, decay), dtype=torch.float32) * (p - e)


def _values(n, seed):
    rng = np.random.RandomState(seed)
    v = (10.0 ** rng.uniform(-6, 2, size=n)) * rng.choice([-1.0, 1.0], size=n)
    return torch.from_numpy(v.astype(np.float32))


@pytest.mark.parametrize('decay', [0.9, 0.999])
def test_ema_update_kernel_against_the_cpu_chain(decay):
    """1: n in {1, 3, 4, 1027, 2^20 + 1}; t inside the warm-up (3; 100 is inside it for D = 0.999 and past it for D = 0.9) and
    far past it (10^4), as a host value and as a device step count.  Bit for bit; elements outside [0, n) untouched."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    pad = 8                                                         # floats in front of and behind the range (keeps 16-byte alignment)
    for i, n in enumerate((1, 3, 4, 1027, 2 ** 20 + 1)):
        p = _values(n, seed=20 + i)
        e0 = _values(n, seed=40 + i)
        for t in (0, 3, 100, 10 ** 4):
            want = _chain(e0, p, t, decay)
            for on_device in (False, True):
                pbuf = torch.full((n + 2 * pad,), 7.25, device='cuda')
                ebuf = torch.full((n + 2 * pad,), -3.5, device='cuda')
                pbuf[pad:pad + n] = p.cuda()
                ebuf[pad:pad + n] = e0.cuda()
                steps = torch.tensor([t], device='cuda', dtype=torch.int32)
                lib.pp_ema_update(pbuf.data_ptr() + 4 * pad, ebuf.data_ptr() + 4 * pad, n, decay,
                                  steps.data_ptr() if on_device else None, -1 if on_device else t, stream_ptr())
                torch.cuda.synchronize()
                got = ebuf.cpu()
                assert torch.equal(got[pad:pad + n], want), (n, t, on_device)
                assert bool((got[:pad] == -3.5).all()) and bool((got[pad + n:] == -3.5).all()), (n, t, on_device)
                assert torch.equal(pbuf.cpu()[pad:pad + n], p) and int(steps) == t      # p and the count are only read
    assert _w(3, decay) > _w(10 ** 4, decay) == struct.unpack('f', struct.pack('f', 1.0 - decay))[0]


def test_slab_swap_kernel():
    """a <-> b in place, tails and neighbours included."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    for n in (1, 3, 4, 1027, 2 ** 20 + 1):
        a0, b0 = _values(n + 8, seed=n % 97), _values(n + 8, seed=n % 89 + 100)
        a, b = a0.cuda(), b0.cuda()
        lib.pp_slab_swap(a.data_ptr() + 16, b.data_ptr() + 16, n, stream_ptr())
        torch.cuda.synchronize()
        wa, wb = a0.clone(), b0.clone()
        wa[4:4 + n], wb[4:4 + n] = b0[4:4 + n], a0[4:4 + n]
        assert torch.equal(a.cpu(), wa) and torch.equal(b.cpu(), wb), n


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_fused_step_equals_plain_step_then_ema_update(kind, clip):
    """2: pp_*_step_ema against pp_*_step_dev / _clip followed by pp_ema_update(t = the count before the step), five consecutive
    steps from t = 0; p, m, v / buf, e and the step count bit for bit."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    n = 2 ** 18 + 3                                                 # a tail of three elements
    decay = 0.9
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).cuda()
    keys = ('p', 'm', 'v', 'e') if kind == 'adam' else ('p', 'm', 'e')
    runs = {tag: dict({k: torch.zeros(n, device='cuda') for k in keys}, steps=torch.zeros(1, device='cuda', dtype=torch.int32))
            for tag in ('fused', 'plain')}
    for r in runs.values():
        r['p'].copy_(p0)
        r['e'].copy_(p0)
    lr_dev = torch.full((1,), 3e-3, device='cuda')
    coef = torch.full((1,), 0.37, device='cuda')
    clip_dev = coef.data_ptr() if clip else None
    st = stream_ptr()

    def common(r, g):
        if kind == 'adam':
            return (r['p'].data_ptr(), g.data_ptr(), r['m'].data_ptr(), r['v'].data_ptr(), n, 3e-3, lr_dev.data_ptr(), 0.9, 0.999, 1e-8,
                    3e-4, r['steps'].data_ptr(), None, 1)
        return (r['p'].data_ptr(), g.data_ptr(), r['m'].data_ptr(), n, 3e-3, lr_dev.data_ptr(), 0.9, 3e-4, r['steps'].data_ptr(), None, 1)

    base = 'pp_adam_step' if kind == 'adam' else 'pp_sgd_momentum_step'
    for it in range(5):
        g = (torch.randn(n, generator=gen) * 10.0 ** float(it - 2)).cuda()
        f, q = runs['fused'], runs['plain']
        getattr(lib, base + '_ema')(*common(f, g), f['e'].data_ptr(), decay, clip_dev, st)
        if clip:
            getattr(lib, base + '_clip')(*common(q, g), clip_dev, st)
        else:
            getattr(lib, base + '_dev')(*common(q, g), st)
        lib.pp_ema_update(q['p'].data_ptr(), q['e'].data_ptr(), n, decay, None, it, st)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(f[k], q[k]), (it, k)
        assert int(f['steps']) == int(q['steps']) == it + 1
    assert not torch.equal(runs['fused']['e'], runs['fused']['p'])   # the average lags: not a vacuous comparison


def _run_steps(opt_cls, steps, args=None, batch=None, **kw):
    from pacingpseudo_amd import optim
    args = _small_args() if args is None else args
    torch.manual_seed(3)
    model = build_model(args)
    opt = getattr(optim, opt_cls)(model.parameters(), **kw)
    batch = _small_batch() if batch is None else batch
    losses = []
    for _ in range(steps):
        rec, _ = iteration(model, opt, batch, args, 0)
        losses.append(rec['total_loss'].reshape(1))
    torch.cuda.synchronize()
    return model, opt, torch.cat(losses).cpu()


@pytest.mark.parametrize('opt_cls,kw,storage', [('FusedAdam', dict(lr=1e-3, weight_decay=3e-4), 'fp32'),
                                                ('FusedSGD', dict(lr=1e-2, momentum=0.9, weight_decay=3e-4), 'fp32'),
                                                ('FusedAdam', dict(lr=1e-3, weight_decay=3e-4), 'bf16')])
def test_training_does_not_depend_on_the_average(opt_cls, kw, storage):
    """3: three whole training steps with ema_decay = 0.9 and three without, from the same seed: parameters, optimizer state,
    step counts and losses identical.  fp32 storage (small widths) and bf16 storage (the model and batch of tests/test_gpu_h16.py)."""
    args = batch = None
    if storage != 'fp32':
        args = O.full_flags()
        args.storage = storage
        batch = O.synthetic_batch(2, 128, 128, seed=3, keep=0.05)
    m_off, o_off, l_off = _run_steps(opt_cls, 3, args, batch, **kw)
    m_on, o_on, l_on = _run_steps(opt_cls, 3, args, batch, ema_decay=0.9, **kw)
    if storage != 'fp32':
        assert m_on.engine.last_plan.h16
    assert torch.equal(m_off.flat.params, m_on.flat.params)
    s_off, s_on = o_off.state_dict()['slabs'][0], o_on.state_dict()['slabs'][0]
    for k in o_off.STATE_KEYS:
        assert torch.equal(s_off[k], s_on[k]), k
    assert s_off['steps'] == s_on['steps'] == {'backbone': 3, 'aux_path': 3}
    assert torch.equal(l_off, l_on), (l_off, l_on)
    assert 'ema' in s_on and 'ema' not in s_off
    assert s_on['ema'].shape == m_on.flat.params.shape and s_on['ema'].dtype == torch.float32
    assert not torch.equal(s_on['ema'], m_on.flat.params.cpu())     # and the average is not simply the last iterate


@pytest.mark.parametrize('opt_cls', ['FusedSGD', 'FusedAdam'])
def test_parameters_and_shadow_against_torch_in_float64(opt_cls):
    """4: gradients from the device, torch.optim.SGD / Adam in float64 plus the rule in double on copies, 20 steps.  Parameters:
    rtol 2e-6, atol 1e-8 (tests/test_gpu_clip.py:225); shadow: that plus 20 * 2^-23 * max|e|."""
    from pacingpseudo_amd import optim
    decay, steps = 0.9, 20
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=3e-4) if opt_cls == 'FusedSGD' else dict(lr=1e-3, weight_decay=3e-4)
    args = _small_args()
    batch = _small_batch()
    torch.manual_seed(3)
    model = build_model(args)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    ref_params = {k: torch.nn.Parameter(p.detach().cpu().double().clone()) for k, p in named}
    ref_ema = {k: p.detach().cpu().double().clone() for k, p in named}
    ref_opt = (torch.optim.SGD if opt_cls == 'FusedSGD' else torch.optim.Adam)(list(ref_params.values()), **kw)
    opt = getattr(optim, opt_cls)(model.parameters(), ema_decay=decay, **kw)
    for t in range(steps):
        _, grads = iteration(model, opt, batch, args, 0)
        for k, p in ref_params.items():
            p.grad = grads[k].cpu().double().clone()
        ref_opt.step()
        w = 1.0 - min(decay, (1.0 + t) / (10.0 + t))
        for k, p in ref_params.items():
            ref_ema[k] += w * (p.detach() - ref_ema[k])
    torch.cuda.synchronize()
    flat = model.flat
    shadow = next(iter(opt._slabs.values()))['ema']
    worst_p = worst_e = 0.0
    for k, p in named:
        got, ref = p.detach().cpu().double(), ref_params[k].detach()
        worst_p = max(worst_p, float(((got - ref).abs() - 2e-6 * ref.abs()).max()))
        o = flat.offsets[p]
        got_e, ref_e = shadow[o:o + p.numel()].view(p.shape).cpu().double(), ref_ema[k]
        slack = steps * 2.0 ** -23 * float(ref_e.abs().max())
        worst_e = max(worst_e, float(((got_e - ref_e).abs() - 2e-6 * ref_e.abs() - slack).max()))
        assert torch.allclose(got, ref, rtol=2e-6, atol=1e-8), (k, float((got - ref).abs().max()))
        assert bool(((got_e - ref_e).abs() <= 1e-8 + 2e-6 * ref_e.abs() + slack).all()), (k, float((got_e - ref_e).abs().max()), slack)
        assert not torch.equal(got_e, got)
    print(f'{opt_cls}: worst |p - ref| - rtol |ref| = {worst_p:.3e} (atol 1e-8); worst shadow excess over rtol and slack = {worst_e:.3e}')


class _Recorder:
    """`lib` with the names of the entry points that were called."""

    def __init__(self, real):
        self._real, self.called = real, []

    def __getattr__(self, name):
        self.called.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize('opt_cls,kw,plain', [('FusedAdam', dict(lr=1e-3, weight_decay=3e-4), 'pp_adam_step_dev'),
                                              ('FusedSGD', dict(lr=1e-2, momentum=0.9, weight_decay=3e-4), 'pp_sgd_momentum_step_dev')])
def test_off_is_off(opt_cls, kw, plain, monkeypatch):
    """5: ema_decay=None allocates no shadow, calls exactly the entry points it called before the feature, and its state_dict has
    no `ema` key; with ema_decay on the *_ema entry point replaces the plain one."""
    from pacingpseudo_amd import optim
    rec = _Recorder(optim.lib)
    monkeypatch.setattr(optim, 'lib', rec)
    _, opt, _ = _run_steps(opt_cls, 2, **kw)
    assert set(rec.called) == {plain}, set(rec.called)
    state = next(iter(opt._slabs.values()))
    assert 'ema' not in state and all('ema' not in s for s in opt.state_dict()['slabs'])
    assert opt.param_groups[0]['ema_decay'] is None
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        with opt.ema_weights():
            pass
    rec.called.clear()
    _, opt, _ = _run_steps(opt_cls, 2, ema_decay=0.99, **kw)
    assert set(rec.called) == {plain.replace('_dev', '_ema')}, set(rec.called)
    assert 'ema' in next(iter(opt._slabs.values()))


def test_overflow_skipped_step_leaves_the_average_alone():
    """6: fp16 storage with loss scale 2^40 (the setup of test_gpu_clip.py::test_overflow_skip_with_clipping_on): the skipped step
    leaves the shadow (= the initial parameters) and the count untouched; the next, real step uses t = 0."""
    from pacingpseudo_amd.optim import FusedAdam
    a16 = O.full_flags()
    a16.storage = 'fp16'
    torch.manual_seed(1)
    m = build_model(a16)
    m.engine.loss_scale = 2.0 ** 40
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.0, ema_decay=0.999)
    batch = {k: v.cuda() for k, v in O.synthetic_batch(2, 128, 128, seed=3, keep=0.05).items() if k != 'label'}
    m.train()
    before = m.flat.params.clone()

    def step():
        out = m(batch, mode='train', step=0)
        loss = sum(out[k] for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'))
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    step()
    assert int(m.flat.guard[0]) == 1 and int(m.flat.guard[1]) == 1
    assert torch.equal(m.flat.params, before)
    st = next(iter(opt._slabs.values()))
    assert torch.equal(st['ema'], before)
    assert opt.state_dict()['slabs'][0]['steps'] == {}
    m.engine.set_loss_scale(1024.0)
    step()
    assert int(m.flat.guard[0]) == 0 and int(m.flat.guard[1]) == 1
    assert opt.state_dict()['slabs'][0]['steps'] == {'backbone': 1, 'aux_path': 1}
    assert not torch.equal(m.flat.params, before)
    assert torch.equal(st['ema'].cpu(), _chain(before, m.flat.params, 0, 0.999))       # w(0) = 0.9, not w(1)
    assert not torch.equal(st['ema'].cpu(), _chain(before, m.flat.params, 1, 0.999))


def _loss_fn(args):
    from pacingpseudo_amd.utils import gaussian_ramp_up

    def f(out, epoch):
        loss = out['loss_pce']
        loss = loss + out['loss_ent'] * gaussian_ramp_up(epoch, args.loss_ent_weight, scale=args.ramp_up_scale)
        loss = loss + out['loss_cr'] * gaussian_ramp_up(epoch, args.loss_cr_weight, scale=args.ramp_up_scale)
        return loss + out['loss_aux_cls'] * args.loss_aux_weight + out['loss_memory'] * args.loss_memory_weight
    return f


def test_graph_replay_equals_eager_with_the_average():
    """7: eager vs GraphedStep, four steps (one eager warm-up call, one capture, three replays): parameters, moments, shadow and
    step counts bit for bit; another ema_decay is another capture key."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = _small_args()
    f = _loss_fn(args)
    batch = {k: v.cuda() for k, v in _small_batch().items() if k != 'label'}
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(3)
        model = build_model(args)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=3e-4, ema_decay=0.9)
        gs = GraphedStep(model, opt, f, warmup=10 ** 9 if tag == 'eager' else 1)
        model.train()
        for _ in range(4):
            gs(batch, 0)
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(params=model.flat.params.clone().cpu(), m=sd['m'], v=sd['v'], ema=sd['ema'], steps=sd['steps'],
                         captures=gs.captures, replays=gs.replays)
        if tag == 'graph':
            key = gs._key(batch, 0)
            assert key == gs.key
            opt.param_groups[0]['ema_decay'] = 0.99
            assert gs._key(batch, 0) != key
            opt.param_groups[0]['ema_decay'] = None
            assert gs._key(batch, 0) != key
    e, g = runs['eager'], runs['graph']
    assert e['captures'] == 0 and g['captures'] == 1 and g['replays'] == 3
    for k in ('params', 'm', 'v', 'ema'):
        assert torch.equal(e[k], g[k]), k
    assert e['steps'] == g['steps'] == {'backbone': 4, 'aux_path': 4}
    assert not torch.equal(e['ema'], e['params'])


def _unet():
    from pacingpseudo_amd.models import UNet
    return UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                elab_end_points=True)


def _unet_step(net, opt, image, label):
    from pacingpseudo_amd.losses.losses import dice_loss_fn, partial_cross_entropy_loss
    logits = net(image)['segmentation/logits']
    loss = partial_cross_entropy_loss(logits, label.argmax(1).long(), 5) + dice_loss_fn(logits, label)
    opt.zero_grad()
    loss.backward()
    opt.step()


def test_ema_weights_context():
    """8: inside optimizer.ema_weights() a no-grad forward gives exactly the logits of a bare UNet loaded from ema_state_dict();
    after exit the parameters are what they were and the live logits come back; the next training step equals that of a twin
    that never entered the context (the version bump and the re-pack are right).  Not re-entrant; exits cleanly on an error."""
    from pacingpseudo_amd.optim import FusedAdam
    batch = O.synthetic_batch(3, 64, 64, seed=8)
    image, label = batch['image'].cuda(), batch['label'].cuda()
    twins = []
    for _ in range(2):
        torch.manual_seed(4)
        net = _unet().cuda()
        opt = FusedAdam(net.parameters(), lr=1e-3, weight_decay=3e-4, ema_decay=0.9)
        for _ in range(3):
            _unet_step(net, opt, image, label)
        twins.append((net, opt))
    (net, opt), (twin, twin_opt) = twins
    flat = net._flat
    assert torch.equal(flat.params, twin._flat.params)
    net.eval()
    twin.eval()
    before = flat.params.clone()
    shadow = next(iter(opt._slabs.values()))['ema']
    shadow_before = shadow.clone()
    assert not torch.equal(before, shadow_before)
    with torch.no_grad():
        live = net(image)['segmentation/logits'].clone()            # the forward-only plan has packed the live weights
    sd = opt.ema_state_dict(net)
    assert list(sd) == list(net.state_dict()) and all(not v.is_cuda for v in sd.values())
    assert torch.equal(flat.params, before) and torch.equal(shadow, shadow_before)
    for k, v in net.state_dict().items():                            # buffers come from the live model, parameters from the average
        if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
            assert torch.equal(sd[k], v.cpu()), k
    version = flat.version
    with opt.ema_weights():
        assert flat.version == version + 1
        assert torch.equal(flat.params, shadow_before) and torch.equal(shadow, before)
        with torch.no_grad():
            inside = net(image)['segmentation/logits'].clone()
        with pytest.raises(RuntimeError, match='not re-entrant'):
            with opt.ema_weights():
                pass
        assert torch.equal(flat.params, shadow_before)              # the refused entry swapped nothing
    assert flat.version == version + 2
    assert torch.equal(flat.params, before) and torch.equal(shadow, shadow_before)
    bare = _unet().cuda().eval()
    bare.load_state_dict(sd)
    with torch.no_grad():
        want = bare(image)['segmentation/logits']
        again = net(image)['segmentation/logits']
    assert torch.equal(inside, want)
    assert not torch.equal(inside, live) and torch.equal(again, live)
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert torch.equal(flat.params, before) and torch.equal(shadow, shadow_before)
    with pytest.raises(RuntimeError, match='capture'):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            with opt.ema_weights():
                pass
    torch.cuda.synchronize()
    assert torch.equal(flat.params, before) and torch.equal(shadow, shadow_before)
    # the next training step, against the twin that never entered the context
    for n_, o_ in ((net, opt), (twin, twin_opt)):
        n_.train()
        _unet_step(n_, o_, image, label)
    torch.cuda.synchronize()
    assert torch.equal(flat.params, twin._flat.params)
    a, b = opt.state_dict()['slabs'][0], twin_opt.state_dict()['slabs'][0]
    for k in ('m', 'v', 'ema'):
        assert torch.equal(a[k], b[k]), k
    assert a['steps'] == b['steps']


def test_state_dict_round_trip_of_the_shadow():
    """The shadow travels with state_dict(); a state without one loads with the shadow set to the current parameters."""
    from pacingpseudo_amd.optim import FusedAdam
    kw = dict(lr=1e-3, weight_decay=3e-4)
    model, opt, _ = _run_steps('FusedAdam', 2, ema_decay=0.9, **kw)
    sd = opt.state_dict()
    # into an optimizer that has not stepped yet (the state waits for the slab) and then steps once, against the original
    torch.manual_seed(3)
    other = build_model(_small_args())
    other.load_state_dict(model.state_dict())
    other_opt = FusedAdam(other.parameters(), **kw)
    other_opt.load_state_dict(sd)
    assert other_opt.param_groups[0]['ema_decay'] == 0.9
    for m_, o_ in ((model, opt), (other, other_opt)):
        iteration(m_, o_, _small_batch(), _small_args(), 0)
    torch.cuda.synchronize()
    a, b = opt.state_dict()['slabs'][0], other_opt.state_dict()['slabs'][0]
    assert torch.equal(model.flat.params, other.flat.params)
    for k in ('m', 'v', 'ema'):
        assert torch.equal(a[k], b[k]), k
    # a state without `ema`, into an optimizer whose slab exists
    old = dict(sd, slabs=[{k: v for k, v in sd['slabs'][0].items() if k != 'ema'}])
    opt.load_state_dict(old)
    assert torch.equal(next(iter(opt._slabs.values()))['ema'], model.flat.params)


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def _trim(run, src_root, dst_root, e, last):
    """tests/test_gpu_resume.py::_trimmed_copy, and the EMA files written after epoch e."""
    from tests.test_gpu_resume import _load, _trimmed_copy
    dst = _trimmed_copy(run, src_root, dst_root, e, last)
    for k in range(e + 1, last + 1):
        p = os.path.join(dst, 'ckps', f'ema_ckp_{k}.pth')
        if os.path.exists(p):
            os.remove(p)
    if _load(os.path.join(run, 'ckps', f'state_{last}.pth'))['best_ema_epoch'] > e:
        os.remove(os.path.join(dst, 'best_ema_ckp.pth'))
    return dst


def _same_tensors(a, b, name):
    assert list(a) == list(b), name
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)


def test_driver_validates_saves_and_resumes_the_average(tmp_path):
    """9: train_chaos.py --ema_decay 0.9 on synthetic data, three epochs, --ckp_interval 1: the files, log lines and scalars;
    stopped after epoch 0 and resumed it ends with ema_ckp_*, best_ema_ckp and valdice_ema bit-identical to the uninterrupted
    run (and everything tests/test_gpu_resume.py compares); inference.py --ema evaluates the run directory."""
    from tests.test_gpu_resume import FULL, SMALL, _assert_equal_tree, _assert_same_run, _driver, _load, _run, _scalars
    argv = SMALL + FULL + ['--epoch', '3', '--cpu_input', '--num_workers', '0', '--ema_decay', '0.9', '--ckp_interval', '1']
    full = _run('train_chaos.py', argv + ['--state_interval', '1'], tmp_path / 'full', 'r')
    log = open(os.path.join(full, 'log.txt')).read()
    sc = _scalars(full)
    names = ['BG', 'Liver', 'R-Kidney', 'L-Kidney', 'Spleen']
    for e in range(3):
        assert os.path.isfile(os.path.join(full, 'ckps', f'ema_ckp_{e}.pth')) and os.path.isfile(os.path.join(full, 'ckps', f'ckp_{e}.pth'))
        assert f'val_ema: {e:03d}, loss_pce:' in log and f'val: {e:03d}, loss_pce:' in log
        for tag in [f'DSC_EMA/{n}' for n in names] + ['DSC_EMA/All', 'DSC_EMA/Best'] + [f'DSC/{n}' for n in names] + ['DSC/All', 'DSC/Best']:
            assert (tag, e) in sc, (tag, e)
    assert 'The best EMA at epoch:' in log
    z = np.load(os.path.join(full, 'valdice.npz'))
    assert sorted(z.files) == ['valdice', 'valdice_ema'] and z['valdice_ema'].shape == (3,)
    assert [sc[('DSC_EMA/All', e)] for e in range(3)] == z['valdice_ema'].tolist()
    last = _load(os.path.join(full, 'ckps', 'state_2.pth'))
    assert last['args']['ema_decay'] == 0.9 and 'ema' in last['optimizer']['slabs'][0] and 'best_ema_avg' in last
    ema_ckp, ckp = _load(os.path.join(full, 'ckps', 'ema_ckp_2.pth')), _load(os.path.join(full, 'ckps', 'ckp_2.pth'))
    assert list(ema_ckp) == list(ckp)                                # the ordinary keys
    assert not torch.equal(ema_ckp['backbone.final_conv.weight'], ckp['backbone.final_conv.weight'])
    if os.path.exists(os.path.join(full, 'best_ema_ckp.pth')):
        assert list(_load(os.path.join(full, 'best_ema_ckp.pth'))) == list(ckp)
    # resumed from state_0, with another --ema_val_interval spelled the same way (1) left alone
    copy = _trim(full, tmp_path / 'full', tmp_path / 'resumed', 0, 2)
    r = _driver('train_chaos.py', argv + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'resumed'),
                                          '--resume', os.path.join(copy, 'ckps', 'state_0.pth')])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    st = _assert_same_run(full, copy, 2)
    resumed = _load(os.path.join(copy, 'ckps', 'state_2.pth'))
    for key in ('best_ema_avg', 'best_ema_epoch', 'best_ema_avg_class', 'valdice_ema'):
        _assert_equal_tree(st[key], resumed[key], key)
    for e in (1, 2):
        _same_tensors(_load(os.path.join(full, 'ckps', f'ema_ckp_{e}.pth')), _load(os.path.join(copy, 'ckps', f'ema_ckp_{e}.pth')), f'ema_ckp_{e}')
    assert os.path.exists(os.path.join(full, 'best_ema_ckp.pth')) == os.path.exists(os.path.join(copy, 'best_ema_ckp.pth'))
    if os.path.exists(os.path.join(full, 'best_ema_ckp.pth')):
        _same_tensors(_load(os.path.join(full, 'best_ema_ckp.pth')), _load(os.path.join(copy, 'best_ema_ckp.pth')), 'best_ema_ckp')
    zc = np.load(os.path.join(copy, 'valdice.npz'))
    assert np.array_equal(z['valdice_ema'], zc['valdice_ema']) and np.array_equal(z['valdice'], zc['valdice'])
    # inference.py --ema on the run directory (the best averaged weights: a three-epoch run has no ema_ckp_399.pth)
    if os.path.exists(os.path.join(full, 'best_ema_ckp.pth')):
        from pacingpseudo_amd import inference as I
        out = tmp_path / 'inf'
        dicearr, _ = I.main(['--fold', '1', '--checkpoint_file', full, '--ema', '--best_ckp', '--dataset', 'chaost1', '--root', str(out),
                             '--synthetic', '4', '--image_size', '64', '--batch_size', '4', '--num_workers', '0'])
        assert dicearr.shape == (4, 5)
        text = open(glob.glob(str(out / 'Inference' / 'chaost1' / '*' / 'log.txt'))[0]).read()
        assert 'best_ema_ckp.pth' in text and 'overall Dice' in text


def test_driver_with_the_flag_off_writes_what_it_wrote(tmp_path):
    """9 (off): the run directory holds the file names, scalar tags and log line kinds it held before the flags existed."""
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'off')
    train_main(['--tag', 'off', '--session', 'Experiment', '--root', root, '--synthetic', '8', '--epoch', '2', '--batch_size', '4',
                '--image_size', '64', '--num_workers', '0', '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path',
                '--do_memory', '--state_interval', '1'])
    run = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-off'))[0]
    files = sorted(os.path.relpath(os.path.join(d, f), run) for d, _, fs in os.walk(run) for f in fs)
    data = [f for f in files if f.endswith(('.pth', '.npz', '.jsonl', '.txt'))]          # (besides a copy of the launching script)
    assert [f for f in data if f != 'best_ckp.pth'] == ['ckps/ckp_1.pth', 'ckps/state_0.pth', 'ckps/state_1.pth', 'log.txt',
                                                        'tb_summary/scalars.jsonl', 'valdice.npz'], files
    assert not any('ema' in f for f in files)
    tags = {json.loads(ln)['tag'] for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))}
    names = ['BG', 'Liver', 'R-Kidney', 'L-Kidney', 'Spleen']
    assert tags == {'losses/loss_pce_train', 'losses/loss_cr', 'losses/loss_ent', 'losses/loss_aux_cls', 'losses/loss_memory',
                    'lr/current_lr', 'losses/loss_pce_val', 'DSC/All', 'DSC/Best'} | {f'DSC/{n}' for n in names}, tags
    log = open(os.path.join(run, 'log.txt')).read()
    assert 'ema_decay=0.0' in log and 'val_ema' not in log and 'EMA' not in log      # (the flag dump names the flags)
    assert np.load(os.path.join(run, 'valdice.npz')).files == ['valdice']
    st = torch.load(os.path.join(run, 'ckps', 'state_1.pth'), map_location='cpu', weights_only=True)
    assert set(st) == {'format', 'version', 'args', 'world_size', 'epoch', 'model', 'optimizer', 'loss_scale', 'guard', 'skipped_logged',
                       'training', 'best_avg', 'best_epoch', 'best_avg_class', 'valdice', 'rng'}
    assert set(st['optimizer']['slabs'][0]) == {'m', 'v', 'steps'}


def test_upper_bound_driver_validates_the_average(tmp_path):
    """9: upper_bound_chaos.py likewise, one short case; --ema_val_interval 2 validates the average after epochs 1 and 2 (the last)."""
    from tests.test_gpu_resume import SMALL, _run, _scalars
    run = _run('upper_bound_chaos.py', SMALL + ['--epoch', '3', '--num_workers', '0', '--ema_decay', '0.9', '--ema_val_interval', '2',
                                                '--init_ch', '8', '--max_ch', '64'],
               tmp_path / 'ub', 'ub', session='Upperbound')
    log = open(os.path.join(run, 'log.txt')).read()
    sc = _scalars(run)
    assert 'val_ema: 000,' not in log and 'val_ema: 001, loss_ce:' in log and 'val_ema: 002, loss_ce:' in log
    assert ('DSC_EMA/All', 0) not in sc and ('DSC_EMA/All', 1) in sc and ('DSC_EMA/Best', 2) in sc and ('DSC/All', 0) in sc
    assert os.path.isfile(os.path.join(run, 'ckps', 'ema_ckp_2.pth')) and os.path.isfile(os.path.join(run, 'ckps', 'ckp_2.pth'))
    z = np.load(os.path.join(run, 'valdice.npz'))
    assert sorted(z.files) == ['valdice', 'valdice_ema'] and z['valdice_ema'][0] == 0.0
    assert z['valdice_ema'][1] == sc[('DSC_EMA/All', 1)] and z['valdice_ema'][2] == sc[('DSC_EMA/All', 2)]


def _rank_run(dist_on, port, out_path):
    """Three FusedAdam steps with the average on and one evaluation inside ema_weights(); dist_on: inside a ONE-rank RCCL group."""
    from pacingpseudo_amd.optim import FusedAdam
    if dist_on:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', PP_FORCE_DIST='1')
        import torch.distributed as dist
        from pacingpseudo_amd import parallel
        parallel.init_from_env('nccl')
    args = _small_args()
    torch.manual_seed(3)
    model = build_model(args)
    if dist_on:
        parallel.attach(model)
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=3e-4, ema_decay=0.9)
    batch = _small_batch()
    for _ in range(3):
        iteration(model, opt, batch, args, 0)
    model.eval()
    with opt.ema_weights(), torch.no_grad():
        logits = model.backbone(batch['image'].cuda())['segmentation/logits'].cpu()
    torch.cuda.synchronize()
    sd = opt.state_dict()['slabs'][0]
    torch.save(dict(params=model.flat.params.cpu(), m=sd['m'], v=sd['v'], ema=sd['ema'], logits=logits,
                    attached=model.engine.comm is not None), out_path)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


def test_average_inside_a_one_rank_rccl_group(tmp_path):
    """10: the run inside a one-rank RCCL group equals the single-process run bit for bit, the logits of the averaged weights
    included."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    res = {}
    for tag, dist_on in (('single', False), ('rccl', True)):
        out = str(tmp_path / f'{tag}.pt')
        p = mp.get_context('spawn').Process(target=_rank_run, args=(dist_on, port, out))
        p.start()
        p.join(240)
        if p.is_alive():
            p.kill()
            p.join()
        assert p.exitcode == 0, f'{tag}: exit code {p.exitcode}'
        res[tag] = torch.load(out)
    a, b = res['single'], res['rccl']
    assert b['attached'] and not a['attached']
    for k in ('params', 'm', 'v', 'ema', 'logits'):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['ema'], a['params'])
