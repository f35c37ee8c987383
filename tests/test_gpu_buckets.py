"""Are the gradient buckets complete when the engine announces them?  (StepEngine._bucket, parallel.GradReducer.)

With RCCL a bucket's all-reduce is issued, asynchronously and in place, the moment `_bucket(tag)` fires -- since round 6 from the
second (weight-gradient) stream behind one reused event of the main stream.  A gradient of that bucket enqueued AFTER the
announcement, on either stream, would be summed stale on every rank, silently; so would a bucket announced twice or never.  One rank
cannot see that (its sum is the identity) and the gloo tests reduce after the backward pass.  Here two identical ranks are emulated
on ONE GPU: tests/_bucket_probe.ProbeReducer doubles the bucket in place where the all-reduce would be issued, and the final slab
must be, bit for bit, twice the slab of the same step without a reducer.  Every comparison is torch.equal.

Two models per case, built from the same seed (the memory bank and the BatchNorm buffers move in the forward pass, so one model
cannot run the step twice); the reference slab of a configuration is computed once and shared (the positive controls reuse the
small plan's).  'full' = the Experiment flags at the real widths, 128x128 (kernel selection and what runs on the second stream
depend on the widths); 'small' = init_ch 8 / max_ch 64 at 64x64, the smallest plan that still has six buckets and both streams.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _bucket_probe as P  # noqa: E402
from tests.test_gpu_groupnorm import build_gn_model  # noqa: E402
from tests.test_gpu_step import build_model  # noqa: E402

EPOCH = 37              # (ramp-up weights well above zero: every loss contributes)
SMALL = dict(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
_REF = {}               # configuration key -> (reference gradient slab, loss scale); computed once, never written again


@pytest.fixture(scope='module', autouse=True)
def _drop_the_references():
    yield
    _REF.clear()


def _small(**over):
    return O.full_flags(**SMALL, **over)


def _batch(args, size, seed=3):
    b = O.synthetic_batch(2, size, size, num_classes=args.num_classes, seed=seed, keep=0.05)
    return {k: v.cuda() for k, v in b.items() if k != 'label'}


def _model(args, builder, bn_train, prepare=None):
    torch.manual_seed(1)
    model = builder(args)
    g = torch.Generator().manual_seed(7)
    for k, v in model.state_dict().items():               # non-trivial running statistics (eval mode) and a visited memory bank
        if k.endswith('running_mean'):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith('running_var'):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith('memory_bank'):
            v.copy_(torch.randn(v.shape, generator=g))
    model.train(bn_train)
    if prepare is not None:
        prepare(model)
    return model


def _backward(model, batch, f, probe=None, opt=None):
    torch.manual_seed(11)                                  # the auxiliary Dropout2d masks come from torch's CUDA generator
    out = model(batch, mode='train', step=EPOCH)
    loss = f(out, EPOCH)
    if opt is not None:
        opt.zero_grad()
    if probe is not None:
        probe.log, probe.snap = [], {}
        probe.main = torch.cuda.current_stream()
    loss.backward()
    torch.cuda.synchronize()


def _reference(key, args, builder, bn_train, size, prepare):
    if key not in _REF:
        model = _model(args, builder, bn_train, prepare)
        assert model._reducer is None
        _backward(model, _batch(args, size), P.loss_fn(args))
        _REF[key] = (model.flat.grads.clone(), model.engine.last_plan.loss_scale)
    return _REF[key]


def _two_streams(model):
    return model.engine._side_stream(model.engine.last_plan) is not None


def _case(key, args, *, builder=build_model, bn_train=True, size=64, fenced=True, two_stream=True, prepare=None, wrap=None,
          expect=frozenset()):
    """One training step with the probe against the same step without a reducer.  key: names the reference configuration (everything
    but `fenced`, `wrap` and `expect`, which do not change the reference)."""
    ref, scale = _reference(key, args, builder, bn_train, size, prepare)
    model = _model(args, builder, bn_train, prepare)
    probe = model._reducer = P.ProbeReducer(model, fenced=fenced)
    if wrap is not None:
        wrap(model)
    _backward(model, _batch(args, size), P.loss_fn(args), probe)
    assert model.engine.world == 1 and _two_streams(model) == two_stream
    assert model.engine.last_plan.loss_scale == scale and (scale != 1.0) == (getattr(args, 'storage', 'fp32') != 'fp32')
    return P.check_buckets(probe, model, model.flat, ref, two_stream, bool(args.do_aux_path), loss_scale=scale, expect=expect)


# ------------------------------------------------------------------------------------------------------------ 1. full widths
@pytest.mark.parametrize('storage,bn,fenced', [(s, b, True) for s in ('fp32', 'fp16', 'bf16') for b in ('train', 'eval')]
                         + [('fp32', 'train', False), ('fp32', 'eval', False)],
                         ids=lambda v: {True: 'fenced', False: 'unfenced'}.get(v, v))
def test_full_width_step(storage, bn, fenced):
    """Experiment flags, real widths, 128x128, train- and eval-mode BatchNorm, the three storage modes (16-bit: the slab is compared
    after unscale_grads; the loss scale is a power of two, so the factor 2 survives exactly).  The fp32 pair runs a second time
    without the fence: the shipped schedule, where the main stream runs on beside the all-reduce."""
    args = O.full_flags()
    args.storage = storage
    _case(f'full-{storage}-{bn}', args, bn_train=bn == 'train', size=128, fenced=fenced)


# ------------------------------------------------------------------------------------------------------------ 2./3. variants
def _variants():
    crf = dict(do_loss_crf=True, crf_radius=5, crf_dilation=1, crf_sigma_xy=6.0, crf_sigma_rgb=0.1)
    return {
        'default': (_small(), build_model),
        'control': (O.default_args(**SMALL), build_model),                                   # no auxiliary path: five buckets
        'groupnorm': (_small(), build_gn_model),
        'strided_transposed': (_small(is_stride_conv=True, is_trans_conv=True), build_model),
        'stride16': (_small(output_stride=16), build_model),
        'stride32': (_small(output_stride=32, do_aux_path=False, do_memory=False), build_model),
        'classes17': (_small(num_classes=17, ignored_index=17), build_model),
        'crf': (_small(**crf), build_model),
        'aux_dropout': (_small(aux_drop_prob=0.5), build_model),
    }


@pytest.mark.parametrize('variant', ['default', 'control', 'groupnorm', 'strided_transposed', 'stride16', 'stride32', 'classes17', 'crf',
                                     'aux_dropout'])
def test_small_variants_train_mode(variant):
    """One case per variant that changes WHICH launches write gradients (train-mode BatchNorm)."""
    args, builder = _variants()[variant]
    _case(f'small-{variant}-train', args, builder=builder)


@pytest.mark.parametrize('variant', ['default', 'groupnorm'])
def test_small_variants_eval_mode(variant):
    args, builder = _variants()[variant]
    _case(f'small-{variant}-eval', args, builder=builder, bn_train=False)


# ------------------------------------------------------------------------------------------------------------ 4. one stream
@pytest.mark.parametrize('bn', ['train', 'eval'])
def test_one_stream_branch(monkeypatch, bn):
    """PP_WGRAD_STREAM=0, the other branch of `_bucket`: no second stream, the hook is called on the main stream -- every
    announcement must run there."""
    import pacingpseudo_amd.engine as E
    monkeypatch.setattr(E, 'WGRAD_STREAM', False)          # before the models (their plans) are built
    _case(f'small-onestream-{bn}', _small(), bn_train=bn == 'train', two_stream=False)


# ------------------------------------------------------------------------------------------------------------ 5. SyncBN split
def test_synchronised_batchnorm_backward():
    """The split train-mode BatchNorm backward of --sync_bn (pp_bn_lrelu_bwd_sums, the all-reduce of the sums, pp_bn_lrelu_bwd_apply)
    without a process group: engine.comm is tests/_bucket_probe.NoopComm and engine.sync_bn True, on both models.  Beyond `world`,
    `rank` and a no-op `allreduce_sums` the engine asks the stub for `broadcast_bank` (the memory bank after rank 0's update)."""
    def prepare(model):
        model.engine.comm = P.NoopComm()
        model.engine.sync_bn = True
    _case('small-syncbn-train', _small(), prepare=prepare)


# ------------------------------------------------------------------------------------------------------------ 6. graph replay
def test_graph_replay():
    """GraphedStep with the probe installed: the doubling, its events and the fence are captured with the step.  One eager call, one
    capture, two replays, on two alternating batches; after every call each bucket must be twice its snapshot (from the capture
    on the snapshots are the graph's static tensors), and at the end parameters, Adam state and step counts must equal those of
    an eager loop with the probe on the same batches."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = O.full_flags()
    base = P.loss_fn(args)
    batches = [_batch(args, 128, seed=s) for s in (3, 4)]
    runs = {}
    for mode in ('eager', 'graph'):
        model = _model(args, build_model, True)
        probe = model._reducer = P.ProbeReducer(model, fenced=True)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)

        def f(out, epoch, probe=probe):
            probe.main = torch.cuda.current_stream()       # inside a capture this is the capturing stream
            return base(out, epoch)
        gs = GraphedStep(model, opt, f, warmup=1)
        snaps = None
        for i in range(3):
            b = batches[i % 2]
            probe.log = []
            if mode == 'graph':
                gs(b, 0)
            else:
                gs._eager(b, 0)
            torch.cuda.synchronize()
            if mode == 'graph' and i == 1:
                snaps = dict(probe.snap)                    # the capture's static tensors
            if mode == 'eager' or i < 2:
                assert [t for t, _ in probe.log] == P.expected_tags(model, True) and not any(m for _, m in probe.log), probe.log
            else:
                assert probe.log == [] and all(probe.snap[t] is snaps[t] for t in snaps)      # a replay runs no host code
            assert set(probe.snap) == set(P.expected_tags(model, True))
            assert P.snapshot_failures(probe, model.flat) == set(), (mode, i)
        if mode == 'graph':
            assert gs.captures == 1 and gs.replays == 2, (gs.captures, gs.replays)
        sd = opt.state_dict()['slabs'][0]
        runs[mode] = dict(params=model.flat.params.clone(), grads=model.flat.grads.clone(), m=sd['m'], v=sd['v'], steps=sd['steps'])
    e, g = runs['eager'], runs['graph']
    assert bool(torch.isfinite(e['params']).all()) and bool((e['grads'] != 0).any())
    assert torch.equal(e['grads'], g['grads'])
    assert torch.equal(e['params'], g['params'])
    assert torch.equal(e['m'], g['m']) and torch.equal(e['v'], g['v'])
    assert e['steps'] == g['steps'] == {'backbone': 3, 'aux_path': 3}


# ------------------------------------------------------------------------------------------------------------ 7. clipping
def test_gradient_clipping_reads_the_reduced_slab():
    """max_grad_norm: the clip's sum of squares is the first reader of the slab after `reduce`.  One step with the probe against one
    step whose gradients were doubled by hand before opt.step(): norm, coefficient, parameters and Adam state must be equal."""
    from pacingpseudo_amd.optim import FusedAdam
    args = _small()
    f = P.loss_fn(args)
    batch = _batch(args, 64)
    runs = {}
    for mode in ('by_hand', 'probe'):
        model = _model(args, build_model, True)
        probe = None
        if mode == 'probe':
            probe = model._reducer = P.ProbeReducer(model, fenced=True)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd, max_grad_norm=1e-3)
        _backward(model, batch, f, probe, opt)
        if mode == 'by_hand':
            model.flat.grads.mul_(2)
        opt.step()
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[mode] = dict(params=model.flat.params.clone(), grads=model.flat.grads.clone(), m=sd['m'], v=sd['v'],
                          norm=opt.last_grad_norm.clone(), coef=opt.last_clip_coef.clone())
    h, p = runs['by_hand'], runs['probe']
    assert float(h['norm']) > 0 and 0 < float(h['coef']) < 1            # the clip was active
    assert torch.equal(h['grads'], p['grads'])
    assert torch.equal(h['norm'], p['norm']) and torch.equal(h['coef'], p['coef'])
    assert torch.equal(h['params'], p['params'])
    assert torch.equal(h['m'], p['m']) and torch.equal(h['v'], p['v'])


# ------------------------------------------------------------------------------------------------------------ positive controls
def _rewire(monkeypatch, table):
    """table: {tag announced by the engine: [tags announced in its place]} (host-side announcements only; no kernel sees it)."""
    def wrap(model):
        real = model.engine._bucket

        def _bucket(tag):
            for t in table.get(tag, [tag]):
                real(t)
        monkeypatch.setattr(model.engine, '_bucket', _bucket)
    return wrap


CONTROLS = {
    # dec5 holds main-stream gradients (BatchNorm weight / bias, conv bias) and second-stream weight gradients
    'dec5_early': ({'decoder_upper': ['decoder_upper', 'dec5'], 'dec5': []}, {'dec5'}),
    # enc_rest holds the folded first-layer weight gradient
    'enc_rest_early': ({'enc5': ['enc5', 'enc_rest'], 'enc_rest': []}, {'enc_rest'}),
    'enc6_twice': ({'enc6': ['enc6', 'enc6']}, {'enc6'}),
    'aux_never': ({'aux': []}, {'aux'}),
}


@pytest.mark.parametrize('name', list(CONTROLS))
def test_the_probe_catches_a_planted_mistake(monkeypatch, name):
    """The check must name exactly the bucket whose announcement was moved, doubled or dropped -- and no other."""
    table, caught = CONTROLS[name]
    got = _case('small-default-train', _small(), wrap=_rewire(monkeypatch, table), expect=frozenset(caught))
    assert got == caught
