"""Is every launch of a training step ordered against every launch it conflicts with?  (tests/_stream_hazards.py)

A step runs on two HIP streams (pacingpseudo_amd/engine.py): weight gradients and the auxiliary path's forward / head of its backward
on the second one, tied to the main stream by dz_ready / wg_done, aux_fork / aux_join, bucket_ev and the join before the optimizer.
tests/test_gpu_round4.py compares the OUTCOME with the single-stream order, which a missing wait passes whenever the scheduler is
kind.  Here the ordering itself is checked, in two ways:

  * ten configurations are recorded -- three iterations each of forward, backward and FusedAdam.step with clipping and EMA on, at
    128 px, batch 2, full width -- and the happens-before checker must find no unordered conflicting pair in any of them; then,
    for each kind of wait in turn, its waits are deleted FROM THE LOG and the checker must report a hazard (the checker can see
    what each wait is for);
  * the step of test_second_stream_weight_gradients_are_bit_identical runs with each stream in turn held back by a spin kernel in
    front of every launch, so that a latent race must show, and stays bit-identical to the single-stream run.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _stream_hazards as H  # noqa: E402
from tests._launch_census import BATCH_IMAGE_SIZE  # noqa: E402
from tests.test_gpu_step import build_model, iteration  # noqa: E402

EPOCH = 37              # (ramp-up weights well above zero: every loss contributes)
STEPS = 3               # buffers and events are reused across steps
_CRF_NC = dict(do_loss_crf=True, crf_radius=5, crf_dilation=1, crf_sigma_xy=6.0, crf_sigma_rgb=0.1,
               do_loss_nc=True, nc_radius=5, nc_dilation=1, nc_sigma_xy=6.0, nc_sigma_rgb=0.1)
CONFIGS = {
    'fp32/train-BN': dict(),
    'fp32/eval-BN': dict(bn_eval=True),
    'fp16': dict(storage='fp16'),
    'bf16': dict(storage='bf16'),
    'strided': dict(strided=True),
    'groupnorm': dict(gn=True),
    'aux_dropout': dict(over=dict(aux_drop_prob=0.5)),
    'crf+nc': dict(over=_CRF_NC),
    'sync_bn+buckets': dict(sync_bn=True),
    'graph': dict(graph=True),
}
# which kinds of wait (tests/_stream_hazards.EVENT_KINDS) a configuration issues
KINDS = {name: {'dz_ready', 'wg_done', 'join', 'aux_fork', 'aux_join'} for name in CONFIGS}
KINDS['sync_bn+buckets'] = {'dz_ready', 'wg_done', 'join', 'aux_fork', 'aux_join', 'bucket_ev'}
# Waits whose deletion leaves the LOG free of hazards, by (configuration, kind): what they protect is not in the log, or another
# wait protects it as well.  DESIGN.md (the stream-ordering paragraph) names them; a wait that starts to protect a library launch
# must leave this table (test_a_deleted_wait_is_reported fails on a stale entry).  All three are in the sync_bn + bucket recording:
#   bucket_ev: orders the bucket hook's work on the second stream (the all-reduce; here ProbeReducer's torch kernels) behind the
#     main stream's BatchNorm / bias gradients of that bucket.  The second stream's own launches behind it wait for a later
#     dz_ready anyway.
#   join: with a reducer attached, its reduce() makes the main stream wait for the events it recorded on the second stream behind
#     the last bucket, which is behind the last weight gradient -- the join repeats that.
#   aux_join: with synchronised BatchNorm the auxiliary forward runs in line, so the only aux_join waits left are the backward's,
#     and those are implied by the wg_done waits at slot reuse that the decoder's backward issues first (the second stream runs
#     in order: the event behind a weight gradient is behind the auxiliary head too).  In the other nine recordings the forward's
#     aux_join waits protect the pair sums and the memory bank.
PROTECTS_NOTHING_IN_THE_LOG = {('sync_bn+buckets', 'bucket_ev'), ('sync_bn+buckets', 'join'), ('sync_bn+buckets', 'aux_join')}


def _loss_fn(args):
    from pacingpseudo_amd.losses.losses import weighted_loss_sum
    w = dict(O.loss_weights(args, EPOCH), loss_crf=0.3, loss_nc=0.3)

    def f(out, epoch):
        keys = [k for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory', 'loss_crf', 'loss_nc') if k in out]
        return weighted_loss_sum([out[k] for k in keys], [w[k] for k in keys])      # pp_weighted_sum_fwd, as train.py assembles it
    return f


def _record(name):
    from pacingpseudo_amd.optim import FusedAdam
    cfg = CONFIGS[name]
    args = O.full_flags(**cfg.get('over', {}))
    args.storage = cfg.get('storage', 'fp32')
    if cfg.get('strided'):
        args.is_stride_conv = args.is_trans_conv = True
    size = BATCH_IMAGE_SIZE
    batch = {k: v.cuda() for k, v in O.synthetic_batch(2, size, size, num_classes=args.num_classes, seed=7, keep=0.05).items() if k != 'label'}
    f = _loss_fn(args)
    with pytest.MonkeyPatch.context() as mp, H.Recording(mp) as rec:
        torch.manual_seed(1)
        if cfg.get('gn'):
            from tests.test_gpu_groupnorm import build_gn_model
            model = build_gn_model(args)
        else:
            model = build_model(args)
        model.train(not cfg.get('bn_eval'))
        opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd, max_grad_norm=1.0, ema_decay=0.99)
        probe = None
        if cfg.get('sync_bn'):      # the split train-mode BatchNorm of --sync_bn and a reducer's bucket hook, on one rank
            from tests._bucket_probe import NoopComm, ProbeReducer
            model.engine.comm = NoopComm()
            model.engine.sync_bn = True
            probe = model._reducer = ProbeReducer(model, fenced=False)
        graphed = None
        if cfg.get('graph'):
            from pacingpseudo_amd.graph import GraphedStep
            graphed = GraphedStep(model, opt, f, warmup=STEPS - 1)      # the last step is captured, then replayed
        torch.cuda.synchronize()
        for _ in range(STEPS):
            if graphed is not None:
                graphed(batch, EPOCH)
                continue
            out = model(batch, mode='train', step=EPOCH)
            loss = f(out, EPOCH)
            opt.zero_grad()
            if probe is not None:
                probe.log, probe.snap, probe.main = [], {}, torch.cuda.current_stream()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        if graphed is not None:
            assert (graphed.captures, graphed.replays) == (1, 1)
        eng = model.engine
        rec.name_events(eng.last_plan)
        meta = dict(side=eng._wg_stream.cuda_stream, main=torch.cuda.current_stream().cuda_stream)
    del model, opt
    torch.cuda.empty_cache()
    return rec.log, dict(rec.event_names), meta


@functools.lru_cache(maxsize=None)
def recording(name):
    """(log, {event: name}, dict(side=, main= stream handles)) of one configuration, recorded once per process."""
    return _record(name)


@pytest.fixture(scope='module', autouse=True)
def _drop_the_recordings():
    yield
    recording.cache_clear()


def _launches(log, stream=None, prefix=''):
    return [it for it in log if it[0] == 'L' and it[1].startswith(prefix) and (stream is None or it[3] == stream)]


@pytest.mark.parametrize('name', list(CONFIGS))
def test_no_launch_of_a_step_races_another(name):
    """Three recorded iterations: no pair of launches on different streams with overlapping extents, a write among them, and no
    happens-before path.  Every configuration on its own (addresses are reused between models).  A recorded launch without a row
    in the access table fails here by name (MissingRow): nothing is excluded."""
    log, names, meta = recording(name)
    found, total = H.check(log)
    assert total == 0, f'{name}: ' + H.report(found, total)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_log_is_what_it_claims_to_be(name):
    """A clean verdict on an empty or one-stream log would prove nothing: the recording holds the second-stream launches of the
    weight-gradient family and of the auxiliary path, the optimizer's launches and the loss assembly, what the configuration is
    named after, and the waits and records of each kind of event the configuration uses."""
    log, names, meta = recording(name)
    side = meta['side']
    streams = {it[3] for it in log if it[0] == 'L'}
    assert side in streams and len(streams) >= 2 and side != meta['main']
    n_wg = len(_launches(log, side, 'pp_conv3x3_bwd_weight')) + len(_launches(log, side, 'pp_conv3x3_wino_bwd_weight'))
    assert n_wg >= STEPS * 20, f'{n_wg} weight-gradient launches on the second stream'
    assert not [it for it in _launches(log, None, 'pp_conv3x3_') if 'bwd_weight' in it[1] and it[3] != side]
    # the auxiliary path: the head of its backward on the second stream always, its forward too unless BatchNorm is synchronised
    assert len(_launches(log, side, 'pp_aux_pce_bwd')) == STEPS
    assert len(_launches(log, side, 'pp_aux_pce_fwd')) == (0 if CONFIGS[name].get('sync_bn') else STEPS)
    assert len(_launches(log, None, 'pp_aux_pce_fwd')) == STEPS
    # the optimizer (clipping and EMA on) and the loss assembly
    for entry in ('pp_adam_step_ema', 'pp_grad_sumsq', 'pp_grad_clip_finalize', 'pp_weighted_sum_fwd', 'pp_weighted_sum_bwd'):
        assert len(_launches(log, None, entry)) >= STEPS, entry
        assert not [it for it in _launches(log, side, entry)], entry
    if CONFIGS[name].get('storage'):
        assert len(_launches(log, None, 'pp_scale_guard')) >= STEPS       # the scale-guard launches of 16-bit storage
        suffix = {'fp16': '_h16', 'bf16': '_bf16'}[CONFIGS[name]['storage']]
        assert _launches(log, side, 'pp_conv3x3_bwd_weight_f16x3' + suffix)
    if CONFIGS[name].get('strided'):
        assert _launches(log, None, 'pp_stride2_scatter') and _launches(log, None, 'pp_convtranspose_bwd_weight')
    if CONFIGS[name].get('gn'):
        assert _launches(log, None, 'pp_gn_lrelu_bwd')
    if name == 'crf+nc':
        assert _launches(log, None, 'pp_crf_loss_bwd') and _launches(log, None, 'pp_nc_loss_bwd')
    if name == 'aux_dropout':
        assert len(_launches(log, side, 'pp_channel_scale')) >= 3 * STEPS
    if CONFIGS[name].get('sync_bn'):
        assert _launches(log, None, 'pp_bn_lrelu_bwd_apply')
    kinds = {H.wait_kind(it, names) for it in log} - {None}
    assert kinds == KINDS[name], kinds ^ KINDS[name]
    recorded = {names.get(it[1]) for it in log if it[0] == 'R'}
    assert {'dz_ready', 'wg_done', 'aux_fork', 'aux_join'} <= recorded and ('bucket_ev' in recorded) == ('bucket_ev' in KINDS[name])


def test_each_of_the_six_event_kinds_occurs():
    assert set().union(*KINDS.values()) == set(H.EVENT_KINDS)
    assert {(c, k) for c, k in PROTECTS_NOTHING_IN_THE_LOG} <= {(c, k) for c, ks in KINDS.items() for k in ks}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_a_deleted_wait_is_reported(name):
    """Planted mistakes, made on the log and never on the device: for each kind of wait in turn its waits are deleted from the
    recorded log; the checker must then report at least one hazard -- or the pair is listed, with its reason, in
    PROTECTS_NOTHING_IN_THE_LOG, and then it must report none (a stale entry fails too)."""
    log, names, meta = recording(name)
    for kind in sorted(KINDS[name]):
        cut = H.without_waits(log, names, kind)
        assert len(cut) < len(log), kind
        found, total = H.check(cut, limit=5)
        print(f'{name}: without the {len(log) - len(cut)} {kind} waits: ' + H.report(found, total))
        if (name, kind) in PROTECTS_NOTHING_IN_THE_LOG:
            assert total == 0, f'{name}: the {kind} waits protect a library launch after all: ' + H.report(found, total)
        else:
            assert total >= 1, f'{name}: the log without its {kind} waits shows no hazard'


# ------------------------------------------------------------------------------------------------------------ held-back streams
# Spin cycles (torch.cuda._sleep) in front of every launch of the stream that is held back.  Not a tolerance: it only has to make
# that stream lag, which each run shows with two timed events.  Observed on the MI355X at 10^6 cycles: second stream held back
# (93 delayed launches in three steps): its last launch finished 0.81 ms after the main stream reached the join; main stream held
# back (150 delayed launches): its last launch of the backward pass finished 1.74 ms after the second stream reached its last wait.
SLEEP_CYCLES = 1_000_000


def _held_back_run(which, args, batch):
    """Three steps of tests/test_gpu_step.iteration; which: None (one stream), 'side' (every second-stream launch delayed) or
    'main' (every main-stream launch of the backward pass delayed).  Returns (outputs, gradients, state dict, lag in ms)."""
    from pacingpseudo_amd import engine as E
    from pacingpseudo_amd.optim import FusedAdam
    state = dict(backward=False, eng=None, sleeps=0)
    reached, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    main = torch.cuda.current_stream()

    def before_launch(entry, stream):
        if which == 'side' and stream != main.cuda_stream:
            with torch.cuda.stream(state['eng']._wg_stream):
                torch.cuda._sleep(SLEEP_CYCLES)
            state['sleeps'] += 1
        elif which == 'main' and state['backward'] and stream == main.cuda_stream:
            torch.cuda._sleep(SLEEP_CYCLES)
            state['sleeps'] += 1

    with pytest.MonkeyPatch.context() as mp, H.Recording(mp, before_launch=before_launch if which else None):
        mp.setattr(E, 'WGRAD_STREAM', which is not None)
        mp.setattr(E, 'WGRAD_CUS_FULL', E.WGRAD_CUS_SIDE)          # the same CU budget on both sides: the same partition of the sums
        real_bwd, real_join, real_wait = E.StepEngine.backward_step, E.StepEngine._join_side_stream, torch.cuda.Stream.wait_event

        def backward_step(self, *a, **k):
            state['backward'] = True
            try:
                return real_bwd(self, *a, **k)
            finally:
                state['backward'] = False

        def join(self, plan):
            # the join before the optimizer.  'side': the main stream has reached it (reached), the second stream's last launch is
            # behind `done`.  'main': the main stream's last launch of the backward pass is behind `done`.
            if which == 'side':
                reached.record(main)
                done.record(self._wg_stream)
            elif which == 'main':
                done.record(main)
            return real_join(self, plan)

        def wait_event(stream, event):
            # 'main': the second stream reaches a wait for the main stream (the last one of the backward pass stands)
            if which == 'main' and state['backward'] and stream is state['eng']._wg_stream:
                reached.record(stream)
            return real_wait(stream, event)
        mp.setattr(E.StepEngine, 'backward_step', backward_step)
        mp.setattr(E.StepEngine, '_join_side_stream', join)
        mp.setattr(torch.cuda.Stream, 'wait_event', wait_event)
        torch.manual_seed(1)
        model = build_model(args)
        state['eng'] = model.engine
        opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
        for _ in range(STEPS):
            rec, grads = iteration(model, opt, batch, args, 0)
        torch.cuda.synchronize()
        assert (model.engine._wg_stream is not None) == (which is not None)
        lag = reached.elapsed_time(done) if which else 0.0
    return rec, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}, lag, state['sleeps']


def test_a_held_back_stream_changes_nothing():
    """Each stream in turn lags far behind the other; gradients and state stay bit-identical to the single-stream run, and the
    lag is shown: the held-back stream's last launch completed `lag` ms after the other stream reached the join (the second
    stream's last wait for the main stream, when the main stream is the one held back).  A run that did not lag fails as vacuous.
    Observed on the MI355X: the figures next to SLEEP_CYCLES."""
    args = O.full_flags()
    batch = O.synthetic_batch(2, 128, 128, seed=3, keep=0.05)
    one = _held_back_run(None, args, batch)
    for which in ('side', 'main'):
        rec, grads, sd, lag, sleeps = _held_back_run(which, args, batch)
        print(f'held back: {which} stream, {sleeps} delayed launches, lag at the join {lag:.2f} ms')
        assert sleeps >= STEPS * 20
        assert lag > 0.0, f'the {which} stream did not lag ({lag:.3f} ms): the run shows nothing'
        for k, v in one[1].items():
            if v is not None:
                assert torch.equal(grads[k], v), f'{which} stream held back: gradient {k}'
        for k, v in one[2].items():
            assert torch.equal(sd[k], v), f'{which} stream held back: {k}'
        for k, v in one[0].items():
            assert torch.equal(rec[k], v), f'{which} stream held back: output {k}'
