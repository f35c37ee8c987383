"""Device-side gradient-norm clipping (FusedAdam / FusedSGD ``max_grad_norm``, ``--clip_grad_norm``) on the MI355X:
``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)`` semantics with the norm and the coefficient as device scalars.

Bounds.  The sum of squares is formed in double from the first add, so the only fp32 roundings of ``total`` are its final
conversion (and, for ``coef``, one more): |total - ref| <= 4 * 2^-24 * ref against numpy's float64 norm is a derived bound,
not a measured one.  The update is compared BIT FOR BIT with the unclipped kernel run on gradients scaled by the reported
coefficient; against torch it keeps the tolerances of the unclipped comparisons (test_gpu_round2.py:115, test_gpu_step.py:254).
"""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests.test_gpu_step import build_model, iteration  # noqa: E402

REL = 4 * 2.0 ** -24


def _small_args():
    return O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])


def _small_batch():
    return O.synthetic_batch(2, 64, 64, seed=4, keep=0.05)


def _norm(g, segs, max_norm, skip=None, stats=None):
    """The library's norm pass over the aligned segments `segs` of the device slab g: ([total, coef] on the host, stats tensor)."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    rows = [int(lib.pp_grad_sumsq_rows(b - a)) for a, b in segs]
    partial = torch.full((sum(rows),), float('nan'), device=g.device, dtype=torch.float64)      # every row must be written
    out2 = torch.full((2,), float('nan'), device=g.device)
    stats = torch.zeros(4, device=g.device, dtype=torch.float64) if stats is None else stats
    off = 0
    for (a, b), r in zip(segs, rows):
        lib.pp_grad_sumsq(g.data_ptr() + 4 * a, b - a, partial.data_ptr() + 8 * off, stream_ptr())
        off += r
    lib.pp_grad_clip_finalize(partial.data_ptr(), off, float(max_norm), None if skip is None else skip.data_ptr(), out2.data_ptr(),
                              stats.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return out2.cpu(), stats


def _split(n, k):
    """Up to k non-empty segments of [0, n) that start on 16-byte boundaries (fewer when n is too small to have them)."""
    cuts = sorted({0, n} | {(n * j // k) // 4 * 4 for j in range(1, k)})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _slab(n, seed):
    rng = np.random.RandomState(seed)
    v = (10.0 ** rng.uniform(-8, 3, size=n)) * rng.choice([-1.0, 1.0], size=n)      # magnitudes 1e-8 .. 1e+3
    return torch.from_numpy(v.astype(np.float32)).cuda()


def _bench_numel():
    args = O.full_flags()
    torch.manual_seed(1)
    return build_model(args).flat.numel


def test_norm_kernel_against_float64():
    """G1."""
    sizes = [1, 3, 4, 1021, 2 ** 20 + 5, _bench_numel()]
    for i, n in enumerate(sizes):
        g = _slab(n, seed=10 + i)
        ref = float(np.linalg.norm(g.cpu().numpy().astype(np.float64)))
        for k in (1, 2, 3):
            segs = _split(n, k)
            assert segs[0][0] == 0 and segs[-1][1] == n and all(a % 4 == 0 for a, _ in segs)
            max_norm = 0.37 * ref
            out, stats = _norm(g, segs, max_norm)
            total, coef = float(out[0]), float(out[1])
            want = min(1.0, max_norm / (ref + 1e-6))
            print(f'n={n} segments={len(segs)}: total {total!r} ref {ref!r} rel {abs(total - ref) / ref:.2e}; coef {coef!r} want {want!r}')
            assert abs(total - ref) <= REL * ref, (n, k, total, ref)
            assert abs(coef - want) <= REL * want, (n, k, coef, want)
            assert stats.tolist()[:2] == [1.0, 1.0] and stats[2].item() == stats[3].item() and abs(stats[3].item() - ref) <= REL * ref
            again, _ = _norm(g, segs, max_norm)
            assert torch.equal(out, again), (n, k)                  # bit-reproducible: no atomics, a fixed summation tree


def test_norm_edge_cases():
    """G2: +inf and a max_norm above the norm give coef == 1.0 exactly; all-zero gradients give total == 0, coef == 1."""
    g = _slab(1021, seed=3)
    ref = float(np.linalg.norm(g.cpu().numpy().astype(np.float64)))
    for max_norm in (math.inf, 1.5 * ref, 1e30):
        out, stats = _norm(g, [(0, 1021)], max_norm)
        assert float(out[1]) == 1.0 and abs(float(out[0]) - ref) <= REL * ref
        assert stats.tolist()[:2] == [1.0, 0.0]                      # seen, not clipped
    out, stats = _norm(torch.zeros(1021, device='cuda'), [(0, 512), (512, 1021)], 1.0)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and stats.tolist() == [1.0, 0.0, 0.0, 0.0]
    # a step the overflow guard is going to skip leaves the statistics alone
    skip = torch.tensor([1, 0], device='cuda', dtype=torch.int32)
    seen = torch.tensor([5.0, 2.0, 7.5, 3.0], device='cuda', dtype=torch.float64)
    _norm(g, [(0, 1021)], 0.1, skip=skip, stats=seen)
    assert seen.tolist() == [5.0, 2.0, 7.5, 3.0]


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_clipped_update_equals_the_unclipped_kernel_on_scaled_gradients(kind):
    """G3: three steps, bit for bit.  Reference = the existing pp_adam_step_dev / pp_sgd_momentum_step_dev on g.mul(coef)."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    n = 2 ** 18 + 3                                                 # a tail of three elements
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen).cuda()
    keys = ('p', 'm', 'v') if kind == 'adam' else ('p', 'm')
    runs = {tag: dict({k: torch.zeros(n, device='cuda') for k in keys}, steps=torch.zeros(1, device='cuda', dtype=torch.int32))
            for tag in ('clip', 'ref')}
    for r in runs.values():
        r['p'].copy_(p0)
    lr_dev = torch.full((1,), 3e-3, device='cuda')
    stats = torch.zeros(4, device='cuda', dtype=torch.float64)
    st = stream_ptr()

    def update(r, g, clip_dev):
        if kind == 'adam':
            common = (r['p'].data_ptr(), g.data_ptr(), r['m'].data_ptr(), r['v'].data_ptr(), n, 3e-3, lr_dev.data_ptr(), 0.9, 0.999, 1e-8,
                      3e-4, r['steps'].data_ptr(), None, 1)
            lib.pp_adam_step_dev(*common, st) if clip_dev is None else lib.pp_adam_step_clip(*common, clip_dev, st)
        else:
            common = (r['p'].data_ptr(), g.data_ptr(), r['m'].data_ptr(), n, 3e-3, lr_dev.data_ptr(), 0.9, 3e-4, r['steps'].data_ptr(), None, 1)
            lib.pp_sgd_momentum_step_dev(*common, st) if clip_dev is None else lib.pp_sgd_momentum_step_clip(*common, clip_dev, st)

    for it in range(3):
        g = (torch.randn(n, generator=gen) * 10.0 ** float(it - 1)).cuda()
        raw = g.clone()
        rows = int(lib.pp_grad_sumsq_rows(n))
        partial = torch.zeros(rows, device='cuda', dtype=torch.float64)
        out2 = torch.zeros(2, device='cuda')
        lib.pp_grad_sumsq(g.data_ptr(), n, partial.data_ptr(), st)
        lib.pp_grad_clip_finalize(partial.data_ptr(), rows, 0.3 * float(g.double().norm()), None, out2.data_ptr(), stats.data_ptr(), st)
        update(runs['clip'], g, out2.data_ptr() + 4)
        torch.cuda.synchronize()
        coef = out2[1:2].clone()
        assert 0.29 < float(coef) < 0.31
        assert torch.equal(g, raw)                                   # the gradient slab is not scaled in place
        update(runs['ref'], g.mul(coef), None)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(runs['clip'][k], runs['ref'][k]), (it, k)
    assert int(runs['clip']['steps']) == int(runs['ref']['steps']) == 3
    assert stats.tolist()[:2] == [3.0, 3.0]


def _run_steps(opt_cls, steps, max_grad_norm, **kw):
    from pacingpseudo_amd import optim
    args = _small_args()
    torch.manual_seed(3)
    model = build_model(args)
    opt = getattr(optim, opt_cls)(model.parameters(), max_grad_norm=max_grad_norm, **kw)
    batch = _small_batch()
    for _ in range(steps):
        iteration(model, opt, batch, args, 0)
    torch.cuda.synchronize()
    return model, opt


@pytest.mark.parametrize('opt_cls,kw', [('FusedAdam', dict(lr=1e-3, weight_decay=3e-4)),
                                        ('FusedSGD', dict(lr=1e-2, momentum=0.9, weight_decay=3e-4))])
def test_off_is_off_and_inf_only_measures(opt_cls, kw):
    """G4: three steps with max_grad_norm=None and three from the same seed with max_grad_norm=inf: parameters and optimizer
    state identical; None has no read side, inf counted three unclipped steps."""
    m_off, o_off = _run_steps(opt_cls, 3, None, **kw)
    m_inf, o_inf = _run_steps(opt_cls, 3, math.inf, **kw)
    assert torch.equal(m_off.flat.params, m_inf.flat.params)
    s_off, s_inf = o_off.state_dict()['slabs'][0], o_inf.state_dict()['slabs'][0]
    for k in o_off.STATE_KEYS:
        assert torch.equal(s_off[k], s_inf[k]), k
    assert s_off['steps'] == s_inf['steps'] == {'backbone': 3, 'aux_path': 3}
    assert o_off.last_grad_norm is None and o_off.last_clip_coef is None and o_off.clip_stats() is None
    assert 'clip' not in next(iter(o_off._slabs.values()))          # off allocates and launches nothing
    st = o_inf.clip_stats()
    assert st['steps'] == 3 and st['clipped'] == 0 and 0 < st['mean_norm'] <= st['max_norm'] < math.inf
    assert float(o_inf.last_clip_coef) == 1.0 and o_inf.last_grad_norm.shape == (1,) and o_inf.last_grad_norm.is_cuda
    assert o_inf.clip_stats(reset=True)['steps'] == 3 and o_inf.clip_stats()['steps'] == 0


@pytest.mark.parametrize('opt_cls', ['FusedSGD', 'FusedAdam'])
def test_clipped_steps_match_torch(opt_cls):
    """G5: gradients from the device, CPU clip_grad_norm_ + torch.optim.SGD / Adam (float64) on copies; max_norm derived from
    the first step's norm: 0.5 x (must clip) and 10 x (must not).  Tolerances of the unclipped comparisons."""
    from pacingpseudo_amd import optim
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=3e-4) if opt_cls == 'FusedSGD' else dict(lr=1e-3, weight_decay=3e-4)
    args = _small_args()
    batch = _small_batch()
    # one unclipped step: the norm of the first step, checked against the parameters' OWN gradients (the slab's alignment
    # padding is inside the segment ranges the kernel sums over and must contribute nothing)
    torch.manual_seed(3)
    model = build_model(args)
    opt = getattr(optim, opt_cls)(model.parameters(), max_grad_norm=math.inf, **kw)
    _, grads = iteration(model, opt, batch, args, 0)
    first = float(opt.last_grad_norm)
    own = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values() if g is not None))
    print(f'{opt_cls}: first-step norm {first!r}, from the parameter gradients {own!r}')
    assert abs(first - own) <= REL * own
    for factor, must_clip in ((0.5, True), (10.0, False)):
        torch.manual_seed(3)
        model = build_model(args)
        ref_params = {k: torch.nn.Parameter(p.detach().cpu().double().clone()) for k, p in model.named_parameters() if p.requires_grad}
        ref_cls = torch.optim.SGD if opt_cls == 'FusedSGD' else torch.optim.Adam
        ref_opt = ref_cls(list(ref_params.values()), **kw)
        opt = getattr(optim, opt_cls)(model.parameters(), max_grad_norm=factor * first, **kw)
        for it in range(3):
            _, grads = iteration(model, opt, batch, args, 0)
            for k, p in ref_params.items():
                p.grad = grads[k].cpu().double().clone()
            ref_norm = torch.nn.utils.clip_grad_norm_(list(ref_params.values()), factor * first, norm_type=2)
            ref_opt.step()
            print(f'{opt_cls} x{factor} step {it}: norm {float(opt.last_grad_norm)!r} (torch {float(ref_norm)!r}), '
                  f'coef {float(opt.last_clip_coef)!r}')
            assert abs(float(opt.last_grad_norm) - float(ref_norm)) <= REL * float(ref_norm)
            for k, p in model.named_parameters():
                if not p.requires_grad:
                    continue
                got, ref = p.detach().cpu().double(), ref_params[k].detach()
                if opt_cls == 'FusedSGD':
                    assert torch.allclose(got, ref, rtol=2e-6, atol=1e-8), (factor, it, k, float((got - ref).abs().max()))
                else:
                    assert float((got - ref).abs().max()) <= 2e-7 * max(1.0, float(ref.abs().max())) + 1e-9, (factor, it, k)
        st = opt.clip_stats()
        assert st['steps'] == 3
        assert (st['clipped'] >= 1) if must_clip else (st['clipped'] == 0), (factor, st)      # not a vacuous configuration


def _loss_fn(args):
    from pacingpseudo_amd.utils import gaussian_ramp_up

    def f(out, epoch):
        loss = out['loss_pce']
        loss = loss + out['loss_ent'] * gaussian_ramp_up(epoch, args.loss_ent_weight, scale=args.ramp_up_scale)
        loss = loss + out['loss_cr'] * gaussian_ramp_up(epoch, args.loss_cr_weight, scale=args.ramp_up_scale)
        return loss + out['loss_aux_cls'] * args.loss_aux_weight + out['loss_memory'] * args.loss_memory_weight
    return f


def test_graph_replay_equals_eager_with_clipping():
    """G6: eager vs GraphedStep, seven steps across an epoch change, FusedAdam at lr 1e-3 with max_norm = 0.5 x the first norm
    (the first step clips, the next two do not: the norm falls); before the fourth step max_grad_norm is lowered on the param
    group to 0.01 x: the graph must capture again and that step -- a replay in the graphed run -- must use the new value.
    Every step's coefficient follows from its norm and the max_norm in force.  Everything bit for bit."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    args = _small_args()
    f = _loss_fn(args)
    batch = {k: v.cuda() for k, v in _small_batch().items() if k != 'label'}
    torch.manual_seed(3)
    probe = build_model(args)
    probe_opt = FusedAdam(probe.parameters(), lr=1e-3, weight_decay=3e-4, max_grad_norm=math.inf)
    GraphedStep(probe, probe_opt, f, warmup=1)(batch, 0)
    first = float(probe_opt.last_grad_norm)
    epochs = [0, 0, 0, 0, 1, 1, 1]
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(3)
        model = build_model(args)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=3e-4, max_grad_norm=0.5 * first)
        gs = GraphedStep(model, opt, f, warmup=10 ** 9 if tag == 'eager' else 1)      # (never leaves the warm-up: the eager step)
        model.train()
        norms, coefs, mid = [], [], None
        for i, ep in enumerate(epochs):
            if ep == 1 and epochs[i - 1] == 0:
                model.eval()
            if i == 3:
                mid = opt.clip_stats()
                opt.param_groups[0]['max_grad_norm'] = 0.01 * first
            gs(batch, ep)
            norms.append(opt.last_grad_norm.clone())
            coefs.append(opt.last_clip_coef.clone())
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(params=model.flat.params.clone(), m=sd['m'], v=sd['v'], steps=sd['steps'], norms=torch.cat(norms).cpu(),
                         coefs=torch.cat(coefs).cpu(), stats=next(iter(opt._slabs.values()))['clip']['stats'].cpu(), mid=mid,
                         captures=gs.captures, replays=gs.replays)
    e, g = runs['eager'], runs['graph']
    print('norms', e['norms'].tolist(), 'coefs', e['coefs'].tolist(), 'stats', e['stats'].tolist(), 'after three steps', e['mid'])
    assert e['captures'] == 0 and g['captures'] == 3 and g['replays'] == 6, (g['captures'], g['replays'])      # first, new max_norm, new epoch
    # some steps clip and some do not, in both halves of the run
    assert 1 <= e['mid']['clipped'] < e['mid']['steps'] == 3, e['mid']
    assert float(e['coefs'][3]) < 1.0, e['coefs']                    # the lowered max_grad_norm is in use at the fourth step
    for i in range(7):
        want = min(1.0, (0.5 if i < 3 else 0.01) * first / (float(e['norms'][i]) + 1e-6))
        assert abs(float(e['coefs'][i]) - want) <= 2 * REL * want, (i, float(e['coefs'][i]), want)
    for k in ('params', 'm', 'v', 'norms', 'coefs', 'stats'):
        assert torch.equal(e[k], g[k]), k
    assert e['steps'] == g['steps'] == {'backbone': 7, 'aux_path': 7} and e['mid'] == g['mid']


@pytest.mark.parametrize('storage', ['fp16', 'bf16'])
def test_norm_is_taken_on_the_unscaled_gradients(storage):
    """G7 (a): 16-bit storage (model and batch of tests/test_gpu_h16.py): the norm is that of the slab AFTER the loss scale was
    removed -- against the float64 norm of flat.grads read back after the step."""
    from pacingpseudo_amd.optim import FusedAdam
    a16 = O.full_flags()
    a16.storage = storage
    torch.manual_seed(1)
    m = build_model(a16)
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.0, max_grad_norm=math.inf)
    batch = {k: v.cuda() for k, v in O.synthetic_batch(2, 128, 128, seed=3, keep=0.05).items() if k != 'label'}
    m.train()
    out = m(batch, mode='train', step=0)
    loss = sum(out[k] for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'))
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert m.engine.last_plan.h16 and m.engine.last_plan.loss_scale > 1.0 and int(m.flat.guard[0]) == 0
    ref = float(np.linalg.norm(m.flat.grads.cpu().numpy().astype(np.float64)))
    got = float(opt.last_grad_norm)
    print(f'{storage}: norm {got!r}, float64 norm of the slab {ref!r}, loss scale {m.engine.last_plan.loss_scale}')
    assert ref > 0 and abs(got - ref) <= REL * ref
    assert opt.clip_stats()['steps'] == 1


def test_overflow_skip_with_clipping_on():
    """G7 (b): fp16 storage with loss scale 2^40 (the setup of test_gpu_h16.py::test_loss_scale_overflow_skips_the_update; bfloat16
    cannot overflow a loss scale) and clipping on: the step is still skipped -- weights, moments and step counts untouched, one
    skipped update counted, clip statistics unchanged."""
    from pacingpseudo_amd.optim import FusedAdam
    a16 = O.full_flags()
    a16.storage = 'fp16'
    torch.manual_seed(1)
    m = build_model(a16)
    m.engine.loss_scale = 2.0 ** 40
    opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    batch = {k: v.cuda() for k, v in O.synthetic_batch(2, 128, 128, seed=3, keep=0.05).items() if k != 'label'}
    m.train()
    before = m.flat.params.clone()
    out = m(batch, mode='train', step=0)
    loss = sum(out[k] for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'))
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert int(m.flat.guard[0]) == 1 and int(m.flat.guard[1]) == 1
    assert torch.equal(m.flat.params, before)
    st = next(iter(opt._slabs.values()))
    assert float(st['m'].abs().max()) == 0.0 and float(st['v'].abs().max()) == 0.0
    assert opt.state_dict()['slabs'][0]['steps'] == {}
    assert opt.clip_stats() == dict(steps=0, clipped=0, mean_norm=0.0, max_norm=0.0)


def test_driver_logs_the_norm_and_resumes_bit_for_bit(tmp_path):
    """G8: train_chaos.py --clip_grad_norm on synthetic data, two epochs: the per-epoch log line, the three scalar tags for both
    epochs; stopped after epoch 0 and resumed it equals the uninterrupted run bit for bit (the method of test_gpu_resume.py,
    whose comparison includes scalars.jsonl and the optimizer's param_groups)."""
    from tests.test_gpu_resume import FULL, SMALL, _resume_case, _scalars
    argv = SMALL + FULL + ['--epoch', '2', '--cpu_input', '--num_workers', '0', '--clip_grad_norm', '1.0']
    full, _, st = _resume_case(tmp_path, 'train_chaos.py', argv, 0, 1)
    assert st['args']['clip_grad_norm'] == 1.0 and st['optimizer']['param_groups'][0]['max_grad_norm'] == 1.0
    log = open(os.path.join(full, 'log.txt')).read()
    sc = _scalars(full)
    for e in (0, 1):
        line = next(ln for ln in log.splitlines() if f'epoch: {e:03d}, grad_norm mean / max:' in ln)
        assert 'of 4 steps clipped' in line, line
        mean, mx, frac = (sc[(t, e)] for t in ('train/grad_norm', 'train/grad_norm_max', 'train/grad_clipped_frac'))
        print(f'epoch {e}: {line.split("] ")[-1]}; scalars {mean!r} {mx!r} {frac!r}')
        assert 0 < mean <= mx < math.inf and 0.0 <= frac <= 1.0


def test_upper_bound_driver_measures_the_norm(tmp_path):
    """upper_bound_chaos.py --clip_grad_norm inf (the bare UNet: one slab segment): the log line and the three tags; nothing clips."""
    from tests.test_gpu_resume import SMALL, _run, _scalars
    run = _run('upper_bound_chaos.py', SMALL + ['--epoch', '1', '--num_workers', '0', '--clip_grad_norm', 'inf'], tmp_path / 'ub', 'ub',
               session='Upperbound')
    assert 'epoch: 000, grad_norm mean / max:' in open(os.path.join(run, 'log.txt')).read()
    sc = _scalars(run)
    assert 0 < sc[('train/grad_norm', 0)] <= sc[('train/grad_norm_max', 0)] < math.inf and sc[('train/grad_clipped_frac', 0)] == 0.0


def test_driver_logs_nothing_when_off(tmp_path):
    """The flag off: no grad_norm line, no train/grad_* tag."""
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'off')
    train_main(['--tag', 'off', '--session', 'Experiment', '--root', root, '--synthetic', '8', '--epoch', '1', '--batch_size', '4',
                '--image_size', '64', '--num_workers', '0', '--cpu_input', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path',
                '--do_memory'])
    run = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-off'))[0]
    log = open(os.path.join(run, 'log.txt')).read()
    assert 'clip_grad_norm=0.0' in log and 'grad_norm mean' not in log and 'steps clipped' not in log      # (the flag dump names the flag)
    tags = {json.loads(ln)['tag'] for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))}
    assert tags and not any(t.startswith('train/grad') for t in tags)


def _rank_run(dist_on, port, out_path):
    """Three clipped FusedAdam steps of the small model; dist_on: inside a ONE-rank RCCL group (parallel.attach: bucketed gradient
    all-reduce, averaged slab) -- each collective is an identity, the library calls are the N > 1 step's."""
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
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=3e-4, max_grad_norm=3.0)
    batch = _small_batch()
    norms = []
    for _ in range(3):
        iteration(model, opt, batch, args, 0)
        norms.append(opt.last_grad_norm.clone())
    torch.cuda.synchronize()
    sd = opt.state_dict()['slabs'][0]
    torch.save(dict(params=model.flat.params.cpu(), m=sd['m'], v=sd['v'], norms=torch.cat(norms).cpu(), stats=opt.clip_stats(),
                    attached=model.engine.comm is not None), out_path)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


def test_clipped_run_inside_a_one_rank_rccl_group(tmp_path):
    """The clipped run inside a one-rank RCCL group equals the single-process run bit for bit: the norm is taken behind the
    all-reduce, on the averaged slab (transport between GPUs stays with the multi-GPU runs)."""
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
    assert 1 <= a['stats']['clipped'] <= 3 and a['stats'] == b['stats'], (a['stats'], b['stats'])
    for k in ('params', 'm', 'v', 'norms'):
        assert torch.equal(a[k], b[k]), k
