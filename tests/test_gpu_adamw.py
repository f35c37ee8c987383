"""Fused AdamW with a per-element exemption from the weight decay (libpacingpseudo_opt.so, ``FusedAdamW``, ``--optimizer adamw
[--wd_exempt_1d]``) on the MI355X.

The reference is ``torch.optim.AdamW`` in float64 on the CPU, with two parameter groups where a mask is given: ``weight_decay``
for the unmarked elements and 0 for the marked ones.  Tolerances are the project's own for fused optimizers against float64 torch:
rtol 2e-6, atol 1e-8 for parameters (tests/test_gpu_round2.py:115, tests/test_gpu_clip.py:225) and, for the shadow slab, that plus
steps * 2^-23 * max|e| (tests/test_gpu_ema.py:177).  What the definition makes exact is compared bit for bit (int32 views).
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests._guard import BandSet  # noqa: E402
from tests.test_gpu_step import build_model, iteration  # noqa: E402

LR, WD, B1, B2, EPS, DECAY, COEF = 1e-3, 0.1, 0.9, 0.999, 1e-8, 0.9, 0.37
STEPS = 3


def _small_args():
    return O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])


def _small_batch():
    return O.synthetic_batch(2, 64, 64, seed=4, keep=0.05)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _trip():
    """Elements one trip of the kernel's grid covers, read from the library's own block cap."""
    from pacingpseudo_amd._opt import opt
    return int(opt.popt_trip_elements())


def _run_mask(n, seed):
    """Random runs of 1 .. 9 marked / unmarked elements: their ends fall at every residue mod 4 once n is large enough."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, 10, size=n)
    ends = np.cumsum(lens)
    idx = np.searchsorted(ends, np.arange(n), side='right')
    return torch.from_numpy(((idx + seed) % 2).astype(np.uint8))


def _grads(n, seed, steps=STEPS):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * 10.0 ** float(it - 1) for it in range(steps)]


class _Slab:
    """p, g, m, v, ema and the mask of one raw launch range, each between sentinel bands of its own."""

    def __init__(self, p0, mask=None, ema=False, pattern=0xFF):
        n = p0.numel()
        self.n, self.bs = n, BandSet(pattern, device='cuda')
        self.p = self.bs.tensor(p0.cuda(), label='p')
        self.g = self.bs.tensor((n,), torch.float32, label='g', fill=0.0)
        self.m = self.bs.tensor((n,), torch.float32, label='m', fill=0.0)
        self.v = self.bs.tensor((n,), torch.float32, label='v', fill=0.0)
        self.e = self.bs.tensor(p0.cuda(), label='ema') if ema else None
        self.mask = self.bs.tensor(mask.cuda(), label='mask') if mask is not None else None
        self.step = torch.zeros(1, device='cuda', dtype=torch.int32)

    def common(self, lr=LR, lr_dev=None, wd=WD, skip=None, count_skip=1, a=0, b=None, step=None):
        b = self.n if b is None else b
        return (self.p.data_ptr() + 4 * a, self.g.data_ptr() + 4 * a, self.m.data_ptr() + 4 * a, self.v.data_ptr() + 4 * a, b - a,
                lr, lr_dev, B1, B2, EPS, wd, (self.step if step is None else step).data_ptr(), skip, count_skip,
                None if self.mask is None else self.mask.data_ptr() + a)

    def launch(self, form, clip_dev=None, **kw):
        from pacingpseudo_amd._lib import stream_ptr
        from pacingpseudo_amd._opt import opt
        a = kw.get('a', 0)
        if form == 'plain':
            opt.popt_adamw_step(*self.common(**kw), stream_ptr())
        elif form == 'clip':
            opt.popt_adamw_step_clip(*self.common(**kw), clip_dev, stream_ptr())
        else:
            opt.popt_adamw_step_ema(*self.common(**kw), self.e.data_ptr() + 4 * a, DECAY, clip_dev, stream_ptr())


def _reference(p0, mask, grads, clip, lr=LR, wd=WD):
    """torch.optim.AdamW in float64: two groups split by the mask; the EMA rule in double beside it.  Returns (p, ema)."""
    n = p0.numel()
    marked = torch.zeros(n, dtype=torch.bool) if mask is None else mask.bool()
    parts = [(~marked, wd), (marked, 0.0)]
    params = [torch.nn.Parameter(p0[sel].double().clone()) for sel, _ in parts]
    groups = [dict(params=[q], weight_decay=w) for q, (sel, w) in zip(params, parts) if q.numel()]
    ref = torch.optim.AdamW(groups, lr=lr, betas=(B1, B2), eps=EPS, amsgrad=False, maximize=False)
    ema = p0.double().clone()
    for t, g in enumerate(grads):
        gc = (g * torch.tensor(COEF, dtype=torch.float32)) if clip else g          # rounded to fp32 on its own
        for q, (sel, _) in zip(params, parts):
            q.grad = gc[sel].double()
        ref.step()
        now = torch.empty(n, dtype=torch.float64)
        for q, (sel, _) in zip(params, parts):
            now[sel] = q.detach()
        ema += (1.0 - min(DECAY, (1.0 + t) / (10.0 + t))) * (now - ema)
    return now, ema


def _close(got, ref, slack=0.0):
    return bool(((got.double() - ref).abs() <= 1e-8 + 2e-6 * ref.abs() + slack).all())


# ---------------------------------------------------------------- 7. raw entry points against torch.optim.AdamW in float64
@pytest.fixture(scope='module')
def big_case():
    """The one large case, computed once: n = C + 5, the smallest size at which the grid-stride loop and the tail both run."""
    n = _trip() + 5
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(77))
    mask = _run_mask(n, 5)
    grads = _grads(n, 78)
    return n, p0, mask, grads, {clip: _reference(p0, mask, grads, clip) for clip in (False, True)}


def _check_raw(n, p0, mask, grads, refs, cases):
    lr_scalar = torch.full((1,), LR, device='cuda')
    coef = torch.full((1,), COEF, device='cuda')
    for form, on_device in cases:
        clip = form in ('clip', 'ema+clip')
        s = _Slab(p0, mask, ema=form.startswith('ema'))
        # lr through lr_dev: the host value is then a decoy the kernel must not use
        kw = dict(lr=0.5, lr_dev=lr_scalar.data_ptr()) if on_device else dict(lr=LR, lr_dev=None)
        for g in grads:
            s.g.copy_(g)
            s.launch(form.split('+')[0] if form != 'clip' else 'clip', coef.data_ptr() if clip else None, **kw)
        torch.cuda.synchronize()
        ref_p, ref_e = refs[clip]
        got = s.p.cpu()
        tag = (n, form, on_device)
        print(f'n={n} {form} lr_dev={on_device}: worst |p - ref| - 2e-6 |ref| = {float(((got.double() - ref_p).abs() - 2e-6 * ref_p.abs()).max()):.3e}')
        assert _close(got, ref_p), tag
        if s.e is not None:
            slack = len(grads) * 2.0 ** -23 * float(ref_e.abs().max())
            assert _close(s.e.cpu(), ref_e, slack), tag
        assert int(s.step) == len(grads), tag
        assert s.bs.damaged() == [], tag
        assert torch.equal(s.mask.cpu(), mask) and torch.equal(s.g.cpu(), grads[-1]), tag          # only read


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1021])
def test_raw_entry_points_against_torch_adamw(n):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(100 + n))
    grads = _grads(n, 200 + n)
    masks = [_run_mask(n, 1), _run_mask(n, 2)]
    if n == 1021:
        m = masks[0].numpy().astype(np.int8)
        change = np.nonzero(np.diff(m))[0] + 1
        starts, ends = change[m[change] == 1], change[m[change] == 0]
        assert {int(s) % 4 for s in starts} == {0, 1, 2, 3} == {int(e) % 4 for e in ends}          # every residue mod 4
    cases = [(form, dev) for form in ('plain', 'clip', 'ema', 'ema+clip') for dev in (False, True)]
    for mask in masks:
        refs = {clip: _reference(p0, mask, grads, clip) for clip in (False, True)}
        _check_raw(n, p0, mask, grads, refs, cases)


@pytest.mark.parametrize('form,on_device', [('plain', False), ('ema+clip', True)])
def test_raw_entry_points_past_one_trip_of_the_grid(big_case, form, on_device):
    n, p0, mask, grads, refs = big_case
    assert n == _trip() + 5 and n % 4 == 1 and n > 4 * 256 * 1024
    _check_raw(n, p0, mask, grads, refs, [(form, on_device)])


# ---------------------------------------------------------------- 8. bit-for-bit properties
N8 = 4 * 256 * 3 + 3          # three blocks and a tail of three


def _three_steps(p0, mask, form='plain', wd=WD, clip=False, pattern=0xFF):
    s = _Slab(p0, mask, ema=form == 'ema', pattern=pattern)
    coef = torch.full((1,), COEF, device='cuda')
    for g in _grads(p0.numel(), 9):
        s.g.copy_(g)
        s.launch(form, coef.data_ptr() if clip else None, wd=wd)
    torch.cuda.synchronize()
    assert s.bs.damaged() == []
    return s


def test_mask_extremes_equal_the_unmasked_calls_bitwise():
    p0 = torch.randn(N8, generator=torch.Generator().manual_seed(8))
    ones, zeros = torch.ones(N8, dtype=torch.uint8), torch.zeros(N8, dtype=torch.uint8)
    other = torch.full((N8,), 0x80, dtype=torch.uint8)          # non-zero = not decayed, whatever the byte
    for form in ('plain', 'ema'):
        no_wd, with_wd = _three_steps(p0, None, form, wd=0.0), _three_steps(p0, None, form)
        assert not _same_bits(no_wd.p, with_wd.p)          # the decay does something: not a vacuous comparison
        for mask, twin in ((ones, no_wd), (other, no_wd), (zeros, with_wd)):
            s = _three_steps(p0, mask, form)
            for k in ('p', 'm', 'v') + (('e',) if form == 'ema' else ()):
                assert _same_bits(getattr(s, k), getattr(twin, k)), (form, int(mask[0]), k)
        # the moments never see the decay
        assert _same_bits(no_wd.m, with_wd.m) and _same_bits(no_wd.v, with_wd.v)


def test_both_band_patterns_give_the_same_bits():
    """Nothing outside [0, n) reaches a result: 0xFF bands (NaN) and 0xA5 bands (small finite values) give the same p, m, v, e."""
    p0 = torch.randn(N8, generator=torch.Generator().manual_seed(8))
    mask = _run_mask(N8, 3)
    a, b = _three_steps(p0, mask, 'ema', clip=True), _three_steps(p0, mask, 'ema', clip=True, pattern=0xA5)
    for k in ('p', 'm', 'v', 'e'):
        assert _same_bits(getattr(a, k), getattr(b, k)) and bool(torch.isfinite(getattr(a, k)).all()), k


def test_ema_form_without_clip_equals_the_plain_form_bitwise():
    p0 = torch.randn(N8, generator=torch.Generator().manual_seed(8))
    mask = _run_mask(N8, 3)
    plain, ema = _three_steps(p0, mask, 'plain'), _three_steps(p0, mask, 'ema')
    for k in ('p', 'm', 'v'):
        assert _same_bits(getattr(plain, k), getattr(ema, k)), k
    assert not _same_bits(ema.e, ema.p)          # the average lags
    clip, ema_clip = _three_steps(p0, mask, 'clip', clip=True), _three_steps(p0, mask, 'ema', clip=True)
    for k in ('p', 'm', 'v'):
        assert _same_bits(getattr(clip, k), getattr(ema_clip, k)), k
    assert not _same_bits(clip.p, plain.p)


def test_zero_padding_stays_zero():
    """Alignment padding holds p = g = 0 and is not marked: after three steps with wd > 0 it is still +0 in p, m, v and ema."""
    p0 = torch.randn(N8, generator=torch.Generator().manual_seed(8))
    pad = torch.zeros(N8, dtype=torch.bool)
    pad[5:8] = pad[1030:1033] = pad[N8 - 3:] = True          # inside lanes, across a block edge, the scalar tail
    p0[pad] = 0.0
    mask = _run_mask(N8, 3)
    mask[pad] = 0
    s = _Slab(p0, mask, ema=True)
    for g in _grads(N8, 9):
        g[pad] = 0.0
        s.g.copy_(g)
        s.launch('ema')
    torch.cuda.synchronize()
    for k in ('p', 'm', 'v', 'e'):
        assert bool((_bits(getattr(s, k))[pad.cuda()] == 0).all()), k
    assert bool((s.p[~pad.cuda()] != 0).all())


def test_without_decay_it_is_adam():
    """weight_decay = 0: the arithmetic of pp_adam_step_dev at weight_decay = 0.  Compared at the parameter tolerance; the count of
    elements whose bits differ is printed, not asserted (two translation units: nobody has checked that they round alike)."""
    from pacingpseudo_amd._lib import lib, stream_ptr
    p0 = torch.randn(N8, generator=torch.Generator().manual_seed(8))
    ours = _three_steps(p0, _run_mask(N8, 3), wd=0.0)
    p, m, v = p0.cuda(), torch.zeros(N8, device='cuda'), torch.zeros(N8, device='cuda')
    step = torch.zeros(1, device='cuda', dtype=torch.int32)
    for g in _grads(N8, 9):
        g = g.cuda()
        lib.pp_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N8, LR, None, B1, B2, EPS, 0.0, step.data_ptr(),
                             None, 1, stream_ptr())
    torch.cuda.synchronize()
    differ = {k: int((_bits(a) != _bits(b)).sum()) for k, a, b in (('p', ours.p, p), ('m', ours.m, m), ('v', ours.v, v))}
    print(f'popt_adamw_step(wd=0) against pp_adam_step_dev(wd=0), {N8} elements, three steps: elements whose bits differ: {differ}')
    assert _close(ours.p.cpu(), p.cpu().double())
    assert int(step) == int(ours.step) == STEPS


# ---------------------------------------------------------------- 9. skipped step
def test_skipped_step_touches_nothing_and_is_counted_once():
    a0, b0, a1, b1 = 0, 1028, 1028, 1028 + 515          # two active segments; the second ends in a tail of three
    n = b1
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(9))
    mask = _run_mask(n, 4)
    g = _grads(n, 10, 1)[0]
    coef = torch.full((1,), COEF, device='cuda')
    for form in ('plain', 'clip', 'ema'):
        clip_dev = coef.data_ptr() if form == 'clip' else None
        s, twin = _Slab(p0, mask, ema=form == 'ema'), _Slab(p0, mask, ema=form == 'ema')
        for x in (s, twin):
            x.g.copy_(g)
            x.m.copy_(torch.randn(n, generator=torch.Generator().manual_seed(11)) * 0.1)          # state worth keeping
            x.v.copy_(torch.rand(n, generator=torch.Generator().manual_seed(12)) * 0.01)
            x.steps = torch.zeros(2, device='cuda', dtype=torch.int32)
        before = {k: getattr(s, k).clone() for k in ('p', 'm', 'v') + (('e',) if form == 'ema' else ())}
        skip = torch.tensor([1, 7], device='cuda', dtype=torch.int32)

        def step(x, skip_ptr):
            x.launch(form, clip_dev, a=a0, b=b0, step=x.steps[0:1], skip=skip_ptr, count_skip=1)
            x.launch(form, clip_dev, a=a1, b=b1, step=x.steps[1:2], skip=skip_ptr, count_skip=0)
            torch.cuda.synchronize()
        step(s, skip.data_ptr())
        for k, was in before.items():
            assert _same_bits(getattr(s, k), was), (form, k)          # the decay did not leak into the skipped step
        assert s.steps.tolist() == [0, 0] and skip.tolist() == [1, 8], form          # not advanced; counted exactly once
        skip[0] = 0
        step(s, skip.data_ptr())
        step(twin, None)          # the same step on a twin that never saw the skipped one: t = 1 in its bias corrections
        assert s.steps.tolist() == twin.steps.tolist() == [1, 1] and skip.tolist() == [0, 8], form
        for k, was in before.items():
            assert _same_bits(getattr(s, k), getattr(twin, k)) and not _same_bits(getattr(s, k), was), (form, k)
        assert s.bs.damaged() == [] and twin.bs.damaged() == []
    # and t = 1 it is: against float64 from zero moments (the plain form, one step)
    s = _Slab(p0, mask)
    s.g.copy_(g)
    skip = torch.tensor([1, 0], device='cuda', dtype=torch.int32)
    s.launch('plain', skip=skip.data_ptr())
    skip[0] = 0
    s.launch('plain', skip=skip.data_ptr())
    torch.cuda.synchronize()
    assert _close(s.p.cpu(), _reference(p0, mask, [g], False)[0]) and int(s.step) == 1 and skip.tolist() == [0, 1]


# ---------------------------------------------------------------- 10. FusedAdamW on the small model
def _first_norm(args, batch):
    from pacingpseudo_amd.optim import FusedAdamW
    torch.manual_seed(3)
    model = build_model(args)
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=math.inf)
    iteration(model, opt, batch, args, 0)
    return float(opt.last_grad_norm)


@pytest.mark.parametrize('case', ['off', 'exempt', 'ema', 'clip'])
def test_fused_adamw_against_torch_in_float64(case):
    """20 steps, gradients from the device.  off / exempt: exempt_1d off / on; ema: + ema_decay 0.9; clip: + max_grad_norm at half the
    first step's measured norm, the CPU side through clip_grad_norm_ (tests/test_gpu_clip.py:188).

    lr = 2^-10 and weight_decay = 2^-3 here, so that the decay factor f = 1 - 2^-13 is an fp32 number.  The definition forms f once
    per launch as ONE fp32 value; where it is not representable its rounding error e_f <= 2^-25 is the same relative error in every
    step of every decayed element, and an element that walks from |p| ~ 0.02 to ~ 0 in 20 steps (|update| ~ lr per step) collects
    20 * e_f * |p| of it while the tolerance's rtol term sees only the final |p|: up to 20 * 3e-8 * 0.02 = 1.2e-8, more than the
    whole atol.  Measured at lr 1e-3, wd 0.1 (e_f = 1.66e-8), 20 steps, worst |p - ref| - 2e-6 |ref|: 8.7e-9 (exempt_1d off) and
    1.004e-8 (on) against the atol of 1e-8, where wd = 0 gives 4.3e-9, FusedAdam at wd 3e-4 4.3e-9, and torch's own fp32 CPU AdamW
    5.7e-9 / 4.9e-9 / 3.2e-9 in the same three runs.  That is the constant's rounding, which torch's fp32 AdamW has too, not the
    kernel's; with f exact the comparison measures the kernel.  The raw entry points are compared at lr 1e-3, wd 0.1 above."""
    from pacingpseudo_amd.optim import FusedAdamW
    steps = 20
    LR, WD = 2.0 ** -10, 2.0 ** -3
    assert float(torch.tensor(1.0 - LR * WD, dtype=torch.float64).float()) == 1.0 - LR * WD          # f is an fp32 number
    args, batch = _small_args(), _small_batch()
    exempt = case != 'off'
    kw = dict(lr=LR, weight_decay=WD, exempt_1d=exempt)
    max_norm = None
    if case == 'ema':
        kw['ema_decay'] = DECAY
    if case == 'clip':
        max_norm = 0.5 * _first_norm(args, batch)
        kw['max_grad_norm'] = max_norm
    torch.manual_seed(3)
    model = build_model(args)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    ref_params = {k: torch.nn.Parameter(p.detach().cpu().double().clone()) for k, p in named}
    ref_ema = {k: p.detach().cpu().double().clone() for k, p in named}
    decayed = [ref_params[k] for k, p in named if not (exempt and p.ndim <= 1)]
    spared = [ref_params[k] for k, p in named if exempt and p.ndim <= 1]
    assert len(spared) == (70 if exempt else 0) and len(decayed) + len(spared) == len(named)
    groups = [dict(params=decayed, weight_decay=WD)] + ([dict(params=spared, weight_decay=0.0)] if spared else [])
    ref_opt = torch.optim.AdamW(groups, lr=LR, betas=(B1, B2), eps=EPS)
    opt = FusedAdamW(model.parameters(), **kw)
    start = model.flat.params.clone()
    for t in range(steps):
        _, grads = iteration(model, opt, batch, args, 0)
        for k, p in ref_params.items():
            p.grad = grads[k].cpu().double().clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(ref_params.values()), max_norm, norm_type=2)
        ref_opt.step()
        w = 1.0 - min(DECAY, (1.0 + t) / (10.0 + t))
        for k, p in ref_params.items():
            ref_ema[k] += w * (p.detach() - ref_ema[k])
    torch.cuda.synchronize()
    state = next(iter(opt._slabs.values()))
    assert ('exempt' in state) == exempt and ('ema' in state) == (case == 'ema')
    if exempt:
        from pacingpseudo_amd.optim import decay_exempt_mask
        assert torch.equal(state['exempt'].cpu(), decay_exempt_mask(model.flat)) and int(state['exempt'].sum()) == 2645
    if case == 'clip':
        st = opt.clip_stats()
        assert st['steps'] == steps and st['clipped'] >= 1          # not a vacuous configuration
    worst = 0.0
    for k, p in named:
        got, ref = p.detach().cpu().double(), ref_params[k].detach()
        worst = max(worst, float(((got - ref).abs() - 2e-6 * ref.abs()).max()))
        assert torch.allclose(got, ref, rtol=2e-6, atol=1e-8), (case, k, float((got - ref).abs().max()))
        if case == 'ema':
            o = model.flat.offsets[p]
            got_e, ref_e = state['ema'][o:o + p.numel()].view(p.shape).cpu().double(), ref_ema[k]
            slack = steps * 2.0 ** -23 * float(ref_e.abs().max())
            assert bool(((got_e - ref_e).abs() <= 1e-8 + 2e-6 * ref_e.abs() + slack).all()), (k, float((got_e - ref_e).abs().max()), slack)
    print(f'{case}: worst |p - ref| - rtol |ref| = {worst:.3e} (atol 1e-8)')
    # the slab's alignment padding is still zero, and the decay is large enough to tell the two references apart
    covered = torch.zeros(model.flat.numel, dtype=torch.bool)
    for p, o in model.flat.offsets.items():
        covered[o:o + p.numel()] = True
    assert int((~covered).sum()) > 0 and bool((_bits(model.flat.params.cpu())[~covered] == 0).all())
    assert not torch.equal(model.flat.params, start)
    assert opt.state_dict()['slabs'][0]['steps'] == {'backbone': steps, 'aux_path': steps}


def test_exemption_changes_exactly_the_one_dimensional_parameters_first():
    """One step from the same state with exempt_1d off and on: m and v are identical (the decay never enters the moments), the 4-D
    parameters are identical, and every 1-D parameter that is not all zeros differs."""
    from pacingpseudo_amd.optim import FusedAdamW
    args, batch = _small_args(), _small_batch()
    runs = {}
    for exempt in (False, True):
        torch.manual_seed(3)
        model = build_model(args)
        start = {k: p.detach().clone() for k, p in model.named_parameters()}
        opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, exempt_1d=exempt)
        iteration(model, opt, batch, args, 0)
        torch.cuda.synchronize()
        runs[exempt] = (model, opt.state_dict()['slabs'][0], start)
    (m_off, s_off, start), (m_on, s_on, _) = runs[False], runs[True]
    assert torch.equal(s_off['m'], s_on['m']) and torch.equal(s_off['v'], s_on['v'])
    changed = 0
    for (k, a), (_, b) in zip(m_off.named_parameters(), m_on.named_parameters()):
        if a.ndim > 1 or not a.requires_grad:
            assert torch.equal(a, b), k
        elif bool((start[k] != 0).any()):          # (a bias that starts at zero has nothing to decay)
            assert not torch.equal(a, b), k
            changed += 1
    assert changed >= 20          # the normalisation weights start at one


def test_frozen_stages_are_neither_updated_nor_decayed():
    from pacingpseudo_amd.optim import FusedAdamW
    from tests.test_gpu_freeze import EPOCH, _batch_cpu, _build, _frozen_keys
    model, args = _build()
    model.freeze_encoder(2)
    model.train()
    opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, exempt_1d=True)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for _ in range(3):
        iteration(model, opt, _batch_cpu(), args, EPOCH)
    torch.cuda.synchronize()
    pre = _frozen_keys(2)
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    n_frozen = 0
    for k, v in model.state_dict().items():
        if k.startswith(pre):
            assert _same_bits(v, start[k]) if v.dtype == torch.float32 else torch.equal(v, start[k]), k
            n_frozen += 1
        elif k in trainable and v.ndim > 1:          # (a conv bias in front of a BatchNorm has a zero gradient and, exempt, no decay)
            assert not torch.equal(v, start[k]), k
    assert n_frozen == 14 * 2
    assert any(k.startswith(pre) and v.ndim == 4 and bool((v != 0).any()) for k, v in start.items())          # weights a decay would move
    assert opt.state_dict()['slabs'][0]['steps'] == {'backbone': 3, 'aux_path': 3}


# ---------------------------------------------------------------- 11. graph replay
def _loss_fn(args):
    from pacingpseudo_amd.utils import gaussian_ramp_up

    def f(out, epoch):
        loss = out['loss_pce']
        loss = loss + out['loss_ent'] * gaussian_ramp_up(epoch, args.loss_ent_weight, scale=args.ramp_up_scale)
        loss = loss + out['loss_cr'] * gaussian_ramp_up(epoch, args.loss_cr_weight, scale=args.ramp_up_scale)
        return loss + out['loss_aux_cls'] * args.loss_aux_weight + out['loss_memory'] * args.loss_memory_weight
    return f


def test_graph_replay_equals_eager():
    """Eager against GraphedStep, four steps (one eager warm-up call, one capture, three replays) with exempt_1d and the average on:
    parameters, moments, shadow and step counts bit for bit; exempt_1d is part of the capture key.  No clipping here."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdamW
    args = _small_args()
    f = _loss_fn(args)
    batch = {k: v.cuda() for k, v in _small_batch().items() if k != 'label'}
    runs = {}
    for tag in ('eager', 'graph'):
        torch.manual_seed(3)
        model = build_model(args)
        opt = FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, exempt_1d=True, ema_decay=DECAY)
        gs = GraphedStep(model, opt, f, warmup=10 ** 9 if tag == 'eager' else 1)
        model.train()
        mask_ptr = None
        for _ in range(4):
            gs(batch, 0)
            state = next(iter(opt._slabs.values()))
            mask_ptr = mask_ptr or state['exempt'].data_ptr()
            assert state['exempt'].data_ptr() == mask_ptr          # never reallocated: the address is baked into the capture
        torch.cuda.synchronize()
        sd = opt.state_dict()['slabs'][0]
        runs[tag] = dict(params=model.flat.params.clone().cpu(), m=sd['m'], v=sd['v'], ema=sd['ema'], steps=sd['steps'],
                         captures=gs.captures, replays=gs.replays)
        if tag == 'graph':
            key = gs._key(batch, 0)
            assert key == gs.key
            opt.param_groups[0]['exempt_1d'] = False
            assert gs._key(batch, 0) != key
            opt.param_groups[0]['exempt_1d'] = True
            assert gs._key(batch, 0) == key
    e, g = runs['eager'], runs['graph']
    assert e['captures'] == 0 and g['captures'] == 1 and g['replays'] == 3
    for k in ('params', 'm', 'v', 'ema'):
        assert _same_bits(e[k], g[k]), k
    assert e['steps'] == g['steps'] == {'backbone': 4, 'aux_path': 4}
    assert not torch.equal(e['ema'], e['params'])


# ---------------------------------------------------------------- 12. drivers
def test_driver_resumes_bit_for_bit(tmp_path):
    """train_chaos.py --optimizer adamw --wd_exempt_1d, two epochs of synthetic 64 x 64 phantoms, stopped after epoch 0 and resumed:
    the final checkpoint and state are bit-identical to the uninterrupted run's; a resume that drops the flag is refused by name."""
    from tests.test_gpu_resume import FULL, SMALL, _driver, _resume_case
    argv = SMALL + FULL + ['--epoch', '2', '--cpu_input', '--num_workers', '0', '--optimizer', 'adamw', '--wd_exempt_1d', '--wd', '0.01']
    full, copy, st = _resume_case(tmp_path, 'train_chaos.py', argv, 0, 1)
    assert st['args']['optimizer'] == 'adamw' and st['args']['wd_exempt_1d'] is True
    group = st['optimizer']['param_groups'][0]
    assert group['exempt_1d'] is True and group['weight_decay'] == 0.01
    assert set(st['optimizer']['slabs'][0]) == {'m', 'v', 'steps'}
    assert st['optimizer']['slabs'][0]['steps'] == {'backbone': 8, 'aux_path': 8}
    assert 'optimizer=adamw\n' in open(os.path.join(full, 'log.txt')).read()
    dropped = [a for a in argv if a != '--wd_exempt_1d']
    r = _driver('train_chaos.py', dropped + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'resumed'),
                                             '--resume', os.path.join(copy, 'ckps', 'state_0.pth')])
    assert r.returncode == 2 and '--wd_exempt_1d' in r.stderr, r.stderr[-2000:]


def test_upper_bound_driver_trains_with_adamw(tmp_path):
    from tests.test_gpu_resume import SMALL, _run, _scalars
    run = _run('upper_bound_chaos.py', SMALL + ['--epoch', '1', '--num_workers', '0', '--optimizer', 'adamw', '--init_ch', '8',
                                                '--max_ch', '64'], tmp_path / 'ub', 'ub', session='Upperbound')
    sc = _scalars(run)
    assert math.isfinite(sc[('losses/loss_ce_train', 0)]) and math.isfinite(sc[('losses/loss_dice_train', 0)])
    assert math.isfinite(sc[('losses/loss_ce_val', 0)])
    assert os.path.isfile(os.path.join(run, 'ckps', 'ckp_0.pth'))
    log = open(os.path.join(run, 'log.txt')).read()
    assert 'optimizer=adamw\n' in log and 'wd_exempt_1d=False\n' in log and 'epoch: 000, lr:' in log
