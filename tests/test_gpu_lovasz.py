"""Lovasz-softmax loss on the device (libpacingpseudo_lov.so): the segmented stable radix sort bit for bit against torch.sort, the
errors, the order, the weights, the loss and dz against the float64 reference of tests/_lovasz_reference.py, determinism and extents
under sentinel bands, and the fully supervised driver with and without --do_loss_lovasz.

Bounds (none of them taken from what the device gives).
  errors   ERR_BOUND = 4 x the largest deviation of torch's own fp32 CPU soft-max from the float64 one over the logits of all cases of
           this file (one figure for the file: a case of two values says nothing about fp32 on its own); the factor 4 because the
           device's exp and division may differ from the host's in the last place.
  order    the reference sorts THE DEVICE'S OWN fp32 errors (bounded above) with torch's stable sort on the CPU: the permutation must
           be equal, no pixel left out.  Two errors 1e-9 apart in float64 legitimately swap in fp32; this chain is exact all the same.
  weights  1e-6 relative to max g against the float64 g of that order: the device rounds once, to fp32.
  loss     ERR_BOUND + 2e-7 against the full float64 reference from the logits: the Lovasz extension of a monotone set function with
           Delta(V) = 1 moves by at most the largest change of an error; two fp32 roundings of a value <= 1 are the 2e-7.
  dz       DZ_BOUND = 8 x what the same formula evaluated in fp32 on the CPU deviates from float64 autograd (relative to max |dz_ref|,
           the largest over all cases), with an upstream gradient of 1.7; DZ_BOUND <= 1e-4, the project's parity tolerance, is asserted."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _lovasz_reference as R  # noqa: E402
from tests._guard import PATTERNS, BandSet  # noqa: E402

pytestmark = pytest.mark.gpu

UP = 1.7
FLT_MIN = 2.0 ** -126          # the smallest normal fp32


def dev():
    return torch.device('cuda', 0)


def _tile():
    from pacingpseudo_amd import _lov
    return _lov.TILE


# ---------------------------------------------------------------- 1. the sort, bit for bit
_SORT_SHAPES = ['1x1', '3x35', '5x63', '5x64', '5x65', '2xT-1', '2xT', '2xT+1', '7x2T+3', '40x4095',
                '2x32T', '2x32T+1', '3x40T+7']      # the last three: either side of the digit table's one-block / chunked scan, and beyond
_SPECIAL = torch.tensor([0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x80000001,
                         0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=torch.int64)


def _sort_shape(name):
    T = _tile()
    s, n = name.split('x')
    return int(s), {'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+3': 2 * T + 3, '32T': 32 * T, '32T+1': 32 * T + 1, '40T+7': 40 * T + 7}.get(n) or int(n)


def _sort_inputs(S, n):
    g = torch.Generator().manual_seed(S * 100003 + n)
    normal = torch.randn(S, n, generator=g)
    special = _SPECIAL[torch.randint(0, len(_SPECIAL), (S, n), generator=g)].to(torch.int32).view(torch.float32)      # int64 -> wraps to the bits
    return {
        'normal': normal,
        'constant': torch.full((S, n), 0.75),
        'four values': torch.tensor([-1.5, 0.0, 0.25, 3.0])[torch.randint(0, 4, (S, n), generator=g)],
        'special': special,
        'sorted': torch.sort(normal, dim=1, descending=True).values,
        'reversed': torch.sort(normal, dim=1).values,
    }


@pytest.mark.parametrize('shape', _SORT_SHAPES)
def test_sort_descending_equals_torch_stable_sort_bit_for_bit(shape):
    from pacingpseudo_amd.utils import sort_descending
    S, n = _sort_shape(shape)
    for kind, v in _sort_inputs(S, n).items():
        ref = torch.sort(v, dim=1, descending=True, stable=True)
        got, perm = sort_descending(v.to(dev()))
        assert perm.dtype == torch.int32 and tuple(perm.shape) == (S, n) == tuple(got.shape)
        assert torch.equal(perm.cpu().long(), ref.indices), (shape, kind)
        assert torch.equal(got.cpu().view(torch.int32), ref.values.view(torch.int32)), (shape, kind)


# ---------------------------------------------------------------- the cases of tests 2 - 5
def _case(name):
    """(logits fp32 (N, K, H, W), target int64 (N, H, W), ignore_index) on the CPU."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    g = torch.Generator().manual_seed(seed)

    def rnd(N, K, H, W):
        # unit-scale logits: with p within 1e-4 of 1 the soft-max Jacobian p (dp - sum p dp) cancels in fp32 and the fp32 formula
        # itself leaves the parity tolerance (DZ_BOUND's condition); the extremes are the cases 'logits +-60' and 'quantised'
        return torch.randn(N, K, H, W, generator=g), torch.randint(0, K, (N, H, W), generator=g)
    shapes = {'1x2x1x1': (1, 2, 1, 1), '1x2x5x7': (1, 2, 5, 7), '2x3x8x8': (2, 3, 8, 8), '2x5x63x65': (2, 5, 63, 65),
              '3x4x64x64': (3, 4, 64, 64), '2x17x9x11': (2, 17, 9, 11), '1x32x8x8': (1, 32, 8, 8),
              '2x2x190x190': (2, 2, 190, 190)}      # 72200 keys per segment: the digit table's chunked scan (more than 32 tiles of 2048)
    if name in shapes:                        # '3x4x64x64': a segment of 12288 keys, more than two tiles
        z, t = rnd(*shapes[name])
        return z, t, None
    if name == 'absent classes':              # class 3 absent from the whole batch, class 2 from image 1 only
        z, t = rnd(2, 5, 63, 65)
        t[t == 3] = 0
        t[1][t[1] == 2] = 4
        return z, t, None
    if name == 'ignored 30%':                 # ignore_index = K on about 30 % of the pixels, image 1 ignored altogether
        z, t = rnd(3, 4, 64, 64)
        t[torch.rand(t.shape, generator=g) < 0.3] = 4
        t[1] = 4
        return z, t, 4
    if name == 'ignored class':               # the ignored value is one of the classes
        z, t = rnd(2, 3, 8, 8)
        return z, t, 1
    if name == 'all ignored':
        z, t = rnd(2, 3, 8, 8)
        return z, torch.full_like(t, 3), 3
    if name == 'out of range':                # K + 3 and -1 without an ignore_index: ignored, not indexed
        z, t = rnd(2, 3, 8, 8)
        m = torch.rand(t.shape, generator=g)
        t[m < 0.2] = 6
        t[m > 0.8] = -1
        return z, t, None
    if name == 'zero logits':                 # every segment has two distinct errors: the tie rule at scale, across tiles
        z, t = rnd(3, 4, 64, 64)
        return torch.zeros_like(z), t, None
    if name == 'logits +-60':                 # errors exactly 0 and 1
        z, t = rnd(2, 3, 8, 8)
        hot = torch.randint(0, 3, t.shape, generator=g)
        return 60.0 * (2.0 * torch.nn.functional.one_hot(hot, 3).permute(0, 3, 1, 2).float() - 1.0), t, None
    if name == 'quantised':                   # multiples of 0.5: many exact ties between different pixels
        z, t = rnd(2, 5, 63, 65)
        return torch.round(z * 2) / 2, t, None
    raise KeyError(name)


_CASES = ['1x2x1x1', '1x2x5x7', '2x3x8x8', '2x5x63x65', '3x4x64x64', '2x17x9x11', '1x32x8x8', '2x2x190x190', 'absent classes', 'ignored 30%',
          'ignored class', 'all ignored', 'out of range', 'zero logits', 'logits +-60', 'quantised']
_MODES = [False, True]
_CONFIGS = [(False, 'present'), (False, 'all'), (True, 'present'), (True, 'all')]
_cache = {}


def _inputs(name):
    if ('in', name) not in _cache:
        _cache[('in', name)] = _case(name)
    return _cache[('in', name)]


def _device_run(name, per_image, classes):
    """One forward with return_parts and one backward with upstream UP on the device, results on the CPU; made once, never changed."""
    key = ('dev', name, per_image, classes)
    if key not in _cache:
        from pacingpseudo_amd.losses.losses import lovasz_softmax_loss
        z, t, ign = _inputs(name)
        zd = z.to(dev()).requires_grad_(True)
        val, err, perm, w = lovasz_softmax_loss(zd, t.to(dev()), ignore_index=ign, per_image=per_image, classes=classes, return_parts=True)
        (val * UP).backward()
        _cache[key] = dict(loss=val.detach().cpu(), errors=err.cpu(), perm=perm.cpu(), weights=w.cpu(), dz=zd.grad.cpu())
    return _cache[key]


def _fp32_formula_dz(z, t, ign, per_image, classes, g64):
    """The backward formula of include/pacingpseudo_lov.h evaluated in fp32 on the CPU, with the weights g rounded to fp32."""
    N, K, H, W = z.shape
    p = torch.softmax(z, dim=1)
    valid = R.valid_mask(t, K, ign)
    fg = torch.nn.functional.one_hot(t.clamp(0, K - 1), K).permute(0, 3, 1, 2).bool() & valid[:, None]
    present = fg.flatten(2).any(2) if per_image else fg.permute(1, 0, 2, 3).flatten(1).any(1)[None].expand(N, K)
    avg = torch.ones_like(present) if classes == 'all' else present
    cnt = avg.sum(1, keepdim=True).float()
    scale = torch.where(avg & (cnt > 0), 1.0 / (cnt * (N if per_image else 1)).clamp(min=1), torch.zeros(()))
    g = g64.float().reshape(K, N, H, W).permute(1, 0, 2, 3)
    dp = torch.sign(p - fg.float()) * g * (scale[:, :, None, None] * torch.tensor(UP)) * valid[:, None].float()
    return p * (dp - (p * dp).sum(1, keepdim=True))


def _bounds():
    """(ERR_BOUND, DZ_BOUND) of the module docstring: from the fp32 CPU arithmetic on the logits of all cases, never from the device."""
    if 'bounds' not in _cache:
        err_dev, dz_dev = 0.0, 0.0
        for name in _CASES:
            z, t, ign = _inputs(name)
            err_dev = max(err_dev, float((torch.softmax(z, 1).double() - torch.softmax(z.double(), 1)).abs().max()))
            for per_image, classes in _CONFIGS:
                zr = z.double().requires_grad_(True)
                val, g64, _ = R.loss(zr, t, ign, per_image, classes)
                (dz_ref,) = torch.autograd.grad(val * UP, zr, allow_unused=True) if val.requires_grad else (None,)
                if dz_ref is None or float(dz_ref.abs().max()) < FLT_MIN:      # no gradient that fp32 can hold: nothing to be relative to
                    continue
                d32 = _fp32_formula_dz(z, t, ign, per_image, classes, g64)
                dz_dev = max(dz_dev, float((d32.double() - dz_ref).abs().max() / dz_ref.abs().max()))
        print(f'fp32 CPU soft-max deviates from float64 by {err_dev:.3e}: ERR_BOUND {4 * err_dev:.3e}; '
              f'fp32 CPU dz formula deviates by {dz_dev:.3e} (relative): DZ_BOUND {8 * dz_dev:.3e}')
        _cache['bounds'] = (4 * err_dev, 8 * dz_dev)
    return _cache['bounds']


def _device_order_reference(name, per_image, classes):
    """The float64 reference along the stable order of the device's own fp32 errors: (loss, g, perms, dz)."""
    key = ('ref', name, per_image, classes)
    if key not in _cache:
        z, t, ign = _inputs(name)
        e_dev = _device_run(name, per_image, classes)['errors']
        zr = z.double().requires_grad_(True)
        val, g, perms = R.loss(zr, t, ign, per_image, classes, sort_errors=e_dev)
        dz = torch.autograd.grad(val * UP, zr)[0] if val.requires_grad else torch.zeros_like(zr)
        _cache[key] = (val.detach(), g, perms, dz)
    return _cache[key]


# ---------------------------------------------------------------- 2. errors
@pytest.mark.parametrize('name', _CASES)
def test_errors_against_float64_softmax(name):
    z, t, ign = _inputs(name)
    bound, _ = _bounds()
    e64, _, valid = R.errors(z, t, ign)
    got = _device_run(name, False, 'present')['errors'].double()
    assert tuple(got.shape) == tuple(e64.shape)
    assert not got[:, ~valid].any()                          # 0 at ignored pixels
    worst = float((got - e64)[:, valid].abs().max()) if valid.any() else 0.0
    print(f'{name}: device errors deviate from float64 by {worst:.3e} (bound {bound:.3e})')
    assert worst <= bound
    for cfg in _CONFIGS[1:]:                                 # the errors do not depend on the mode
        assert torch.equal(_device_run(name, *cfg)['errors'], _device_run(name, False, 'present')['errors'])


# ---------------------------------------------------------------- 3. order and weights
@pytest.mark.parametrize('per_image', _MODES)
@pytest.mark.parametrize('name', _CASES)
def test_order_and_weights_along_the_devices_own_errors(name, per_image):
    z, t, ign = _inputs(name)
    N, K, H, W = z.shape
    run = _device_run(name, per_image, 'present')
    _, g, perms, _ = _device_order_reference(name, per_image, 'present')
    perm = run['perm'].long()
    assert tuple(perm.shape) == ((N * K, H * W) if per_image else (K, N * H * W))
    assert torch.equal(perm, torch.stack(perms))             # every pixel of every segment, ignored ones last in index order
    gmax = float(g.max())
    worst = float((run['weights'].double() - g).abs().max())
    print(f'{name} per_image={per_image}: device g deviates by {worst:.3e}, max g {gmax:.3e}')
    assert worst <= 1e-6 * gmax
    assert torch.equal(run['weights'], _device_run(name, per_image, 'all')['weights'])      # g does not depend on `classes`


# ---------------------------------------------------------------- 4. loss value
@pytest.mark.parametrize('per_image,classes', _CONFIGS)
@pytest.mark.parametrize('name', _CASES)
def test_loss_against_the_float64_reference(name, per_image, classes):
    z, t, ign = _inputs(name)
    bound, _ = _bounds()
    ref = float(R.loss(z.double(), t, ign, per_image, classes)[0])
    got = float(_device_run(name, per_image, classes)['loss'])
    print(f'{name} per_image={per_image} classes={classes}: loss {got:.9f}, reference {ref:.9f}, off by {abs(got - ref):.3e} '
          f'(tolerance {bound + 2e-7:.3e})')
    assert abs(got - ref) <= bound + 2e-7
    if name == 'all ignored':
        assert got == 0.0


# ---------------------------------------------------------------- 5. dz
@pytest.mark.parametrize('per_image,classes', _CONFIGS)
@pytest.mark.parametrize('name', _CASES)
def test_dz_against_float64_autograd(name, per_image, classes):
    _, bound = _bounds()
    assert 0.0 < bound <= 1e-4                               # the bound itself stays within the project's parity tolerance
    dz = _device_run(name, per_image, classes)['dz']
    _, _, _, ref = _device_order_reference(name, per_image, classes)
    top = float(ref.abs().max())
    if top == 0.0:                                           # nothing is averaged: the gradient is exactly 0
        assert not dz.any()
        return
    if top < FLT_MIN:                                        # (logits +-60: |dz_ref| ~ 1e-53) below what fp32 holds: nothing to be relative to
        assert float(dz.abs().max()) <= FLT_MIN
        return
    worst = float((dz.double() - ref).abs().max()) / top
    print(f'{name} per_image={per_image} classes={classes}: dz deviates by {worst:.3e} relative to max |dz_ref| (bound {bound:.3e})')
    assert worst <= bound
    if name == 'ignored 30%':
        z, t, ign = _inputs(name)
        assert not dz.permute(0, 2, 3, 1)[t == ign].any()    # exactly 0 at ignored pixels


def test_a_nan_logit_gives_nan_and_leaves_later_calls_alone():
    from pacingpseudo_amd.losses.losses import lovasz_softmax_loss
    z, t, ign = _inputs('2x5x63x65')
    td = t.to(dev())

    def run(zz, per_image):
        zd = zz.to(dev()).requires_grad_(True)
        v = lovasz_softmax_loss(zd, td, ignore_index=ign, per_image=per_image)
        (v * UP).backward()
        torch.cuda.synchronize()
        return v.detach().cpu(), zd.grad.cpu()
    before = [run(z, pi) for pi in _MODES]
    bad = z.clone()
    bad[1, 2, 30, 31] = float('nan')
    for pi in _MODES:
        v, _ = run(bad, pi)
        assert torch.isnan(v)                                # a defined case: the call returns
    for pi, (v0, d0) in zip(_MODES, before):
        v1, d1 = run(z, pi)
        assert torch.equal(v0, v1) and torch.equal(d0, d1) and torch.isfinite(d1).all()


# ---------------------------------------------------------------- 7. extents and determinism
def _guarded_run(pattern):
    """Every launch of the library between sentinel bands, workspaces of exactly the queried size and stale."""
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._lov import lov
    z, t, _ = _inputs('ignored 30%')
    N, K, H, W = z.shape
    P = N * H * W
    S, n = 3, _tile() + 5
    vals = _sort_inputs(S, n)['four values']
    bs = BandSet(pattern, dev())
    st = stream_ptr()
    zd, tdv, vd = bs.tensor(z.to(dev()), label='z'), bs.tensor(t.to(dev()), label='target'), bs.tensor(vals.to(dev()), label='values')
    up = bs.tensor(torch.tensor([UP], device=dev()), label='upstream')
    srt, sperm = bs.tensor((S, n), torch.float32, 'sorted'), bs.tensor((S, n), torch.int32, 'sort perm')
    ws0 = bs.ws(lov.plov_sort_workspace(S, n), 'sort workspace')
    lov.plov_sort_descending(vd.data_ptr(), S, n, srt.data_ptr(), sperm.data_ptr(), ws0.data_ptr(), ws0.n, st)
    res = [srt, sperm]
    for per_image in (0, 1):
        segs = N * K if per_image else K
        loss, w = bs.tensor((1,), torch.float32, 'loss'), bs.tensor((K, P), torch.float32, 'weights')
        sc, err = bs.tensor((segs,), torch.float32, 'seg scale'), bs.tensor((K, P), torch.float32, 'errors')
        perm, dz = bs.tensor((segs, K * P // segs), torch.int32, 'perm'), bs.tensor((N, K, H, W), torch.float32, 'dz')
        ws = bs.ws(lov.plov_loss_workspace(N, K, H, W, per_image), 'loss workspace')
        assert ws.n >= 16 * K * P
        lov.plov_loss_fwd(zd.data_ptr(), tdv.data_ptr(), N, K, H, W, 1, 4, per_image, 0, loss.data_ptr(), w.data_ptr(), sc.data_ptr(),
                          err.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.n, st)
        lov.plov_loss_bwd(zd.data_ptr(), tdv.data_ptr(), N, K, H, W, 1, 4, per_image, w.data_ptr(), sc.data_ptr(), up.data_ptr(),
                          dz.data_ptr(), st)
        res += [loss, w, sc, err, perm, dz]
    damaged = bs.damaged()
    return [r.clone() for r in res], damaged, vals


def test_same_bits_under_both_band_patterns_and_bands_intact():
    from pacingpseudo_amd.losses.losses import lovasz_softmax_loss
    from pacingpseudo_amd.utils import sort_descending
    runs = []
    for pattern in PATTERNS:
        res, damaged, vals = _guarded_run(pattern)
        assert damaged == [], damaged
        assert all(bool(torch.isfinite(r).all()) for r in res if r.dtype == torch.float32)      # nothing stale reached a result
        runs.append(res)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # two plain runs through the Python surface: the same bits again
    z, t, ign = _inputs('ignored 30%')
    for _ in range(2):
        s, p = sort_descending(vals.to(dev()))
        assert torch.equal(s, runs[0][0]) and torch.equal(p, runs[0][1])
        for per_image in (0, 1):
            zd = z.to(dev()).requires_grad_(True)
            v, err, perm, w = lovasz_softmax_loss(zd, t.to(dev()), ignore_index=ign, per_image=bool(per_image), return_parts=True)
            (v * UP).backward()
            loss0, w0, _, err0, perm0, dz0 = runs[0][2 + 6 * per_image: 8 + 6 * per_image]
            assert torch.equal(v.detach().view(1), loss0) and torch.equal(w, w0) and torch.equal(err, err0)
            assert torch.equal(perm, perm0) and torch.equal(zd.grad, dz0)


# ---------------------------------------------------------------- 8. driver
_DRIVER = ['--synthetic', '8', '--image_size', '64', '--init_ch', '8', '--max_ch', '64', '--batch_size', '4', '--epoch', '2', '--num_workers', '0']


def _run_dir(root, tag):
    runs = glob.glob(os.path.join(root, 't1', 'Upperbound', f'Upperbound-*-fold1-{tag}'))
    assert len(runs) == 1, runs
    return runs[0]


def _fields(line):
    """The field names of an `epoch:` / `val:` log line."""
    return [f.split(':')[0].strip() for f in line.split('] ')[-1].split(', ')]


def test_driver_with_the_flag(tmp_path, monkeypatch, capsys):
    """Four steps (two epochs of two) with --do_loss_lovasz (and the boundary term, to pin the order of the fields): the log and the
    scalars carry the term behind the boundary one, the first step's value is the reference's for that step's logits and label, and the
    state file refuses a resume without the flag."""
    from pacingpseudo_amd.losses import losses as L
    from pacingpseudo_amd.upper_bound import train_main
    real, calls = L.lovasz_softmax_loss, []

    def spy(logits, target, *a, **kw):
        v = real(logits, target, *a, **kw)
        calls.append((torch.is_grad_enabled(), logits.detach().cpu(), target.cpu(), float(v.detach()), kw))
        return v
    monkeypatch.setattr(L, 'lovasz_softmax_loss', spy)
    root = str(tmp_path / 'on')
    train_main(['--tag', 'lv', '--root', root, '--do_loss_lovasz', '--do_loss_boundary', '--state_interval', '1'] + _DRIVER)
    run = _run_dir(root, 'lv')
    train = [c for c in calls if c[0]]
    assert len(train) == 4 and len(calls) > 4                          # four steps, and the validation passes
    _, logits, target, value, kw = train[0]
    assert target.dtype == torch.int64 and tuple(logits.shape) == (4, 5, 64, 64) and kw == dict(ignore_index=5, per_image=False)
    ref = float(R.loss(logits.double(), target, 5)[0])
    tol = 4 * float((torch.softmax(logits, 1).double() - torch.softmax(logits.double(), 1)).abs().max()) + 2e-7
    print(f'first step: loss_lovasz {value:.9f}, reference {ref:.9f} (tolerance {tol:.3e})')
    assert abs(value - ref) <= tol and value != 0.0
    log = open(os.path.join(run, 'log.txt')).read().splitlines()
    for e in (0, 1):
        ep = next(ln for ln in log if f'epoch: {e:03d},' in ln)
        va = next(ln for ln in log if f'val: {e:03d},' in ln)
        assert _fields(ep)[:6] == ['epoch', 'lr', 'loss_ce', 'loss_dice', 'loss_boundary', 'loss_lovasz']
        assert _fields(va)[:5] == ['val', 'loss_ce', 'loss_dice', 'loss_boundary', 'loss_lovasz']
        logged = float(ep.split('loss_lovasz: ')[1].split(',')[0])
        assert abs(logged - (train[2 * e][3] + train[2 * e + 1][3]) / 2) < 2e-6
    sc, order = {}, []
    for line in open(os.path.join(run, 'tb_summary', 'scalars.jsonl')):
        r = json.loads(line)
        sc[(r['tag'], r['step'])] = r['value']
        if r['step'] == 0:
            order.append(r['tag'])
    assert order.index('losses/boundary_weight') < order.index('losses/loss_lovasz_train') < order.index('losses/loss_lovasz_val') \
        < order.index('losses/lovasz_weight')
    for e in (0, 1):
        assert abs(sc[('losses/loss_lovasz_train', e)] - (train[2 * e][3] + train[2 * e + 1][3]) / 2) < 1e-6
        assert np.isfinite(sc[('losses/loss_lovasz_val', e)]) and sc[('losses/lovasz_weight', e)] == 1.0
    # resume: the same command line is accepted by the check, the one without the flag is a usage error
    from pacingpseudo_amd import resume, upper_bound
    from pacingpseudo_amd.train import apply_dataset_preset
    state = os.path.join(run, 'ckps', 'state_1.pth')
    saved = resume.load(state)['args']
    assert saved['do_loss_lovasz'] is True and saved['lovasz_per_image'] is False
    argv = ['--tag', 'lv', '--root', root, '--do_loss_boundary', '--state_interval', '1', '--resume', state] + _DRIVER
    resume.check_compatible(saved, resume.flag_dict(apply_dataset_preset(upper_bound.parser.parse_args(argv + ['--do_loss_lovasz']))), 1, 1)
    capsys.readouterr()
    with pytest.raises(SystemExit) as ex:
        train_main(argv)
    assert ex.value.code == 2 and '--do_loss_lovasz' in capsys.readouterr().err


def test_driver_without_the_flag_is_the_parents(tmp_path):
    """The flag off, in a process of its own: the parent's log fields and scalar tags, and the tenth library is never loaded."""
    root = str(tmp_path / 'off')
    code = ('import sys\n'
            'from pacingpseudo_amd.upper_bound import train_main\n'
            f'train_main({["--tag", "off", "--root", root] + _DRIVER!r})\n'
            'm = sys.modules.get("pacingpseudo_amd._lov")\n'
            'assert m is None or m.lov._dll is None, "libpacingpseudo_lov.so was loaded"\n'
            'assert "libpacingpseudo_lov" not in open("/proc/self/maps").read()\n'
            'print("LOV_NOT_LOADED", m is None)\n')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE')}
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert 'LOV_NOT_LOADED' in r.stdout
    run = _run_dir(root, 'off')
    log = open(os.path.join(run, 'log.txt')).read()
    assert 'do_loss_lovasz=False' in log                               # (the flag dump names the flag)
    for e in (0, 1):
        ep = next(ln for ln in log.splitlines() if f'epoch: {e:03d},' in ln)
        va = next(ln for ln in log.splitlines() if f'val: {e:03d},' in ln)
        assert _fields(ep) == ['epoch', 'lr', 'loss_ce', 'loss_dice', _fields(ep)[-1]] and _fields(ep)[-1].endswith('s/epoch')
        assert _fields(va) == ['val', 'loss_ce', 'loss_dice', _fields(va)[-1]] and _fields(va)[-1].endswith('s/epoch')
        assert 'loss_lovasz' not in ep and 'loss_lovasz' not in va
    tags = {json.loads(ln)['tag'] for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))}
    assert tags and not [t for t in tags if 'lovasz' in t]
    assert {'losses/loss_ce_train', 'losses/loss_dice_train', 'losses/loss_ce_val', 'losses/loss_dice_val', 'lr/current_lr'} <= tags
