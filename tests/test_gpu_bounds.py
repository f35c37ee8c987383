"""Bounds table: every launch entry point the two censuses do not own, behind sentinel bands (tests/_guard.py).

One table (FAMILIES), one adapter per family, one parametrised test.  Each case runs TWICE on the same seeded operands -- once
with the bands, the stale workspace content, the not-yet-written outputs and the padding columns at 0xFF (NaN / -1), once at
0xA5 (small finite / a large negative integer) -- and must leave
  * every band intact (a write outside an output, an input or a workspace of exactly the size its query returns),
  * every output finite where the operation is defined,
  * every output BIT-IDENTICAL between the two runs: a read outside the stated extents, a dependence on stale workspace or
    output content and an order-dependent reduction all show here (the project claims no floating-point atomics).
The values themselves are the business of each family's own test and reference; nothing is compared with a reference here.
Shapes are the smallest at which the launchers change path (read off pp_optim.hip, pp_loss.hip, pp_post.hip, pp_augment.hip,
pp_spatial.hip): n around the float4 body / scalar tail of the flat-slab kernels and the first n at which the 4096-block cap makes
the grid-stride loop take a second trip with the tail live; the hand-over of pp_grad_sumsq's unrolled loop and its 1024-row cap;
ragged images (17 x 13, 7 x 9: every extent odd, H W no multiple of 4 nor of a block), the class counts 2, 5, 17, 32, mask on / off,
1 and 3 image channels.  tests/test_bounds_ownership.py (no GPU) holds this table and the census adapters against _lib._PROTOS.
What the bands do not see is stated in tests/_guard.py: an access more than 32 KiB outside a buffer."""
import ctypes
import zlib

import pytest
import torch

from tests._guard import PATTERNS, BandSet

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def _dev():
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------------------------ one run
class Ctx:
    """One run of one case under one pattern: banded operands, seeded values (the same in both runs), recorded calls."""

    def __init__(self, pattern, seed):
        from pacingpseudo_amd._lib import lib, stream_ptr
        self.pattern, self.lib, self.st = pattern, lib, stream_ptr()
        self.bands = BandSet(pattern, _dev())
        self.g = torch.Generator().manual_seed(seed)
        self.results, self.unchanged, self.called, self.keep = [], [], set(), []

    # operands
    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g)

    def randint(self, lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=self.g)

    def inp(self, t, dtype=None, label=None):
        """an input: its values between bands"""
        return self.bands.tensor(t, dtype, label)

    def out(self, shape, dtype=F32, label=None, fill=None, finite=True):
        """an output the call writes completely: stale (the pattern) before, a result afterwards; fill: a defined start value
        where the call accumulates or leaves elements alone"""
        t = self.bands.tensor(shape, dtype, label, fill)
        self.results.append((label or f'output {len(self.results)}', t, finite))
        return t

    def io(self, t, label, dtype=None, finite=True):
        """an operand updated in place: values in, result out"""
        x = self.bands.tensor(t, dtype, label)
        self.results.append((label, x, finite))
        return x

    def rows(self, vals, ld, dtype=F32, label=None, result=False):
        """(..., C) values in rows of length ld whose padding columns hold the pattern"""
        full = self.bands.tensor(tuple(vals.shape[:-1]) + (ld,), dtype, label)
        full[..., :vals.shape[-1]] = vals.to(full.device)
        if result:
            self.results.append((label, full[..., :vals.shape[-1]], True))
        return full

    def ws(self, nbytes, label='workspace'):
        return self.bands.ws(nbytes, label)

    def keep_same(self, label, t):
        """t must hold the same bits after the case as now"""
        self.unchanged.append((label, t, t.clone()))

    def call(self, name, *args):
        self.called.add(name)
        getattr(self.lib, name)(*args, self.st)


def _bits(t):
    return t.contiguous().reshape(-1).view(U8)


def _run_case(fn, pattern, seed):
    c = Ctx(pattern, seed)
    fn(c)
    torch.cuda.synchronize()
    problems = [f'{label}: band damaged [{pattern:#x}]' for label in c.bands.damaged()]
    outs = {}
    for label, t, finite in c.results:
        assert label not in outs, label
        outs[label] = _bits(t).clone()
        if finite and t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
            problems.append(f'{label}: not finite [{pattern:#x}]')
    for label, t, before in c.unchanged:
        if not torch.equal(_bits(t), _bits(before)):
            problems.append(f'{label}: changed [{pattern:#x}]')
    return problems, outs, c.called


def check_case(fn, entries, seed):
    """The assertion of the table: both patterns, bands intact, finite, bit-identical, and the entry points named were called."""
    runs = [_run_case(fn, p, seed) for p in PATTERNS]
    problems = runs[0][0] + runs[1][0]
    for label in runs[0][1]:
        if not torch.equal(runs[0][1][label], runs[1][1][label]):
            diff = int((runs[0][1][label] != runs[1][1][label]).sum())
            problems.append(f'{label}: {diff} bytes differ between the 0xFF and the 0xA5 run')
    assert not problems, '; '.join(problems)
    assert runs[0][2] == set(entries), (sorted(runs[0][2]), sorted(entries))


# ---------------------------------------------------------------------------------------------------------------- flat slabs
CAP_N = 4 * 256 * 4096 + 3      # first n whose float4 body needs a second trip of the 4096-block grid while the scalar tail is live
FLAT_N = (1, 3, 4, 5, 1023, CAP_N)
ADAM = (1e-3, 0.9, 0.999, 1e-8, 3e-4)           # lr, beta1, beta2, eps, weight decay
SGD = (1e-2, 0.9, 3e-4)                         # lr, momentum, weight decay


def _slabs(c, n, names, off):
    """Banded fp32 slabs of n elements; off > 0: each a segment at `off` floats (a multiple of 4) inside a larger banded slab
    whose other elements must not change (optim.py's segments).  -> {name: tensor of n elements}"""
    out = {}
    for i, nm in enumerate(names):
        vals = c.randn(n, scale=0.5) if nm != 'v' else c.rand(n) * 0.1
        if off:
            o = off * (i + 1)
            whole = c.bands.tensor(torch.cat([torch.full((o,), 3.0 + i), vals, torch.full((8,), -2.0 - i)]), label=nm + ' slab')
            c.keep_same(nm + ' slab before the segment', whole[:o])
            c.keep_same(nm + ' slab behind the segment', whole[o + n:])
            t = whole[o:o + n]
            if nm != 'g':
                c.results.append((nm, t, True))
        else:
            t = c.inp(vals, label=nm) if nm == 'g' else c.io(vals, nm)
        out[nm] = t
    return out


def _update_case(opt, form, n, skip=0, off=0):
    """pp_adam_step* / pp_sgd_momentum_step*: form in step, guard, dev, clip, ema, clip_ema"""
    adam = opt == 'adam'
    base = 'pp_adam_step' if adam else 'pp_sgd_momentum_step'
    entry = base + {'step': '', 'guard': '_guard', 'dev': '_dev', 'clip': '_clip', 'ema': '_ema', 'clip_ema': '_ema'}[form]

    def fn(c):
        names = ('p', 'g', 'm', 'v') if adam else ('p', 'g', 'm')
        if 'ema' in form:
            names += ('e',)
        s = _slabs(c, n, names, off)
        state = [s['p'].data_ptr(), s['g'].data_ptr(), s['m'].data_ptr()] + ([s['v'].data_ptr()] if adam else [])
        hyper = ADAM if adam else SGD
        if form in ('step', 'guard'):
            args = state + [n, *hyper, 3]
            if form == 'guard':
                sk = c.io(torch.tensor([skip, 5], dtype=I32), 'skip')
                args.append(sk.data_ptr())
        else:
            step_dev = c.io(torch.tensor([2], dtype=I32), 'step_dev')                  # 4 bytes between bands
            sk = c.io(torch.tensor([skip, 5], dtype=I32), 'skip')                      # 8 bytes
            lr_dev = c.inp(torch.tensor([hyper[0]]), label='lr_dev')
            args = state + [n, 0.0, lr_dev.data_ptr(), *hyper[1:], step_dev.data_ptr(), sk.data_ptr(), 1]
            clip = None
            if 'clip' in form:
                out2 = c.inp(torch.tensor([7.0, 0.625]), label='out2 (clip_dev = out2 + 1)')
                clip = out2.data_ptr() + 4
            if 'ema' in form:
                args += [s['e'].data_ptr(), 0.999, clip]
            elif clip:
                args.append(clip)
        if skip:
            for nm in names:
                c.keep_same(nm + ' (skipped step)', s[nm])
        c.call(entry, *args)
    return fn, (entry,)


def _ema_update_case(n, dev, off=0):
    def fn(c):
        s = _slabs(c, n, ('g', 'e'), off)             # 'g': read only (the live weights p)
        step_dev = c.inp(torch.tensor([4], dtype=I32), label='step_dev') if dev else None
        c.keep_same('p', s['g'])
        c.call('pp_ema_update', s['g'].data_ptr(), s['e'].data_ptr(), n, 0.999, step_dev.data_ptr() if dev else None, 0 if dev else 4)
    return fn, ('pp_ema_update',)


def _two_slab_case(entry, n, off=0):
    def fn(c):
        if entry == 'pp_slab_swap':
            s = _slabs(c, n, ('p', 'm'), off)
            c.call(entry, s['p'].data_ptr(), s['m'].data_ptr(), n)
        else:                                          # pp_fill / pp_scale: one slab
            s = _slabs(c, n, ('p',), off)
            c.call(entry, s['p'].data_ptr(), n, 0.25)
    return fn, (entry,)


def _optim_cases():
    cases = {}
    for n in FLAT_N + (('off', 1023),):
        off, nn = (8, n[1]) if isinstance(n, tuple) else (0, n)
        tag = f'n{nn}' + ('-offset-segments' if off else '')
        for opt in ('adam', 'sgd'):
            for form in ('step', 'dev', 'clip', 'ema', 'clip_ema'):
                cases[f'{opt}_{form}/{tag}'] = _update_case(opt, form, nn, 0, off)
            for skip in (0, 1):
                cases[f'{opt}_guard/skip{skip}/{tag}'] = _update_case(opt, 'guard', nn, skip, off)
            for form in ('dev', 'clip_ema'):
                cases[f'{opt}_{form}/skip1/{tag}'] = _update_case(opt, form, nn, 1, off)
        for dev in (0, 1):
            cases[f'ema_update/{"step_dev" if dev else "t_host"}/{tag}'] = _ema_update_case(nn, dev, off)
        for entry in ('pp_slab_swap', 'pp_fill', 'pp_scale'):
            cases[f'{entry[3:]}/{tag}'] = _two_slab_case(entry, nn, off)
    return cases


# pp_grad_sumsq: rows = min(1024, ceil((n / 4 + 1) / 1024)); the unrolled loop (4 float4 per thread and trip) hands over to the
# single loop where n / 4 leaves a multiple of 4 * rows * 256 -- reachable only under the cap: n / 4 = 4 * 1024 * 256 -+ 1
SUMSQ_N = FLAT_N + (4 * (4 * 1024 * 256 - 1) + 1, 4 * (4 * 1024 * 256 + 1) + 3, 4 * 1023 * 1024 - 1, 4 * 1023 * 1024)


def _sumsq_case(n):
    def fn(c):
        rows = c.lib.pp_grad_sumsq_rows(n)
        assert rows == min(1024, (n // 4 + 1 + 1023) // 1024)
        g = c.inp(c.randn(n), label='g')
        partial = c.out((rows,), F64, 'partial')          # exactly pp_grad_sumsq_rows(n) doubles
        c.call('pp_grad_sumsq', g.data_ptr(), n, partial.data_ptr())
    return fn, ('pp_grad_sumsq',)


def _clip_finalize_case(rows, skip, max_norm):
    def fn(c):
        partial = c.inp(c.rand(rows).double() * 3, label='partial')
        sk = None if skip is None else c.inp(torch.tensor([skip, 0], dtype=I32), label='skip')
        out2 = c.out((2,), F32, 'out2')
        stats = c.io(torch.tensor([3.0, 1.0, 12.5, 6.0], dtype=F64), 'stats')
        c.call('pp_grad_clip_finalize', partial.data_ptr(), rows, max_norm, sk.data_ptr() if sk is not None else None, out2.data_ptr(),
               stats.data_ptr())
    return fn, ('pp_grad_clip_finalize',)


def _clip_cases():
    cases = {f'grad_sumsq/n{n}': _sumsq_case(n) for n in SUMSQ_N}
    for rows in (1, 255, 257, 1024):
        for skip, mx in ((None, 1.0), (0, float('inf')), (1, 1.0)):
            cases[f'grad_clip_finalize/rows{rows}/skip-{skip}/max_norm-{mx}'] = _clip_finalize_case(rows, skip, mx)
    return cases


# -------------------------------------------------------------------------------------------------------------------- losses
IMAGES = ((2, 17, 13), (3, 7, 9))             # N, H, W: every extent odd, H W no multiple of 4
KS = (2, 5, 17, 32)


def _onehot(c, N, K, HW, extra=0):
    t = c.randint(0, K + extra, (N, HW))
    return torch.nn.functional.one_hot(t, K + extra).permute(0, 2, 1).float().contiguous()


def _dice_case(N, K, HW, acc):
    def fn(c):
        z = c.inp(c.randn(N, K, HW, scale=2.0), label='logits')
        lab = c.inp(_onehot(c, N, K, HW), label='label')
        counts = c.out((N, K, 3), F32, 'counts')
        c.call('pp_dice_counts', z.data_ptr(), lab.data_ptr(), N, K, HW, counts.data_ptr())
        sums, loss = c.out((N, K, 3), F64, 'sums'), c.out((), F32, 'loss')
        nws = c.lib.pp_dice_loss_workspace(N, K)
        ws = c.ws(nws)
        c.call('pp_dice_loss_fwd', z.data_ptr(), lab.data_ptr(), N, K, HW, sums.data_ptr(), loss.data_ptr(), ws.data_ptr(), nws)
        g = c.inp(torch.tensor(0.7), label='g')
        dz = c.io(c.randn(N, K, HW), 'dlogits') if acc else c.out((N, K, HW), F32, 'dlogits')
        c.call('pp_dice_loss_bwd', z.data_ptr(), lab.data_ptr(), N, K, HW, sums.data_ptr(), g.data_ptr(), 2.0, dz.data_ptr(), acc)
    return fn, ('pp_dice_counts', 'pp_dice_loss_fwd', 'pp_dice_loss_bwd')


def _pairwise_case(kind, N, K, C, H, W, mask, grad, radius=2, dilation=1):
    """pp_nc_loss_fwd / _bwd and pp_ms_loss_fwd / _bwd"""
    def fn(c):
        z = c.inp(c.randn(N, K, H, W, scale=2.0), label='logits')
        img = c.inp(c.rand(N, C, H, W), label='image')
        m = c.inp((c.rand(N, 1, H, W) > 0.3).float(), label='mask') if mask else None
        unit = c.out((N, K, H, W), F32, 'unit_grad') if grad else None
        sums = c.out((2,), F64, 'sums')
        mp, up = (m.data_ptr() if mask else None), (unit.data_ptr() if grad else None)
        if kind == 'nc':
            av = c.out((N, K, 2), F64, 'assoc_vol')
            nws = c.lib.pp_nc_loss_workspace(N, K, H, W)
            ws = c.ws(nws)
            c.call('pp_nc_loss_fwd', z.data_ptr(), img.data_ptr(), mp, N, K, C, H, W, radius, dilation, 6.0, 0.1, up, av.data_ptr(), sums.data_ptr(),
                   ws.data_ptr(), nws)
        else:
            stats = c.out((N, K, 1 + C), F64, 'stats')
            nws = c.lib.pp_ms_loss_workspace(N, K, C, H, W)
            ws = c.ws(nws)
            c.call('pp_ms_loss_fwd', z.data_ptr(), img.data_ptr(), mp, N, K, C, H, W, 0.1, up, stats.data_ptr(), sums.data_ptr(),
                   ws.data_ptr(), nws)
        if grad:
            g = c.inp(torch.tensor(0.3), label='g_up')
            dl = c.io(c.randn(N, K, H, W), 'dlogits')
            n = N * K * H * W
            if kind == 'nc':
                c.call('pp_nc_loss_bwd', unit.data_ptr(), sums.data_ptr(), g.data_ptr(), 4.0, dl.data_ptr(), n)
            else:
                c.call('pp_ms_loss_bwd', unit.data_ptr(), sums.data_ptr(), 1 if mask else 0, g.data_ptr(), 4.0, dl.data_ptr(), n)
    names = (f'pp_{kind}_loss_fwd',) + ((f'pp_{kind}_loss_bwd',) if grad else ())
    return fn, names


def _weighted_sum_case(n):
    def fn(c):
        terms = [c.inp(c.randn(()), label=f'term {i}') for i in range(n)]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in terms])
        w = (ctypes.c_float * n)(*[0.5 + i for i in range(n)])
        c.keep += [ptrs, w]
        out = c.out((), F32, 'out')
        c.call('pp_weighted_sum_fwd', ptrs, w, n, out.data_ptr())
        g = c.inp(torch.tensor(1.5), label='g')
        gout = c.out((n,), F32, 'gout')
        c.call('pp_weighted_sum_bwd', g.data_ptr(), w, n, gout.data_ptr())
    return fn, ('pp_weighted_sum_fwd', 'pp_weighted_sum_bwd')


def _memory_update_case(entry, hid, h, w, K, H, W, cosine):
    dt = {'pp_memory_update': F32, 'pp_memory_update_h16': torch.float16, 'pp_memory_update_bf16': torch.bfloat16}[entry]

    def fn(c):
        ld = hid + 8
        feat = c.rows(c.randn(h, w, hid), ld, dt, 'feat0')                  # padding columns hold the pattern
        scb = c.inp(_onehot(c, 1, K, H * W, extra=1)[0], label='scribble0')
        bank = torch.zeros(K, hid)
        bank[1 % K] = c.randn(hid)
        bd = c.io(bank, 'bank')
        nws = c.lib.pp_memory_update_workspace(K, hid)
        ws = c.ws(nws)
        c.call(entry, feat.data_ptr(), ld, hid, h, w, scb.data_ptr(), K, H, W, bd.data_ptr(), 0.9, cosine, ws.data_ptr(), nws)
    return fn, (entry,)


def _loss_cases():
    cases = {}
    for N, H, W in IMAGES + ((2, 61, 67),):               # 4087 pixels: more than one block per image
        for K in KS:
            for acc in (0, 1):
                cases[f'dice/{N}x{H}x{W}/K{K}/acc{acc}'] = _dice_case(N, K, H * W, acc)
    for kind in ('nc', 'ms'):
        for N, H, W in IMAGES:
            for K in KS:
                cases[f'{kind}/{N}x{H}x{W}/K{K}/C1/mask/grad'] = _pairwise_case(kind, N, K, 1, H, W, True, True)
            for C in (1, 3):
                for mask in (False, True):
                    for grad in (False, True):
                        cases[f'{kind}/{N}x{H}x{W}/K5/C{C}/{"mask" if mask else "no-mask"}/{"grad" if grad else "value-only"}'] = \
                            _pairwise_case(kind, N, 5, C, H, W, mask, grad)
    # the smallest and the path-changing cases of the families' own tests (tests/test_gpu_nc.py CASES, tests/test_gpu_ms.py SHAPES,
    # tests/test_gpu_classes.py): one class, the largest halo with the run-time channel count, K = 32 with C = 4 (the LDS bound
    # shrinks the class chunks), more than one 64 x 4 tile per image; one-row and one-column images
    for N, K, C, H, W, r, d, mask in ((2, 1, 1, 24, 20, 1, 1, False), (1, 8, 2, 40, 64, 8, 2, True), (1, 32, 4, 20, 70, 4, 4, False),
                                      (1, 5, 1, 70, 130, 4, 1, False)):
        cases[f'nc/{N}x{H}x{W}/K{K}/C{C}/r{r}d{d}/{"mask" if mask else "no-mask"}/grad'] = _pairwise_case('nc', N, K, C, H, W, mask, True, r, d)
    for N, K, C, H, W in ((2, 5, 1, 24, 40), (2, 4, 1, 1, 130), (2, 9, 2, 67, 1), (1, 1, 1, 8, 64), (1, 32, 4, 9, 65)):
        for mask in (False, True):
            cases[f'ms/{N}x{H}x{W}/K{K}/C{C}/{"mask" if mask else "no-mask"}/grad'] = _pairwise_case('ms', N, K, C, H, W, mask, True)
    cases['dice/2x64x64/K5/acc0'] = _dice_case(2, 5, 64 * 64, 0)
    for n in (1, 3, 8):
        cases[f'weighted_sum/n{n}'] = _weighted_sum_case(n)
    for entry in ('pp_memory_update', 'pp_memory_update_h16', 'pp_memory_update_bf16'):
        for (hid, h, w, K, H, W) in ((64, 8, 8, 5, 32, 32), (20, 3, 5, 17, 13, 7), (256, 5, 3, 32, 9, 11), (4, 1, 1, 2, 7, 9)):
            for cosine in (0, 1):
                cases[f'{entry[3:]}/hid{hid}-{h}x{w}-K{K}-{H}x{W}/cosine{cosine}'] = _memory_update_case(entry, hid, h, w, K, H, W, cosine)
    return cases


# ----------------------------------------------------------------------------------------------- metrics and post-processing
def _class_maps(c, N, K, H, W):
    """blobby class maps: a coarse random map up-sampled by 3 (components of several pixels) and a noisy copy"""
    coarse = c.randint(0, K, (N, (H + 2) // 3, (W + 2) // 3))
    a = coarse.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W].contiguous()
    b = torch.where(c.rand(N, H, W) < 0.1, c.randint(0, K, (N, H, W)), a)
    return a, b


def _hd95_case(N, K, H, W):
    def fn(c):
        a, b = _class_maps(c, N, K, H, W)
        pred, lab = c.inp(a, I64, 'pred'), c.inp(b, I64, 'label')
        # dist holds counts-many entries per set, the rest is not written: it starts from zeros and must come back the same
        dist = c.out((N * K, 2, H * W), F32, 'dist', fill=0.0)
        counts = c.out((N * K, 4), I32, 'counts')
        nws = c.lib.pp_hd95_workspace(N, K, H, W)
        ws = c.ws(nws)
        c.call('pp_hd95_surface_distances', pred.data_ptr(), lab.data_ptr(), N, K, H, W, 1.5, 0.75, dist.data_ptr(), counts.data_ptr(),
               ws.data_ptr(), nws)
        out = c.out((N * K, 8), F64, 'surface metrics')
        c.call('pp_surface_reduce', dist.data_ptr(), counts.data_ptr(), N * K, H * W, 95.0, 1.0, out.data_ptr())
    return fn, ('pp_hd95_surface_distances', 'pp_surface_reduce')


def _components_case(N, K, H, W, conn):
    def fn(c):
        a, _ = _class_maps(c, N, K, H, W)
        cls = c.inp(a, I64, 'cls')
        labels = c.out((N, H, W), I32, 'labels')
        n1 = c.lib.pp_components_workspace(N, 1, H, W)
        ws1 = c.ws(n1, 'workspace (label)')
        c.call('pp_label_components', cls.data_ptr(), N, H, W, conn, labels.data_ptr(), ws1.data_ptr(), n1)
        out, stats = c.out((N, H, W), I64, 'kept'), c.out((N, K, 2), I32, 'stats')
        nk = c.lib.pp_components_workspace(N, K, H, W)
        wsk = c.ws(nk, 'workspace (keep largest)')
        c.call('pp_keep_largest_components', cls.data_ptr(), N, K, H, W, conn, out.data_ptr(), stats.data_ptr(), wsk.data_ptr(), nk)
    return fn, ('pp_label_components', 'pp_keep_largest_components')


def _tta_case(N, K, H, W, ops, want_cls):
    def fn(c):
        x = c.inp(c.randn(N, 1, H, W), label='image')
        acc = c.out((N, K, H, W), F32, 'acc')                      # first != 0 stores: the stale content is never read
        for i, op in enumerate(ops):
            Hv, Wv = (W, H) if op & 4 else (H, W)
            view = c.out((N, 1, Hv, Wv), F32, f'view {op}')
            c.call('pp_tta_view', x.data_ptr(), N, H, W, op, view.data_ptr())
            z = c.inp(c.randn(N, K, Hv, Wv, scale=2.0), label=f'logits of view {op}')
            c.call('pp_tta_accumulate', z.data_ptr(), N, K, H, W, op, int(i == 0), acc.data_ptr())
        cls = c.out((N, H, W), I64, 'cls') if want_cls else None
        c.call('pp_tta_finalize', acc.data_ptr(), N, K, H, W, len(ops), cls.data_ptr() if want_cls else None)
    return fn, ('pp_tta_view', 'pp_tta_accumulate', 'pp_tta_finalize')


def _crf_refine_case(N, K, C, H, W, iters, want_cls):
    def fn(c):
        z = c.inp(c.randn(N, K, H, W, scale=2.0), label='logits')
        img = c.inp(c.rand(N, C, H, W), label='image')
        prob = c.out((N, K, H, W), F32, 'prob')
        cls = c.out((N, H, W), I64, 'cls') if want_cls else None
        nws = c.lib.pp_crf_refine_workspace(N, K, H, W)
        ws = c.ws(nws)
        c.call('pp_crf_refine', z.data_ptr(), img.data_ptr(), N, K, C, H, W, iters, 2, 1, 3.0, 0.1, 1.0, 4.0, 2.0, prob.data_ptr(),
               cls.data_ptr() if want_cls else None, ws.data_ptr(), nws)
    return fn, ('pp_crf_refine',)


def _post_cases():
    cases = {}
    for N, H, W in IMAGES:
        for K in KS:
            cases[f'hd95/{N}x{H}x{W}/K{K}'] = _hd95_case(N, K, H, W)
            cases[f'components/{N}x{H}x{W}/K{K}/conn{1 + K % 2}'] = _components_case(N, K, H, W, 1 + K % 2)
            cases[f'tta/{N}x{H}x{W}/K{K}'] = _tta_case(N, K, H, W, tuple(range(8)) if K == 5 else (0, 5), K != 17)
            cases[f'crf_refine/{N}x{H}x{W}/K{K}'] = _crf_refine_case(N, K, 1 + 2 * (K % 2), H, W, 1 + K % 3, K != 17)
    # sizes of the families' own tests: one pixel, one row / column of tiles, partial tiles (tests/test_gpu_postprocess.py,
    # tests/test_gpu_tta.py, tests/test_gpu_crf_refine.py)
    for H, W in ((1, 1), (1, 70), (70, 1), (37, 53)):
        cases[f'components/1x{H}x{W}/K3/conn2'] = _components_case(1, 3, H, W, 2)
        cases[f'tta/1x{H}x{W}/K3'] = _tta_case(1, 3, H, W, (0, 1, 2, 3, 4, 5, 6, 7), True)
    cases['crf_refine/1x37x53/K5'] = _crf_refine_case(1, 5, 1, 37, 53, 5, True)
    cases['crf_refine/1x16x70/K17'] = _crf_refine_case(1, 17, 3, 16, 70, 2, True)
    cases['hd95/1x64x64/K4'] = _hd95_case(1, 4, 64, 64)                     # tests/test_gpu_surface.py's size class
    cases['components/2x63x65/K4/conn1'] = _components_case(2, 4, 63, 65, 1)
    return cases


# ------------------------------------------------------------------------------------------- augmentation, scribble synthesis
AUG_PLANES = ((3, 7, 9), (2, 17, 13), (5, 33, 65))            # B, H, W


def _rects(B, H, W):
    forms = [(0, 0, H, W), (H // 2, W // 3, 1, 1), (H - 1, 0, 1, W), (0, W - 1, H, 1), (1, 1, H - 2, W - 2)]
    return torch.tensor([forms[n % 5] for n in range(B)], dtype=I32)


def _aug_elementwise_case(B, H, W, use_rect):
    def fn(c):
        rect = c.inp(_rects(B, H, W), label='rect') if use_rect else None
        rp = rect.data_ptr() if use_rect else None
        x = c.randn(B, H, W) * 20 + 50
        xs = c.inp(x, label='x (stats)')
        stats = c.out((B, 4), F64, 'stats')
        c.call('pp_aug_stats', xs.data_ptr(), B, H, W, rp, stats.data_ptr())
        stats0 = c.inp(torch.stack([c.rand(B) * 50, c.rand(B) * 20 + 1, -c.rand(B) * 100 - 100, c.rand(B) * 100 + 100], 1).double(),
                       label='stats0')
        par = c.inp(c.rand(B) + 0.5, label='param')
        for mode in range(5):
            coef = c.out((B, 4), F32, f'coef mode {mode}')
            c.call('pp_aug_coef', None if mode == 4 else stats.data_ptr(), stats0.data_ptr() if mode == 3 else None,
                   par.data_ptr() if mode else None, mode, B, coef.data_ptr())
        lin = c.inp(torch.stack([c.rand(B) + 0.5, c.randn(B) * 10, torch.full((B,), 20.0), torch.full((B,), 80.0)], 1), label='linear map')
        y = c.io(x, 'x (scalar map)')
        c.call('pp_aug_scalar_map', y.data_ptr(), B, H, W, lin.data_ptr(), rp)
        mn = x.reshape(B, -1).min(1).values
        gam = c.inp(torch.stack([mn, x.reshape(B, -1).max(1).values - mn + 1e-8, torch.tensor([0.7, 1.5, -1.0])[torch.arange(B) % 3],
                                 torch.zeros(B)], 1), label='gamma map')
        y = c.io(x, 'x (gamma)')
        c.call('pp_aug_gamma', y.data_ptr(), B, H, W, gam.data_ptr(), rp)
        y, f = c.io(x, 'x (add field)'), c.inp(c.randn(B, H, W), label='field')
        c.call('pp_aug_add_field', y.data_ptr(), f.data_ptr(), B, H, W, rp)
        y, sig = c.io(x, 'x (noise)'), c.inp(torch.tensor([0.5, 0.0, 2.0])[torch.arange(B) % 3], label='sigma')
        c.call('pp_aug_add_noise', y.data_ptr(), B, H, W, sig.data_ptr(), rp, 0xABCDEF0123)
        y, other = c.io(x.abs() + 0.5, 'x (mix)'), c.inp(c.rand(B, H, W) + 0.5, label='mix partner')
        lam = c.inp(torch.tensor([0.8, -1.0, 1.0, 0.0])[torch.arange(B) % 4], label='lam')
        c.call('pp_aug_mix', y.data_ptr(), other.data_ptr(), B, H * W, lam.data_ptr())
    return fn, ('pp_aug_stats', 'pp_aug_coef', 'pp_aug_scalar_map', 'pp_aug_gamma', 'pp_aug_add_field', 'pp_aug_add_noise', 'pp_aug_mix')


def _aug_filter_case(B, H, W):
    """pp_aug_gaussian_blur, pp_aug_elastic_field (their scratch planes are workspaces: stale), pp_aug_onehot"""
    def fn(c):
        x = c.io(c.randn(B, H, W), 'x (blur)')
        scr = c.bands.tensor((B, H, W), F32, 'blur scratch')
        sp = c.inp(torch.stack([torch.tensor([1.7, 0.0, 0.6])[torch.arange(B) % 3], torch.zeros(B)], 1), label='sigma_pad')
        c.call('pp_aug_gaussian_blur', x.data_ptr(), scr.data_ptr(), B, H, W, sp.data_ptr())
        disp = c.out((B, 2, H, W), F32, 'disp')
        scr2 = c.bands.tensor((B, 2, H, W), F32, 'field scratch')
        sa = c.inp(torch.tensor([[1.7, 150.0], [0.0, 0.0], [0.6, 40.0]])[torch.arange(B) % 3], label='sigma_alpha')
        c.call('pp_aug_elastic_field', disp.data_ptr(), scr2.data_ptr(), B, H, W, sa.data_ptr(), 4243)
        for K in KS + (KS[-1] + 1,):                  # the class counts, and K + 1 planes as the scribble one-hot has
            lab = c.inp(c.randint(-1, K + 1, (B, H, W)), I32, f'class map K{K}')
            hot = c.out((B, K, H, W), F32, f'one-hot K{K}')
            c.call('pp_aug_onehot', lab.data_ptr(), hot.data_ptr(), B, K, H * W)
    return fn, ('pp_aug_gaussian_blur', 'pp_aug_elastic_field', 'pp_aug_onehot')


def _warp_case(s, r, cubic, outputs, clip, spline=False):
    """pp_aug_warp over one launch of tests/_input_reference.py's case table (8 maps, ragged slices inside planes whose rest
    holds 1e6 / 99); spline: pp_aug_spline_prefilter + pp_aug_warp_spline over its small ragged slices.  The warps take no class
    count: their `lab_pad` argument (R.K here) is the VALUE stored in out_lab / out_scb where the source lies outside the slice
    (pp_augment.hip: `olab[i] = in_src ? lab[...] : lab_pad`), no extent, index or plane count depends on it -- so the class
    counts 2, 5, 17, 32 of the other families have nothing to vary here."""
    def fn(c):
        import numpy as np
        from tests import _input_reference as R
        L = R.spline_launch() if spline else R.warp_launch(s, r)
        B, Hp, Wp = L['img'].shape
        Ho, Wo = (Hp, Wp) if spline else (R.HO, R.WO)
        t = {k: c.inp(torch.from_numpy(np.ascontiguousarray(L[k])), label=k) for k in ('img', 'lab', 'scb', 'maps')}
        disp = c.inp(torch.from_numpy(np.ascontiguousarray(L['disp'])), label='disp') if L.get('disp') is not None else None
        cl = None
        if clip or spline:
            cl = c.inp(torch.from_numpy(np.ascontiguousarray(L['clip'] if spline else R.slice_clip(L['img'], L['sizes']))), label='clip_stats')
        oi = c.out((B, Ho, Wo), F32, 'out_img')
        ol, os_, ov = ((c.out((B, Ho, Wo), I32, 'out_lab'), c.out((B, Ho, Wo), I32, 'out_scb'), c.out((B, Ho, Wo), F32, 'out_valid'))
                       if outputs else (None, None, None))
        p = lambda x: None if x is None else x.data_ptr()       # noqa: E731
        head = (t['img'].data_ptr(), p(t['lab']) if outputs else None, p(t['scb']) if outputs else None, Hp, Wp, oi.data_ptr(), p(ol),
                p(os_), p(ov), Ho, Wo, B, t['maps'].data_ptr(), p(disp))
        if not spline:
            c.call('pp_aug_warp', *head, p(cl), R.IMG_PAD, R.K, cubic)
            return
        use = c.inp(torch.from_numpy(np.ascontiguousarray(L['use'])), label='use')
        d64 = c.inp(torch.from_numpy(np.ascontiguousarray(L['disp64'])), label='disp64')
        # the prefilter writes the (hs + 24) x (ws + 24) corner of the samples that use the spline and nothing else: the rest of
        # the coefficient planes starts from zeros and must come back the same
        coef = c.out((B, Hp + 24, Wp + 24), F64, 'spline coefficients', fill=0.0)
        c.call('pp_aug_spline_prefilter', t['img'].data_ptr(), B, Hp, Wp, t['maps'].data_ptr(), use.data_ptr(), coef.data_ptr())
        c.call('pp_aug_warp_spline', *head, d64.data_ptr(), p(cl), R.IMG_PAD, R.K, cubic, coef.data_ptr(), use.data_ptr())
    return fn, (('pp_aug_spline_prefilter', 'pp_aug_warp_spline') if spline else ('pp_aug_warp',))


def _scribble_case(H, W, M=3):
    def fn(c):
        masks = (c.rand(M, H, W) > 0.35).to(U8)
        m = c.io(masks * 255, 'skeleton')
        c.call('pp_skeletonize', m.data_ptr(), M, H, W)
        seeds = c.io((c.rand(M, H, W) > 0.97).to(U8) * 3, 'seeds')
        area = c.inp(masks * 200, label='dilation mask')
        c.call('pp_dilate_antidiagonal', seeds.data_ptr(), area.data_ptr(), M, H, W, 5)
        img = c.inp((c.rand(M, H, W) > 0.6).to(U8) * 9, label='curves')
        ends = c.out((M, H, W), U8, 'end points')
        c.call('pp_curve_endpoints', img.data_ptr(), ends.data_ptr(), M, H, W)
    return fn, ('pp_skeletonize', 'pp_dilate_antidiagonal', 'pp_curve_endpoints')


def _input_cases():
    cases = {}
    for B, H, W in AUG_PLANES:
        for use_rect in (False, True):
            cases[f'aug_elementwise/{B}x{H}x{W}/{"rect" if use_rect else "whole-plane"}'] = _aug_elementwise_case(B, H, W, use_rect)
        cases[f'aug_filters/{B}x{H}x{W}'] = _aug_filter_case(B, H, W)
    for B, H, W in ((4, 1, 7), (4, 7, 1)):                                          # axes of length 1
        cases[f'aug_filters/{B}x{H}x{W}'] = _aug_filter_case(B, H, W)
    for i, (s, r) in enumerate(((0, 0), (1, 1), (2, 3), (3, 2))):
        cubic = (1, 0, 2, 1)[i]
        cases[f'aug_warp/slices{s}-rects{r}/mode{cubic}/all-outputs'] = _warp_case(s, r, cubic, True, i % 2 == 0)
        cases[f'aug_warp/slices{s}-rects{r}/mode{cubic}/image-only'] = _warp_case(s, r, cubic, False, i % 2 == 1)
    cases['aug_warp_spline/small-ragged-slices'] = _warp_case(0, 0, 1, True, True, spline=True)
    for H, W in ((5, 7), (17, 13), (1, 9), (9, 1), (37, 53)):
        cases[f'scribble/{H}x{W}'] = _scribble_case(H, W)
    return cases


# ------------------------------------------------------------------------------------------------------- weight packs, probe
def _pack_case(O_, I, Ipad):
    def fn(c):
        w = c.inp(c.randn(O_, I, 3, 3), label='w')
        wf, wb = c.out((O_, 9, Ipad), F32, 'wf', fill=0.0), c.out((Ipad, 9, O_), F32, 'wb', fill=0.0)
        c.call('pp_pack_conv3x3_weights_f16x3', w.data_ptr(), O_, I, Ipad, wf.data_ptr(), wb.data_ptr())
        if I == Ipad:
            uf, ub = c.out((36, O_, I), F32, 'Uf', fill=0.0), c.out((36, I, O_), F32, 'Ub', fill=0.0)
            c.call('pp_wino_pack_weights_f16x3', w.data_ptr(), O_, I, 4, uf.data_ptr(), ub.data_ptr())
    return fn, ('pp_pack_conv3x3_weights_f16x3',) + (('pp_wino_pack_weights_f16x3',) if I == Ipad else ())


def _probe_case(blocks):
    def fn(c):
        out = c.out((blocks * 256,), F32, 'out')
        fl = ctypes.c_double()
        c.call('pp_mfma_probe', out.data_ptr(), blocks, 3, ctypes.byref(fl))
    return fn, ('pp_mfma_probe',)


def _misc_cases():
    cases = {f'weight_packs/O{o}-I{i}-Ipad{ip}': _pack_case(o, i, ip) for o, i, ip in ((32, 32, 32), (40, 24, 24), (8, 1, 4), (72, 256, 256))}
    cases['mfma_probe/3-blocks'] = _probe_case(3)
    return cases


# ------------------------------------------------------------------------- 16-bit twins that no plan of the engine reaches
def _rows_out(c, shape, C, ld, dt, label):
    """an NHWC output of row length ld: stale, its first C columns a result, its padding columns to stay the pattern"""
    full = c.bands.tensor(tuple(shape) + (ld,), dt, label)
    c.results.append((label, full[..., :C], True))
    c.keep_same(label + ' padding columns', full[..., C:])
    return full


def _lazy16_case(sfx):
    """pp_conv3x3_fwd_bn_lazy and pp_conv3x3_bwd_weight_f16x3_lazy as _h16 / _bf16: the census replays them in fp32 storage only
    (the 16-bit plans do not take the lazy halo forms), so their 16-bit builds run here, on the smallest shape of the census'
    edge table that pp_conv3x3_lazy_ok accepts, with the padding columns of the activations AND of the coefficient rows stale."""
    dt = torch.float16 if sfx == '_h16' else torch.bfloat16
    B, H, W, C, O_ = 3, 12, 96, 32, 32

    def fn(c):
        from pacingpseudo_amd._lib import PpLazyIn
        assert getattr(c.lib, 'pp_conv3x3_lazy_ok' + sfx)(C, O_, B, H, W, 1) == 1
        w = c.inp(c.randn(O_, C, 3, 3, scale=1 / 17.0), label='w')
        wf, wb = c.out((O_, 9, C), F32, 'wf', fill=0.0), c.out((C, 9, O_), F32, 'wb', fill=0.0)
        c.call('pp_pack_conv3x3_weights_f16x3', w.data_ptr(), O_, C, C, wf.data_ptr(), wb.data_ptr())
        z = c.rows(c.randn(B, H, W, C), C + 8, dt, 'z (lazy input)')
        coef = c.rows(torch.stack([c.rand(C) + 0.3, c.randn(C) * 0.5, torch.full((C,), 0.01)])[None], C + 8, F32, 'lazy coefficient rows')
        lz = PpLazyIn(coef.data_ptr(), C + 8, 1)
        bias, sc, sh = (c.inp(t, label=n) for n, t in (('bias', c.randn(O_)), ('scale', c.rand(O_) + 0.5), ('shift', c.randn(O_))))
        out = _rows_out(c, (B, H, W), O_, O_ + 8, dt, 'z out')
        nst = c.lib.pp_conv3x3_bn_stats_bytes(O_, B, H, W, 1)
        stats = c.bands.tensor((nst // 8,), F64, 'stats')                  # exactly pp_conv3x3_bn_stats_bytes
        rows = ctypes.c_int(0)
        c.keep += [lz, rows]
        c.call('pp_conv3x3_fwd_bn_lazy' + sfx, z.data_ptr(), C + 8, C, wf.data_ptr(), bias.data_ptr(), out.data_ptr(), O_ + 8, O_, B, H, W,
               1, 1, None, 1, sc.data_ptr(), sh.data_ptr(), 0.01, 1, stats.data_ptr(), nst, ctypes.byref(rows), ctypes.byref(lz))
        assert 0 < rows.value * 2 * O_ <= nst // 8
        c.results.append(('stats rows written', stats[:rows.value * 2 * O_], True))
        dz = c.rows(c.randn(B, H, W, O_, scale=1e-2), O_ + 8, dt, 'dz')
        amax = c.inp(dz[..., :O_].float().abs().max().reshape(1), label='dz_amax')
        dw = c.out((O_, C, 3, 3), F32, 'dw')
        nws = c.lib.pp_conv3x3_bwd_weight_workspace(O_, C, B, H, W)
        ws = c.ws(nws)
        c.call('pp_conv3x3_bwd_weight_f16x3_lazy' + sfx, dz.data_ptr(), O_ + 8, O_, z.data_ptr(), C + 8, C, C, B, H, W, 1, dw.data_ptr(), 0,
               ws.data_ptr(), nws, amax.data_ptr(), ctypes.byref(lz))
    return fn, ('pp_pack_conv3x3_weights_f16x3', 'pp_conv3x3_fwd_bn_lazy' + sfx, 'pp_conv3x3_bwd_weight_f16x3_lazy' + sfx)


def _dgrad16_case(sfx, B, H, W, I, acc):
    """pp_conv3x3_bwd_data as _h16 / _bf16 (the fp32-product data gradient on 16-bit tensors: a 16-bit plan takes the split-fp16
    form or none).  The 16-bit build has ONE fp32-product kernel, the first layer's (pp_conv.hip: c4_eligible -- 4 channels in,
    a multiple of 16 up to 64 out, W a multiple of 16) and refuses everything else; as a data gradient that is dz with 4 channels
    and dx with 16 / 48 / 64, at the image sizes of the census' fp32 edge rows."""
    dt = torch.float16 if sfx == '_h16' else torch.bfloat16
    O_ = 4

    def fn(c):
        w = c.inp(c.randn(O_, I, 3, 3, scale=1 / 6.0), label='w')
        wf, wb = c.out((O_, 9, I), F32, 'wf', fill=0.0), c.out((I, 9, O_), F32, 'wb', fill=0.0)
        c.call('pp_pack_conv3x3_weights', w.data_ptr(), O_, I, I, wf.data_ptr(), wb.data_ptr())
        dz = c.rows(c.randn(B, H, W, O_, scale=1e-2), O_ + 8, dt, 'dz')
        if acc:
            dx = c.rows(c.randn(B, H, W, I, scale=1e-2), I + 8, dt, 'dx', result=True)
            c.keep_same('dx padding columns', dx[..., I:])
        else:
            dx = _rows_out(c, (B, H, W), I, I + 8, dt, 'dx')
        c.call('pp_conv3x3_bwd_data' + sfx, dz.data_ptr(), O_ + 8, O_, wb.data_ptr(), dx.data_ptr(), I + 8, I, B, H, W, 1, acc)
    return fn, ('pp_pack_conv3x3_weights', 'pp_conv3x3_bwd_data' + sfx)


def _twin_cases():
    cases = {}
    for sfx in ('_h16', '_bf16'):
        cases[f'lazy_halo{sfx}/3x12x96/C32-O32'] = _lazy16_case(sfx)
        for (B, H, W), I, acc in (((1, 2, 64), 16, 0), ((5, 7, 64), 48, 1), ((3, 5, 128), 64, 0)):
            cases[f'conv3x3_bwd_data{sfx}/{B}x{H}x{W}/O4-C{I}/acc{acc}'] = _dgrad16_case(sfx, B, H, W, I, acc)
    return cases


# one adapter per family: removing a row removes its cases from the test AND its entry points from the ownership gate
FAMILIES = {
    'flat-slab optimizer kernels (pp_optim.hip)': _optim_cases,
    'gradient-norm clipping (pp_optim.hip)': _clip_cases,
    'dice, normalised-cut, Mumford-Shah, weighted sum, memory bank (pp_loss.hip)': _loss_cases,
    'surface distances, components, TTA, CRF refinement (pp_loss.hip, pp_post.hip)': _post_cases,
    'augmentation and scribble synthesis (pp_augment.hip, pp_spatial.hip)': _input_cases,
    'split-fp16 weight packs and the MFMA probe (pp_conv.hip, pp_wino.hip)': _misc_cases,
    '16-bit twins no 16-bit plan takes: lazy halo forms, fp32-product data gradient (pp_conv.hip)': _twin_cases,
}


def all_cases():
    """{case id: (fn, entry points the case calls)} over every family"""
    out = {}
    for family, make in FAMILIES.items():
        for tag, case in make().items():
            assert tag not in out, tag
            out[tag] = case
    return out


def owned_by_family():
    """{family: sorted entry points its cases call}: what tests/test_bounds_ownership.py counts as owned by this table"""
    return {family: sorted({e for _, entries in make().values() for e in entries}) for family, make in FAMILIES.items()}


CASES = all_cases()


@pytest.mark.parametrize('tag', sorted(CASES))
def test_launch_stays_inside_its_buffers_and_reads_nothing_outside(tag):
    fn, entries = CASES[tag]
    check_case(fn, entries, zlib.crc32(tag.encode()))


# ------------------------------------------------------------------------------------------------------------ the gate bites
PLANTS = {'one byte just before the payload': lambda b, G: G - 1, 'one byte just after the payload': lambda b, G: G + b.nbytes,
          'the far end of the front band': lambda b, G: 0, 'the far end of the tail band': lambda b, G: 2 * G + b.nbytes - 1}


@pytest.mark.parametrize('where', sorted(PLANTS))
def test_planted_byte_on_the_device_is_reported(where):
    """tests/test_guard_helper.py's plants on device tensors: plain tensor writes, no kernel of the library."""
    from tests._guard import GUARD
    for pattern in PATTERNS:
        bs = BandSet(pattern, _dev())
        a, b = bs.banded((5, 7), torch.float16, label='a'), bs.banded((5, 7), F32, label='b')
        ws = bs.ws(1000, 'ws')
        assert bs.damaged() == []
        b.full[PLANTS[where](b, GUARD)] = 0
        assert bs.damaged() == ['b'] and a.ok() and ws.ok()
        ws.full[GUARD + 1000] = 0                                   # one byte just past the workspace size
        assert bs.damaged() == ['b', 'ws']


def test_fill_of_one_element_too_many_is_reported():
    """The one plant through a real kernel: pp_fill with n + 1 on a Banded of n floats writes four bytes into the tail band --
    inside the test's own allocation -- and the case must fail, naming the buffer; the honest call passes."""
    n = 1023

    def case(extra):
        def fn(c):
            p = c.out((n,), F32, 'p')
            c.call('pp_fill', p.data_ptr(), n + extra, 0.25)
        return fn
    check_case(case(0), ('pp_fill',), 1)
    with pytest.raises(AssertionError, match='p: band damaged'):
        check_case(case(1), ('pp_fill',), 1)
