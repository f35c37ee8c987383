"""Census of the norm, spatial and loss launches of real steps, each replayed against a float64 reference.

The second half of tests/test_gpu_conv_census.py: the same recording (tests/_launch_census.py, made once per process), and every
launch the convolution census does not own -- BatchNorm / GroupNorm statistics, apply and backward passes, pooling, bilinear
resampling, slab copies, channel scales, the loss kernels -- replayed with every recorded non-pointer argument (ld's, groups,
training, accumulate flags, rows, class counts, slopes) on seeded operands:
  * rows of length ld hold 5.0 in the columns a call must not read, outputs start as 7.0 and their padding is checked afterwards;
    outputs that accumulate start from random content and the sum is compared;
  * normalisation operands are z = sigma_c * randn + mu_c (sigma in [0.5, 2], mu in [-2, 2] per channel), gamma[0] < 0, and the last
    channel is the constant 0.5 -- it sums exactly, so its variance must be exactly 0 and invstd = 1 / sqrt(eps) (a NormProfile of
    the convolution census moves the means to +-r sigma and scales z: tests/test_gpu_norm_range.py);  the partial rows
    of pp_bn_train_finalize[_lazy] are the float64 sums of such a z split into the recorded number of row chunks;
  * references in float64 on the device, one module call per statistics group in order: F.batch_norm / F.group_norm + leaky_relu
    and autograd, max_pool2d, interpolate(align_corners=True); the losses against the float64 restatements of tests/test_gpu_ops.py
    (oracle/pacing_oracle.py);
  * tolerances are the project's own: 1e-4 (activations, data and parameter gradients), 1e-5 (sums, running statistics,
    coefficient rows, bilinear, loss values), the conv-bias gradient of a BatchNorm backward relative to sum |dz| (test_bn_lrelu:
    the sum itself is 0 in train mode); bit equality for pooling, stride-2 gather / scatter, copies without accumulation, arg-max,
    image packing and bilinear at scale 1;
  * 16-bit storage: the _h16 / _bf16 entry against its fp32 twin through _act_ratio, fp32 results at the fp32 tolerance, the twin
    against float64 -- replay() of the convolution census, fed this module's adapters.
dz_amax: every backward form documents *dz_amax = max |dz| OF THE LAUNCH (include/pacingpseudo_hip.h) and clears it first -- the
engine allocates one amax per layer per plan and never resets it.  The replay therefore starts it from a stale LARGER value and
requires the bits of max |dz| of the tensor the launch wrote (fp32 storage; 16-bit storage: within half a 16-bit ulp, the kernel
takes the maximum before the store rounds).
The recording also wraps engine.py's module-level entry-point table, so the launches that bypass plan.K are in it and replayed:
pp_bn_eval_coeffs_batch (every row against float64 and bit for bit against pp_bn_eval_coeffs), the batched split-fp16 weight packs
(bit for bit against the per-layer packs the convolution census feeds its kernels with), pp_scale_guard.  Their item tables are host
arrays the launch shape cannot show, so the adapters build tables of the recorded length over layers of several widths.
Operands, outputs and workspaces lie between the sentinel bands of the convolution census (tests/_guard.py, 0xFF); _bn_ws gives
every BatchNorm launch exactly the bytes include/pacingpseudo_hip.h asks for that entry point.
Together the two censuses own every recorded launch: a name without an adapter in either fails by name; nothing is excluded.
What the operands give up: backward operands are moved off the LeakyReLU kink (|z * scale + shift| >= 1e-4) and the operands of the
pooled forms lie on a 2^-10 grid, because there fp32 and float64 legitimately choose differently; the replay therefore cannot see
a wrong comparison at exactly 0, nor a wrong winner among values closer than 2^-10.  Exact ties it does see: the constant channel
ties all four values of every window (first maximum wins), and tests/test_gpu_ops.py::test_maxpool and the pooled-backward unit
tests keep their tie cases.
The edge table at the end feeds hand-made launch shapes the network never makes to the same adapters: the sizes at which
col_plan / fin_reduce2 (pp_norm.hip) and the bilinear column walker (pp_spatial.hip: the 2 / scale <= 4.1 threshold, the row
bands RB = 8 / 16) change path.  The planted-mistake test shows the gate fails when an entry point is called wrongly.
"""
import ctypes
import math
import zlib
from collections import defaultdict
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests.test_gpu_conv_census import (_NORM_PROFILE, MANT, NORM_CENSUS, TOL, TOL_SUMS, _b, _dev, _empty, _full, _is_conv_launch, _L, _lazy64,  # noqa: E402
                                        _Ops, _p, _Run, _signs, _ws, _zeros, replay as _replay)

TOL_BIL = 1e-5        # test_bilinear
TOL_LOSS = 1e-5       # loss values, bank rows, up-sampled logits (tests/test_gpu_ops.py)
EPS, MOM, SLOPE = 1e-5, 0.1, 0.01


# ------------------------------------------------------------------------------------------------------------------ operands
class _DOps(_Ops):
    """_Ops drawing on the device (the streaming launches are large and many): same seed, same rounding to the storage type."""

    def __init__(self, key):
        super().__init__(key)
        self.g = torch.Generator(device=_dev()).manual_seed(zlib.crc32(repr(key[1:]).encode()))
        self.mu = self.sig = None          # per-channel mean and deviation of the last norm_z under a NormProfile

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g, device=_dev()) * scale

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g, device=_dev())

    def pad(self, vals, ld, fill=5.0):
        """vals (..., C) -> rows of length ld with `fill` in the columns the call must not read."""
        C = vals.shape[-1]
        t = torch.full(vals.shape[:-1] + (ld,), fill, device=_dev())
        t[..., :C] = vals
        return t

    def act(self, B, H, W, ld, C, scale=1.0, fill=5.0):
        return self.pad(self.r(self.randn(B, H, W, C, scale=scale)), ld, fill)

    def norm_z(self, N, H, W, C, grid=None):
        """z = sigma_c * randn + mu_c, last channel constant 0.5 (its fp32 sums are exact: variance exactly 0).  grid: values on
        multiples of it, for the forms that pick the winner of a 2 x 2 window -- two values of a window are then equal or far
        enough apart that fp32 and float64 order y = lrelu(z * scale + shift) alike (a near-tie would move a whole dpool)."""
        sig, mu = self.rand(C) * 1.5 + 0.5, self.rand(C) * 4 - 2
        prof = self.nprof
        if prof.offset is not None:             # NormProfile: mean-to-spread ratio r, sign alternating by channel
            mu = prof.offset * sig * _signs(C, _dev())
        z = self.randn(N, H, W, C) * sig + mu
        if grid:
            z = torch.round(z / grid) * grid
        z[..., C - 1] = 0.5
        if prof.scale:
            z = z * 2.0 ** prof.scale           # exact; the constant channel stays one whose sums are exact
        if prof != NORM_CENSUS:
            mu = mu.clone()
            mu[C - 1] = 0.5
            self.mu, self.sig = mu * 2.0 ** prof.scale, sig * 2.0 ** prof.scale
        return self.r(z)

    def affine(self, C):
        """gamma (gamma[0] < 0), beta, running mean, running variance (under a NormProfile: of the z drawn before it)"""
        gamma = self.rand(C) + 0.5
        gamma[0] = -0.7
        beta, rm, rv = self.randn(C), self.randn(C) * 0.1, self.rand(C) + 0.5
        if self.mu is not None:
            rm, rv = self.mu + rm * self.sig, rv * self.sig * self.sig
        return gamma, beta, rm, rv


def _out(run, shape, ld, C, prior=None, fill=7.0):
    t = torch.full(tuple(shape) + (ld,), fill, device=_dev())
    if prior is not None:
        t[..., :C] = prior
    return run.d(t)


def _c64(t):
    """NHWC (exactly C channels) -> NCHW float64"""
    return t.double().permute(0, 3, 1, 2)


def _flag(run, label, ok):
    run.res.append((label, None, bool(ok), None, False))


def _exact(run, label, got, ref):
    """bit equality with the float64 reference rounded once to the storage type"""
    _flag(run, label + ' bit-identical', torch.equal(got, ref.to(got.dtype)))


def _f32(run, t):
    return run.d(t, act=False)


def _bn_ws(name, C, ppg, groups):
    """(workspace, bytes) of one BatchNorm launch: EXACTLY what include/pacingpseudo_hip.h asks for that entry point, from the
    query the engine sizes its workspace with -- the statistics and sums passes pp_bn_workspace(C, P_per_group, groups); the
    backward forms with batch statistics 3 * groups * C floats (the k rows of the apply pass) on top; the one-pass eval forms
    pp_bn_workspace(C, P_total, 1); pp_bn_lrelu_bwd_apply 6 * groups * C floats + 16."""
    lib = _L()
    short = name[len('pp_bn_lrelu_bwd'):] if name.startswith('pp_bn_lrelu_bwd') else None
    if short in ('', '_amax', '_pool'):
        n = lib.pp_bn_workspace(C, ppg, groups) + 3 * groups * C * 4
    elif short in ('_eval', '_eval_pool'):
        n = lib.pp_bn_workspace(C, ppg * groups, 1)
    elif short == '_apply':
        n = 6 * groups * C * 4 + 16
    elif short == '_sums' or name in ('pp_bn_train_stats', 'pp_bn_stats_sums'):
        n = lib.pp_bn_workspace(C, ppg, groups)
    else:
        raise KeyError(name)
    return _ws(n), n


def _coef64(z64, gamma, beta, rm, rv, training, eps):
    """(4, groups, C) float64: mean, invstd, scale, shift of z64 (groups, P, C)"""
    G = z64.shape[0]
    if training:
        mean, var = z64.mean(1), z64.var(1, unbiased=False)
    else:
        mean, var = rm.double().expand(G, -1), rv.double().expand(G, -1)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    return torch.stack([mean, invstd, scale, beta.double() - mean * scale])


def _off_kink(ops, z, groups, coef_of, si, hi):
    """(z, coefficient rows) with the few elements moved whose pre-activation z * scale + shift lies within 1e-4 of the LeakyReLU
    kink (by 1/8: at least two steps of either 16-bit grid): there fp32 and float64 may take different branches -- the gradient
    jumps by a factor 1 / slope -- and a 16-bit store flushes y to 0, which no longer tells the branch.  A coarse 16-bit grid
    puts MANY equal values there at once.  The rows are taken again afterwards (they move by ~1e-6, the margin stays)."""
    coef = coef_of(z)
    v = z.reshape(groups, -1, z.shape[-1])
    near = (v * coef[si][:, None] + coef[hi][:, None]).abs() < 1e-4
    near[..., -1] = False                                   # the constant channel stays constant
    z = torch.where(near.reshape(z.shape), ops.r(z + 0.125), z)
    return z, coef_of(z)


def _bn_lrelu64(z, groups, gamma, beta, rm, rv, training, slope, eps=EPS, mom=MOM):
    """leaky_relu(batch_norm(z)) in float64 NCHW, one module call per statistics group, in order (rm / rv updated in place)"""
    per = z.shape[0] // groups
    return torch.cat([F.leaky_relu(F.batch_norm(z[g * per:(g + 1) * per], rm, rv, gamma, beta, training, mom, eps), slope)
                      for g in range(groups)])


# ---------------------------------------------------------------------------------------------------------------- norm: forward
def _bn_stats(key, run):
    """pp_bn_train_stats / pp_bn_stats_sums"""
    _, name, a = key
    ops = _DOps(key)
    if name == 'pp_bn_stats_sums':
        _, ld, C, ppg, groups = a[:5]
        eps, mom = EPS, MOM
    else:
        _, ld, C, ppg, groups, eps, mom = a[:7]
    z = ops.norm_z(groups, ppg, 1, C)
    zd = run.d(ops.pad(z, ld))
    z64 = z.double().reshape(groups, ppg, C)
    ws, nws = _bn_ws(name, C, ppg, groups)
    if name == 'pp_bn_stats_sums':
        sums = _full((groups, 2, C), 7.0, dtype=torch.float64)
        run.K.pp_bn_stats_sums(zd.data_ptr(), ld, C, ppg, groups, sums.data_ptr(), ws.data_ptr(), nws, run.st)
        run.check('sum', sums[:, 0], z64.sum(1), TOL_SUMS, act=False)
        run.check('sum of squares', sums[:, 1], z64.pow(2).sum(1), TOL_SUMS, act=False)
        return
    gamma, beta, rm, rv = ops.affine(C)
    gd, bd, rmd, rvd = (_f32(run, t.clone()) for t in (gamma, beta, rm, rv))
    nbt = _full((), 3, dtype=torch.int64)
    coef = _full((4, groups, C), 7.0)
    run.K.pp_bn_train_stats(zd.data_ptr(), ld, C, ppg, groups, eps, mom, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(),
                            nbt.data_ptr(), *(coef[i].data_ptr() for i in range(4)), ws.data_ptr(), nws, run.st)
    _check_stats(run, z64, gamma, beta, rm, rv, eps, mom, coef, rmd, rvd, nbt)


def _check_stats(run, z64, gamma, beta, rm, rv, eps, mom, coef, rmd, rvd, nbt):
    groups, n, C = z64.shape
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    for g in range(groups):
        F.batch_norm(z64[g].t().reshape(1, C, n, 1), rm64, rv64, gamma.double(), beta.double(), True, mom, eps)
    ref = _coef64(z64, gamma, beta, rm, rv, True, eps)
    for i, lab in enumerate(('save_mean', 'save_invstd', 'scale', 'shift')):
        run.check(lab, coef[i], ref[i], TOL_SUMS, act=False)
    run.check('running_mean', rmd, rm64, TOL_SUMS, act=False)
    run.check('running_var', rvd, rv64, TOL_SUMS, act=False)
    _varying_rows(run, ('save_invstd', 'scale', 'shift'), coef[1:], ref[1:], C)
    _flag(run, 'num_batches_tracked', int(nbt) == 3 + groups)
    # the constant channel: its sums are exact, the variance must be exactly 0
    want = 1.0 / math.sqrt(torch.tensor(eps).float().item())
    const = float(z64[0, 0, C - 1])                    # 0.5, times a power of two under a NormProfile
    _flag(run, 'constant channel: mean 0.5, variance exactly 0', bool((coef[0, :, C - 1] == const).all())
          and float((coef[1, :, C - 1].double() - want).abs().max()) <= 5e-7 * want)          # fp32 rounding of 1 / sqrt(eps)
    return ref


def _varying_rows(run, labels, got, ref, C):
    """Under a NormProfile the rows once more without the constant channel: its invstd = 1 / sqrt(eps) ~ 316 is the maximum the
    whole row is relative to, which would hide the cancellation error of the varying channels a hundred times over."""
    if _NORM_PROFILE[0] != NORM_CENSUS and C > 1:
        for i, lab in enumerate(labels):
            run.check(lab + ' of the varying channels', got[i][..., :C - 1], ref[i][..., :C - 1], TOL_SUMS, act=False)


def _bn_finalize(key, run):
    """pp_bn_train_finalize[_lazy]: the partial rows are real ones (float64 sums of a z split into `rows` chunks per group)"""
    _, name, a = key
    _, rows, C, n, groups, eps, mom = a[:7]
    lazy = name.endswith('_lazy')
    ops = _DOps(key)
    z64 = ops.norm_z(groups, n, 1, C).double().reshape(groups, n, C)
    part = _zeros(groups, rows, 2, C, dtype=torch.float64)
    for r, chunk in enumerate(torch.tensor_split(z64, rows, dim=1)):
        part[:, r, 0], part[:, r, 1] = chunk.sum(1), chunk.pow(2).sum(1)
    gamma, beta, rm, rv = ops.affine(C)
    gd, bd, rmd, rvd = (_f32(run, t.clone()) for t in (gamma, beta, rm, rv))
    nbt = _full((), 3, dtype=torch.int64)
    coef = _full((4, groups, C), 7.0)
    args = (part.data_ptr(), rows, C, n, groups, eps, mom, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(),
            nbt.data_ptr(), *(coef[i].data_ptr() for i in range(4)))
    if lazy:
        lld, slope = a[17], a[18]
        lz = _full((groups, 3, lld), 7.0)
        run.K.pp_bn_train_finalize_lazy(*args, lz.data_ptr(), lld, slope, run.st)
    else:
        run.K.pp_bn_train_finalize(*args, run.st)
    ref = _check_stats(run, z64, gamma, beta, rm, rv, eps, mom, coef, rmd, rvd, nbt)
    if lazy:
        run.check('lazy scale row', lz[:, 0, :C], ref[2], TOL_SUMS, act=False)
        run.check('lazy shift row', lz[:, 1, :C], ref[3], TOL_SUMS, act=False)
        _flag(run, 'lazy slope row', bool((lz[:, 2, :C] == torch.tensor(slope, device=_dev()).float()).all()))
        run.canary('lazy rows', lz, C)


def _bn_eval_coeffs(key, run):
    """pp_bn_eval_coeffs"""
    _, _, a = key
    C, groups, eps = a[:3]
    ops = _DOps(key)
    gamma, beta, rm, rv = ops.affine(C)
    gd, bd, rmd, rvd = (_f32(run, t) for t in (gamma, beta, rm, rv))
    coef = _full((4, groups, C), 7.0)
    run.K.pp_bn_eval_coeffs(C, groups, eps, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(),
                            *(coef[i].data_ptr() for i in range(4)), run.st)
    ref = _coef64(torch.zeros(groups, 1, C, dtype=torch.float64, device=_dev()), gamma, beta, rm, rv, False, eps)
    for i, lab in enumerate(('save_mean', 'save_invstd', 'scale', 'shift')):
        run.check(lab, coef[i], ref[i], TOL_SUMS, act=False)


def _bn_eval_coeffs_batch(key, run):
    """pp_bn_eval_coeffs_batch: n layers in one launch (the item table is a host array the launch shape does not show: layers of
    every width class of col_plan, one and two groups); every row against float64 and, as include/pacingpseudo_hip.h promises,
    bit for bit against pp_bn_eval_coeffs of that layer."""
    _, _, a = key
    _, n, eps = a[:3]
    from pacingpseudo_amd._lib import PpBnCoefItem
    lib = _L()
    ops = _DOps(key)
    widths = (32, 64, 128, 256, 512, 1024, 12, 516)
    items, layers = [], []
    for i in range(n):
        C, groups = widths[i % len(widths)], 1 + (i // len(widths) + i) % 2
        par = ops.affine(C)
        dev = [_f32(run, t) for t in par]
        coef = _f32(run, torch.full((4, groups, C), 7.0, device=_dev()))
        items.append(PpBnCoefItem(C, groups, *(t.data_ptr() for t in dev), *(coef[j].data_ptr() for j in range(4))))
        layers.append((C, groups, par, dev, coef))
    arr = (PpBnCoefItem * n)(*items)
    run.keep.append(arr)
    run.K.pp_bn_eval_coeffs_batch(arr, n, eps, run.st)
    same = True
    for i, (C, groups, par, dev, coef) in enumerate(layers):
        ref = _coef64(torch.zeros(groups, 1, C, dtype=torch.float64, device=_dev()), *par, False, eps)
        for j, lab in enumerate(('save_mean', 'save_invstd', 'scale', 'shift')):
            run.check(f'layer {i} (C={C}, groups={groups}) {lab}', coef[j], ref[j], TOL_SUMS, act=False)
        one = _full((4, groups, C), 7.0)
        lib.pp_bn_eval_coeffs(C, groups, eps, *(t.data_ptr() for t in dev), *(one[j].data_ptr() for j in range(4)), run.st)
        same = same and torch.equal(one, coef)
    _flag(run, 'rows bit-identical to pp_bn_eval_coeffs', same)


def _bn_fwd(key, run):
    """pp_bn_lrelu_fwd / pp_bn_lrelu_fwd_pool (BatchNorm: one coefficient row per group; GroupNorm: one per image)"""
    _, name, a = key
    pool = name.endswith('_pool')
    if pool:
        _, ld_z, _, _, _, ld_y, _, ld_p, C, N, H, W, groups, slope = a[:14]
    else:
        _, ld_z, _, _, _, ld_y, C, ppg, groups, slope = a[:10]
        N, H, W = groups, ppg, 1
    ops = _DOps(key)
    z = ops.norm_z(N, H, W, C)
    zd = run.d(ops.pad(z, ld_z))
    scale = ops.rand(groups, C) + 0.5
    scale[:, 0] = -0.7
    shift = ops.randn(groups, C)
    if ops.mu is not None:          # NormProfile: rows of a normalisation, shift = beta - mean * scale, so z * scale + shift cancels
        scale = scale / ops.sig
        shift = shift - ops.mu * scale
    sd, hd = _f32(run, scale), _f32(run, shift)
    y = _out(run, (N, H, W), ld_y, C)
    if pool:
        pooled = _out(run, (N, H // 2, W // 2), ld_p, C)
        run.K.pp_bn_lrelu_fwd_pool(zd.data_ptr(), ld_z, sd.data_ptr(), hd.data_ptr(), y.data_ptr(), ld_y, pooled.data_ptr(), ld_p, C, N, H,
                                   W, groups, slope, run.st)
    else:
        run.K.pp_bn_lrelu_fwd(zd.data_ptr(), ld_z, sd.data_ptr(), hd.data_ptr(), y.data_ptr(), ld_y, C, ppg, groups, slope, run.st)
    per = N // groups
    pre = z.double().reshape(groups, per * H * W, C) * scale.double()[:, None] + shift.double()[:, None]
    ref = torch.where(pre > 0, pre, pre * slope).reshape(N, H, W, C)
    run.check('y', y[..., :C], ref)
    run.canary('y', y, C)
    if pool:
        run.check('pooled', pooled[..., :C], F.max_pool2d(_c64(ref), 2, 2).permute(0, 2, 3, 1))
        run.canary('pooled', pooled, C)


# --------------------------------------------------------------------------------------------------------------- norm: backward
def _param_grads(run, ops, C, acc, have):
    """dgamma, dbeta, dbias_conv buffers (null where the recorded launch passed null) and their prior content"""
    prior = ops.randn(3, C, scale=ops.gs)
    bufs = [(_f32(run, prior[i].clone() if acc else torch.full((C,), 9.0, device=_dev())) if h else None) for i, h in enumerate(have)]
    return bufs, prior


def _check_bwd(run, storage, C, dz, z_grad, dzabs, bufs, prior, acc, refs, am):
    """dz (N, H, W, ld) against z_grad NCHW float64; parameter gradients; the conv-bias gradient relative to sum |dz| per channel
    (test_bn_lrelu: in train mode the sum itself is 0); amax == max |dz| of the stored tensor although it started larger."""
    run.check('dz', dz[..., :C], z_grad.permute(0, 2, 3, 1))
    run.canary('dz', dz, C)
    for i, lab in enumerate(('dgamma', 'dbeta')):
        if bufs[i] is not None:
            run.res.append((lab, bufs[i], refs[i] + (prior[i].double() if acc else 0), TOL, False))
    if bufs[2] is not None:
        mag = torch.full((C,), float(dzabs.max()) + float(prior[2].abs().max() if acc else 0), dtype=torch.float64, device=_dev())
        run.res.append(('dbias_conv', bufs[2].double() - (refs[2] + (prior[2].double() if acc else 0)) + mag, mag, TOL, False))
    if am is not None:
        stored = dz[..., :C].float().abs().max()
        if dz.dtype == torch.float32:          # (the fp32 twin of a 16-bit key stores fp32 too)
            _flag(run, 'dz_amax == max |dz| (stale larger value cleared)', torch.equal(am.reshape(()), stored))
        else:
            _flag(run, 'dz_amax == max |dz| (stale larger value cleared)',
                  abs(float(am) - float(stored)) <= 2.0 ** -(MANT[storage][0] + 1) * float(stored))


def _bn_bwd(key, run):
    """pp_bn_lrelu_bwd / _amax / _pool / _apply (statistics of the batch, or training = 0) and _eval / _eval_pool (from y alone)"""
    storage, name, a = key
    short = name[len('pp_bn_lrelu_bwd'):]
    ev, pool = short.startswith('_eval'), short.endswith('_pool')
    if short in ('', '_amax'):
        (_, ld_dy, _, ld_z, _, _, _, _, _, training, _, ld_dz, dgp, dbp, dcp, acc, C, ppg, groups, slope) = a[:20]
        amp = a[22] if short == '_amax' else None
    elif short == '_apply':
        (_, ld_dy, _, ld_z, _, _, _, _, _, training, _, _, n_glob, _, ld_dz, dgp, dbp, dcp, acc, C, ppg, groups, slope) = a[:23]
        amp = a[25]
        if n_glob != ppg:
            raise KeyError(f'{name} with n_global != P_per_group (no one-rank reference)')
    elif short == '_pool':
        (_, ld_dy, _, ld_dp, _, ld_z, _, _, _, _, _, training, _, ld_dz, dgp, dbp, dcp, acc, C, N, H, W, groups, slope) = a[:24]
        amp = a[26]
    elif short == '_eval':
        (_, ld_dy, _, ld_z, _, _, _, _, ld_dz, dgp, dbp, dcp, acc, C, ppg, slope) = a[:16]
        groups, training, amp = 1, 0, a[18]
    elif short == '_eval_pool':
        (_, ld_dy, _, ld_dp, _, ld_z, _, _, _, _, ld_dz, dgp, dbp, dcp, acc, C, N, H, W, slope) = a[:20]
        groups, training, amp = 1, 0, a[22]
    else:
        raise KeyError(name)
    if not pool:
        N, H, W = groups, ppg, 1
    ppg = (N // groups) * H * W
    ops = _DOps(key)
    z = ops.norm_z(N, H, W, C, grid=2.0 ** -10 if pool else None)
    gamma, beta, rm, rv = ops.affine(C)
    z, coef = _off_kink(ops, z, groups, lambda t: _coef64(t.double().reshape(groups, ppg, C), gamma, beta, rm, rv, bool(training),
                                                          EPS).float(), 2, 3)
    if ev:      # the one-pass eval forms read the stored output y = lrelu(z * scale + shift); the reference differentiates the
        #         float64 network whose output IS that stored y (z recovered from it)
        pre = z.reshape(groups, ppg, C) * coef[2][:, None] + coef[3][:, None]
        ysto = ops.r(torch.where(pre > 0, pre, pre * slope)).reshape(N, H, W, C)
        y64 = ysto.double()
        pre64 = torch.where(y64 > 0, y64, y64 / slope)
        z64 = (pre64 - beta.double()) / gamma.double() * torch.sqrt(rv.double() + EPS) + rm.double()
        src = run.d(ops.pad(ysto, ld_z))
    else:
        z64 = z.double()
        src = run.d(ops.pad(z, ld_z))
    dy = ops.r(ops.randn(N, H, W, C, scale=ops.gs))
    dyd = run.d(ops.pad(dy, ld_dy))
    if pool:
        dp = ops.r(ops.randn(N, H // 2, W // 2, C, scale=ops.gs))
        dpd = run.d(ops.pad(dp, ld_dp))
    # float64 reference: autograd through one module call per statistics group
    zr = _c64(z64).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = _bn_lrelu64(zr, groups, gr, br, rm.double().clone(), rv.double().clone(), bool(training), slope)
    loss = (yr * _c64(dy)).sum()
    if pool:
        loss = loss + (F.max_pool2d(yr, 2, 2) * _c64(dp)).sum()
    loss.backward()
    refs = (gr.grad, br.grad, zr.grad.sum((0, 2, 3)))
    dzabs = zr.grad.abs().sum((0, 2, 3))
    cd = _f32(run, coef)
    mean, invstd, scale, shift = (cd[i].data_ptr() for i in range(4))
    gd, bd = _f32(run, gamma), _f32(run, beta)
    bufs, prior = _param_grads(run, ops, C, acc, (dgp, dbp, dcp))
    dz = _out(run, (N, H, W), ld_dz, C)
    am = _full((1,), 1e30) if amp else None
    ws, nws = _bn_ws(name, C, ppg, groups)
    K, st = run.K, run.st
    tail = (dz.data_ptr(), ld_dz, _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), acc, C)
    if short == '':
        K.pp_bn_lrelu_bwd(dyd.data_ptr(), ld_dy, src.data_ptr(), ld_z, scale, shift, mean, invstd, gd.data_ptr(), training, *tail, ppg, groups,
                          slope, ws.data_ptr(), nws, st)
    elif short == '_amax':
        K.pp_bn_lrelu_bwd_amax(dyd.data_ptr(), ld_dy, src.data_ptr(), ld_z, scale, shift, mean, invstd, gd.data_ptr(), training, *tail, ppg,
                               groups, slope, ws.data_ptr(), nws, _p(am), st)
    elif short == '_apply':
        # local = global sums (one rank), given in float64: (sum g, sum g * xhat) per group and channel
        s64 = _b(_bwd_sums64(z64.reshape(groups, ppg, C), dy.double().reshape(groups, ppg, C), coef.double(), slope))
        K.pp_bn_lrelu_bwd_apply(dyd.data_ptr(), ld_dy, src.data_ptr(), ld_z, scale, shift, mean, invstd, gd.data_ptr(), training,
                                s64.data_ptr(), s64.data_ptr(), n_glob, *tail, ppg, groups, slope, ws.data_ptr(), nws, _p(am), st)
    elif short == '_pool':
        K.pp_bn_lrelu_bwd_pool(dyd.data_ptr(), ld_dy, dpd.data_ptr(), ld_dp, src.data_ptr(), ld_z, scale, shift, mean, invstd, gd.data_ptr(),
                               training, *tail, N, H, W, groups, slope, ws.data_ptr(), nws, _p(am), st)
    elif short == '_eval':
        K.pp_bn_lrelu_bwd_eval(dyd.data_ptr(), ld_dy, src.data_ptr(), ld_z, scale, gd.data_ptr(), bd.data_ptr(), *tail, ppg, slope,
                               ws.data_ptr(), nws, _p(am), st)
    else:
        K.pp_bn_lrelu_bwd_eval_pool(dyd.data_ptr(), ld_dy, dpd.data_ptr(), ld_dp, src.data_ptr(), ld_z, scale, gd.data_ptr(), bd.data_ptr(),
                                    *tail, N, H, W, slope, ws.data_ptr(), nws, _p(am), st)
    _check_bwd(run, storage, C, dz, zr.grad, dzabs, bufs, prior, acc, refs, am)


def _bwd_sums64(z64, dy64, coef64, slope):
    """(groups, 2, C) float64: sum g, sum g * xhat with g = dy * lrelu'(z * scale + shift), xhat = (z - mean) * invstd"""
    mean, invstd, scale, shift = (coef64[i][:, None] for i in range(4))
    g = dy64 * torch.where(z64 * scale + shift > 0, 1.0, slope)
    return torch.stack([g.sum(1), (g * (z64 - mean) * invstd).sum(1)], 1).contiguous()


def _bn_bwd_sums(key, run):
    """pp_bn_lrelu_bwd_sums (the local half of the synchronised backward)"""
    _, name, a = key
    _, ld_dy, _, ld_z, _, _, _, _, C, ppg, groups, slope = a[:12]
    ops = _DOps(key)
    z = ops.norm_z(groups, ppg, 1, C)
    gamma, beta, rm, rv = ops.affine(C)
    z, coef = _off_kink(ops, z, groups, lambda t: _coef64(t.double().reshape(groups, ppg, C), gamma, beta, rm, rv, True, EPS).float(), 2, 3)
    dy = ops.r(ops.randn(groups, ppg, 1, C, scale=ops.gs))
    zd, dyd, cd = run.d(ops.pad(z, ld_z)), run.d(ops.pad(dy, ld_dy)), _f32(run, coef)
    sums = _full((groups, 2, C), 7.0, dtype=torch.float64)
    ws, nws = _bn_ws(name, C, ppg, groups)
    run.K.pp_bn_lrelu_bwd_sums(dyd.data_ptr(), ld_dy, zd.data_ptr(), ld_z, cd[2].data_ptr(), cd[3].data_ptr(), cd[0].data_ptr(),
                               cd[1].data_ptr(), C, ppg, groups, slope, sums.data_ptr(), ws.data_ptr(), nws, run.st)
    ref = _bwd_sums64(z.double().reshape(groups, ppg, C), dy.double().reshape(groups, ppg, C), coef.double(), slope)
    for i, lab in enumerate(('sum g', 'sum g xhat')):
        run.check(lab, sums[:, i], ref[:, i], TOL_SUMS, act=False)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _gn_rows64(z64, G, gamma, beta, eps):
    """(5, N, C) float64 rows of pp_gn_stats: mean, invstd, xbar, scale, shift; z64 (N, HW, C)"""
    N, HW, C = z64.shape
    zg = z64.reshape(N, HW, G, C // G)
    mean = zg.mean((1, 3), keepdim=True)
    var = zg.var((1, 3), unbiased=False, keepdim=True)
    invstd = 1.0 / torch.sqrt(var + eps)
    xbar = ((zg - mean) * invstd).mean(1).reshape(N, C)
    mean, invstd = (t.expand(N, 1, G, C // G).reshape(N, C) for t in (mean, invstd))
    scale = gamma.double() * invstd
    return torch.stack([mean, invstd, xbar, scale, beta.double() - mean * scale])


def _gn_stats(key, run):
    """pp_gn_stats"""
    _, _, a = key
    _, ld, C, HW, N, G, eps = a[:7]
    lib = _L()
    ops = _DOps(key)
    z = ops.norm_z(N, HW, 1, C)
    gamma, beta, _, _ = ops.affine(C)
    zd, gd, bd = run.d(ops.pad(z, ld)), _f32(run, gamma), _f32(run, beta)
    rows = _full((5, N, C), 7.0)
    nws = lib.pp_gn_workspace(C, HW, N)
    ws = _ws(nws)
    run.K.pp_gn_stats(zd.data_ptr(), ld, C, HW, N, G, eps, gd.data_ptr(), bd.data_ptr(), *(rows[i].data_ptr() for i in range(5)),
                      ws.data_ptr(), nws, run.st)
    ref = _gn_rows64(z.double().reshape(N, HW, C), G, gamma, beta, eps)
    for i, lab in enumerate(('save_mean', 'save_invstd', 'save_xbar', 'scale', 'shift')):
        run.check(lab, rows[i], ref[i], TOL_SUMS, act=False)
    _varying_rows(run, ('save_invstd', 'scale', 'shift'), (rows[1], rows[3], rows[4]), (ref[1], ref[3], ref[4]), C)


def _gn_bwd(key, run):
    """pp_gn_lrelu_bwd / pp_gn_lrelu_bwd_pool"""
    storage, name, a = key
    pool = name.endswith('_pool')
    if pool:
        (_, ld_dy, _, ld_dp, _, ld_z, _, _, _, _, _, _, _, ld_dz, dgp, dbp, dcp, acc, C, N, H, W, G, slope) = a[:24]
        amp = a[26]
    else:
        (_, ld_dy, _, ld_z, _, _, _, _, _, _, _, ld_dz, dgp, dbp, dcp, acc, C, HW, N, G, slope) = a[:21]
        H, W, amp = HW, 1, a[23]
    lib = _L()
    ops = _DOps(key)
    z = ops.norm_z(N, H, W, C, grid=2.0 ** -10 if pool else None)
    gamma, beta, _, _ = ops.affine(C)
    eps = 1e-5
    z, rows = _off_kink(ops, z, N, lambda t: _gn_rows64(t.double().reshape(N, H * W, C), G, gamma, beta, eps).float(), 3, 4)
    dy = ops.r(ops.randn(N, H, W, C, scale=ops.gs))
    zd, dyd, rd, gd = run.d(ops.pad(z, ld_z)), run.d(ops.pad(dy, ld_dy)), _f32(run, rows), _f32(run, gamma)
    if pool:
        dp = ops.r(ops.randn(N, H // 2, W // 2, C, scale=ops.gs))
        dpd = run.d(ops.pad(dp, ld_dp))
    zr = _c64(z).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = F.leaky_relu(F.group_norm(zr, G, gr, br, eps), slope)
    loss = (yr * _c64(dy)).sum()
    if pool:
        loss = loss + (F.max_pool2d(yr, 2, 2) * _c64(dp)).sum()
    loss.backward()
    refs = (gr.grad, br.grad, zr.grad.sum((0, 2, 3)))
    bufs, prior = _param_grads(run, ops, C, acc, (dgp, dbp, dcp))
    dz = _out(run, (N, H, W), ld_dz, C)
    am = _full((1,), 1e30) if amp else None
    nws = lib.pp_gn_workspace(C, H * W, N)
    ws = _ws(nws)
    mean, invstd, xbar, scale, shift = (rd[i].data_ptr() for i in range(5))
    tail = (dz.data_ptr(), ld_dz, _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), acc, C)
    if pool:
        run.K.pp_gn_lrelu_bwd_pool(dyd.data_ptr(), ld_dy, dpd.data_ptr(), ld_dp, zd.data_ptr(), ld_z, scale, shift, mean, invstd, xbar,
                                   gd.data_ptr(), *tail, N, H, W, G, slope, ws.data_ptr(), nws, _p(am), run.st)
    else:
        run.K.pp_gn_lrelu_bwd(dyd.data_ptr(), ld_dy, zd.data_ptr(), ld_z, scale, shift, mean, invstd, xbar, gd.data_ptr(), *tail, H * W, N, G,
                              slope, ws.data_ptr(), nws, _p(am), run.st)
    _check_bwd(run, storage, C, dz, zr.grad, zr.grad.abs().sum((0, 2, 3)), bufs, prior, acc, refs, am)


def _lazy_materialize(key, run):
    """pp_lazy_materialize"""
    _, _, a = key
    _, ld_s, lz, _, ld_d, C, B, HW = a[:8]
    from pacingpseudo_amd._lib import PpLazyIn
    ops = _DOps(key)
    x = ops.act(B, HW, 1, ld_s, C)
    coef = ops.lazy(lz, C).to(_dev())
    cd = _f32(run, coef)
    st = PpLazyIn(cd.data_ptr(), lz[1], lz[2])
    run.keep.append(st)
    y = _out(run, (B, HW, 1), ld_d, C)
    run.K.pp_lazy_materialize(run.d(x).data_ptr(), ld_s, ctypes.byref(st), y.data_ptr(), ld_d, C, B, HW, run.st)
    run.check('y', y[..., :C], _lazy64(x, coef, lz[2], C))
    run.canary('y', y, C)


# -------------------------------------------------------------------------------------------------------------------- spatial
def _stride2(key, run):
    """pp_stride2_gather / pp_stride2_scatter (fp32 storage only)"""
    _, name, a = key
    _, ld_a, _, ld_b, C, N, Ho, Wo = a[:8]
    ops = _DOps(key)
    if name == 'pp_stride2_gather':
        full = ops.act(N, 2 * Ho, 2 * Wo, ld_a, C)
        out = _out(run, (N, Ho, Wo), ld_b, C)
        run.K.pp_stride2_gather(run.d(full).data_ptr(), ld_a, out.data_ptr(), ld_b, C, N, Ho, Wo, run.st)
        _exact(run, 'out', out[..., :C], full[:, ::2, ::2, :C])
        run.canary('out', out, C)
        return
    dz = ops.act(N, Ho, Wo, ld_a, C, ops.gs)
    full = _out(run, (N, 2 * Ho, 2 * Wo), ld_b, C)
    run.K.pp_stride2_scatter(run.d(dz).data_ptr(), ld_a, full.data_ptr(), ld_b, C, N, Ho, Wo, run.st)
    ref = torch.zeros(N, 2 * Ho, 2 * Wo, C, device=_dev())
    ref[:, ::2, ::2] = dz[..., :C]
    _exact(run, 'full', full[..., :C], ref)
    run.canary('full', full, C)


def _maxpool(key, run):
    """pp_maxpool2_fwd / pp_maxpool2_bwd: bit for bit (one fp32 addition per element when accumulating)"""
    storage, name, a = key
    ops = _DOps(key)
    if name == 'pp_maxpool2_fwd':
        _, ld_x, _, ld_y, C, N, H, W = a[:8]
    else:
        _, ld_x, _, ld_dy, _, ld_dx, C, N, H, W, acc = a[:11]
    x = ops.act(N, H, W, ld_x, C)
    x[0, 0, 0, :C] = x[0, 0, 1, :C] = 4.0                     # ties: the first maximum takes the gradient
    x[0, 1, 0, 0] = 4.0
    xr = _c64(x[..., :C]).requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    if name == 'pp_maxpool2_fwd':
        y = _out(run, (N, H // 2, W // 2), ld_y, C)
        run.K.pp_maxpool2_fwd(run.d(x).data_ptr(), ld_x, y.data_ptr(), ld_y, C, N, H, W, run.st)
        _exact(run, 'y', y[..., :C], yr.detach().permute(0, 2, 3, 1))
        run.canary('y', y, C)
        return
    dy = ops.act(N, H // 2, W // 2, ld_dy, C, ops.gs)
    prior = ops.r(ops.randn(N, H, W, C, scale=ops.gs)) if acc else None
    dx = _out(run, (N, H, W), ld_dx, C, prior)
    run.K.pp_maxpool2_bwd(run.d(x).data_ptr(), ld_x, run.d(dy).data_ptr(), ld_dy, dx.data_ptr(), ld_dx, C, N, H, W, acc, run.st)
    yr.backward(_c64(dy[..., :C]))
    ref = xr.grad.permute(0, 2, 3, 1) + (prior.double() if acc else 0)
    run.check('dx', dx[..., :C], ref)
    if storage == 'fp32' or not acc:
        _exact(run, 'dx', dx[..., :C], ref)
    run.canary('dx', dx, C)


def _bilinear(key, run):
    """pp_bilinear_fwd / pp_bilinear_bwd (align_corners = True); scale 1 is an exact copy"""
    storage, name, a = key
    ops = _DOps(key)
    if name == 'pp_bilinear_fwd':
        _, ld_x, _, ld_y, C, N, Hi, Wi, Ho, Wo = a[:10]
        x = ops.act(N, Hi, Wi, ld_x, C)
        y = _out(run, (N, Ho, Wo), ld_y, C)
        run.K.pp_bilinear_fwd(run.d(x).data_ptr(), ld_x, y.data_ptr(), ld_y, C, N, Hi, Wi, Ho, Wo, run.st)
        ref = F.interpolate(_c64(x[..., :C]), size=(Ho, Wo), mode='bilinear', align_corners=True).permute(0, 2, 3, 1)
        run.check('y', y[..., :C], ref, TOL_BIL)
        if (Hi, Wi) == (Ho, Wo):
            _exact(run, 'y (scale 1)', y[..., :C], x[..., :C])
        run.canary('y', y, C)
        return
    _, ld_dy, _, ld_dx, C, N, Hi, Wi, Ho, Wo, acc = a[:11]
    dy = ops.act(N, Ho, Wo, ld_dy, C, ops.gs)
    prior = ops.r(ops.randn(N, Hi, Wi, C, scale=ops.gs)) if acc else None
    dx = _out(run, (N, Hi, Wi), ld_dx, C, prior)
    run.K.pp_bilinear_bwd(run.d(dy).data_ptr(), ld_dy, dx.data_ptr(), ld_dx, C, N, Hi, Wi, Ho, Wo, acc, run.st)
    xr = torch.zeros(N, C, Hi, Wi, dtype=torch.float64, device=_dev(), requires_grad=True)
    F.interpolate(xr, size=(Ho, Wo), mode='bilinear', align_corners=True).backward(_c64(dy[..., :C]))
    ref = xr.grad.permute(0, 2, 3, 1) + (prior.double() if acc else 0)
    run.check('dx', dx[..., :C], ref, TOL_BIL)
    if (Hi, Wi) == (Ho, Wo) and (storage == 'fp32' or not acc):
        _exact(run, 'dx (scale 1)', dx[..., :C], ref)
    if Ho < Hi and Wo < Wi:       # inputs no output touches: exactly 0, or exactly the prior content
        untouched = xr.grad.permute(0, 2, 3, 1) == 0
        want = prior if acc else torch.zeros(N, Hi, Wi, C, device=_dev())
        _flag(run, 'dx of untouched inputs unchanged', torch.equal(dx[..., :C].float()[untouched], want[untouched]))
    run.canary('dx', dx, C)


def _copy_slab(key, run):
    """pp_copy_slab"""
    storage, _, a = key
    _, ld_x, _, ld_y, C, P, acc = a[:7]
    ops = _DOps(key)
    x = ops.act(1, P, 1, ld_x, C)
    prior = ops.r(ops.randn(1, P, 1, C)) if acc else None
    y = _out(run, (1, P, 1), ld_y, C, prior)
    run.K.pp_copy_slab(run.d(x).data_ptr(), ld_x, y.data_ptr(), ld_y, C, P, acc, run.st)
    ref = x[..., :C].double() + (prior.double() if acc else 0)
    run.check('y', y[..., :C], ref)
    if storage == 'fp32' or not acc:
        _exact(run, 'y', y[..., :C], ref)
    run.canary('y', y, C)


def _channel_scale(key, run):
    """pp_channel_scale (Dropout2d masks: 0 or 1 / (1 - p) per sample and channel)"""
    _, _, a = key
    _, ld_x, _, ld_y, _, C, N, HW, acc = a[:9]
    ops = _DOps(key)
    x = ops.act(N, HW, 1, ld_x, C)
    scale = (ops.rand(N, C) > 0.3).float() * (ops.rand(N, C) + 1.0)
    prior = ops.r(ops.randn(N, HW, 1, C)) if acc else None
    y = _out(run, (N, HW, 1), ld_y, C, prior)
    run.K.pp_channel_scale(run.d(x).data_ptr(), ld_x, y.data_ptr(), ld_y, _f32(run, scale).data_ptr(), C, N, HW, acc, run.st)
    ref = x[..., :C].double() * scale.double()[:, None, None] + (prior.double() if acc else 0)
    run.check('y', y[..., :C], ref)
    run.canary('y', y, C)


def _pack_image(key, run):
    """pp_pack_image_nchw_to_nhwc: channels [C, Cpad) are zero-filled"""
    _, _, a = key
    _, N, C, H, W, _, ld, Cpad = a[:8]
    ops = _DOps(key)
    src = ops.r(ops.randn(N, C, H, W))
    dst = _out(run, (N, H, W), ld, Cpad)
    run.K.pp_pack_image_nchw_to_nhwc(_f32(run, src).data_ptr(), N, C, H, W, dst.data_ptr(), ld, Cpad, run.st)
    ref = torch.zeros(N, H, W, Cpad, device=_dev())
    ref[..., :C] = src.permute(0, 2, 3, 1)
    _exact(run, 'dst', dst[..., :Cpad], ref)
    run.canary('dst', dst, Cpad)


def _pack_weights(key, run):
    """pp_pack_conv3x3_weights / pp_wino_pack_weights (the layers outside the batched split-fp16 packs): the packs are opaque
    layouts, so they are checked by what they are for -- the forward and the data-gradient kernels fed with them, on a small
    image of the geometry that selects the recorded Winograd tile."""
    _, name, a = key
    lib = _L()
    ops = _DOps(key)
    _, O_, I = a[:3]
    wb_given = a[5] is not None
    w = _f32(run, ops.randn(O_, I, 3, 3, scale=1 / math.sqrt(9 * I)))
    if name == 'pp_wino_pack_weights':
        tile = a[3]
        geo = next(g for g in ((1, 16, 16, 1), (1, 6, 10, 1), (1, 28, 28, 2)) if lib.pp_conv3x3_wino_tile(*g[1:]) == tile)
        B, H, W, dil = geo
        n = (tile + 2) ** 2
        wf, wb = _zeros(n, O_, I), (_zeros(n, I, O_) if wb_given else None)
        run.K.pp_wino_pack_weights(w.data_ptr(), O_, I, tile, wf.data_ptr(), _p(wb), run.st)
        Ipad = I
    else:
        Ipad = a[3]
        B, H, W, dil = 1, 8, 8, 1
        wf, wb = _zeros(O_, 9, Ipad), (_zeros(Ipad, 9, O_) if wb_given else None)
        run.K.pp_pack_conv3x3_weights(w.data_ptr(), O_, I, Ipad, wf.data_ptr(), _p(wb), run.st)
    x = ops.randn(B, H, W, Ipad)
    x[..., I:] = 0
    x, dz = _b(x), _b(ops.randn(B, H, W, O_))
    y, dx = _empty(B, H, W, O_), _empty(B, H, W, Ipad)
    if name == 'pp_wino_pack_weights':
        nws = lib.pp_conv3x3_wino_workspace(I, O_, B, H, W, dil)                 # each launch its own, exact workspace
        lib.pp_conv3x3_wino_fwd(x.data_ptr(), Ipad, I, wf.data_ptr(), None, y.data_ptr(), O_, O_, B, H, W, dil, 0, None,
                                _ws(nws).data_ptr(), nws, run.st)
        if wb_given:
            nws = lib.pp_conv3x3_wino_workspace(O_, I, B, H, W, dil)
            lib.pp_conv3x3_wino_bwd_data(dz.data_ptr(), O_, O_, wb.data_ptr(), dx.data_ptr(), Ipad, I, B, H, W, dil, 0,
                                         _ws(nws).data_ptr(), nws, run.st)
    else:
        lib.pp_conv3x3_fwd(x.data_ptr(), Ipad, Ipad, wf.data_ptr(), None, y.data_ptr(), O_, O_, B, H, W, dil, 0, run.st)
        if wb_given:
            lib.pp_conv3x3_bwd_data(dz.data_ptr(), O_, O_, wb.data_ptr(), dx.data_ptr(), Ipad, Ipad, B, H, W, dil, 0, run.st)
    with torch.backends.cudnn.flags(enabled=False):
        run.check('forward through the pack', y, F.conv2d(_c64(x[..., :I]), w.double(), None, 1, dil, dil).permute(0, 2, 3, 1), act=False)
        if wb_given:
            ref = torch.nn.grad.conv2d_input((B, I, H, W), w.double(), _c64(dz), 1, dil, dil).permute(0, 2, 3, 1)
            run.check('data gradient through the pack', dx[..., :I], ref, act=False)


def _pack_batch(key, run):
    """pp_pack_conv3x3_weights_f16x3_batch / pp_wino_pack_weights_f16x3_batch: n layers in one launch (a host item table; the
    launch shape shows only n).  The per-layer packs are what the convolution census feeds its kernels with, so the batch is
    held to them bit for bit, layer by layer, over layer shapes of several sizes."""
    _, name, a = key
    n = a[1]
    from pacingpseudo_amd._lib import PpPackItem, PpWinoPackItem
    lib = _L()
    ops = _DOps(key)
    wino = name.startswith('pp_wino')
    shapes = ((32, 32), (64, 32), (16, 64), (128, 16), (16, 128), (256, 64), (48, 80), (512, 256))
    items, layers = [], []
    for i in range(n):
        O_, I = shapes[i % len(shapes)]
        w = _f32(run, ops.randn(O_, I, 3, 3, scale=1 / math.sqrt(9 * I)))
        planes = 36 if wino else 9
        bufs = [_zeros(d) for d in (((planes, O_, I), (planes, I, O_)) if wino else ((O_, planes, I), (I, planes, O_)))
                for _ in range(2)]                      # wf, wf', wb, wb'
        items.append(PpWinoPackItem(w.data_ptr(), O_, I, bufs[0].data_ptr(), bufs[2].data_ptr()) if wino else
                     PpPackItem(w.data_ptr(), O_, I, I, bufs[0].data_ptr(), bufs[2].data_ptr()))
        layers.append((w, O_, I, bufs))
    arr = ((PpWinoPackItem if wino else PpPackItem) * n)(*items)
    run.keep.append(arr)
    getattr(run.K, name)(arr, n, run.st)
    same = True
    for w, O_, I, bufs in layers:
        if wino:
            lib.pp_wino_pack_weights_f16x3(w.data_ptr(), O_, I, 4, bufs[1].data_ptr(), bufs[3].data_ptr(), run.st)
        else:
            lib.pp_pack_conv3x3_weights_f16x3(w.data_ptr(), O_, I, I, bufs[1].data_ptr(), bufs[3].data_ptr(), run.st)
        same = same and torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[2], bufs[3]) and bool(bufs[0].abs().sum() > 0)
    _flag(run, 'packs bit-identical to the per-layer entry point', same)


def _scale(key, run):
    """pp_scale / pp_scale_guard (the unscaling of the gradient slab by a power of two: exact); the guard word is raised by a
    value that is not finite and by nothing else"""
    _, name, a = key
    _, n, value = a[:3]
    ops = _DOps(key)
    x = ops.randn(n)
    p = _b(x)
    if name == 'pp_scale':
        run.K.pp_scale(p.data_ptr(), n, value, run.st)
    else:
        bad = _zeros(2, dtype=torch.int32)
        run.K.pp_scale_guard(p.data_ptr(), n, value, bad.data_ptr(), run.st)
        q = _b(x)
        q[n // 2] = float('inf')
        bad2 = _zeros(2, dtype=torch.int32)
        run.K.pp_scale_guard(q.data_ptr(), n, value, bad2.data_ptr(), run.st)
        _flag(run, 'guard word: 0 for finite values, 1 for an infinite one', bad.tolist() == [0, 0] and bad2.tolist() == [1, 0])
    _exact(run, 'p', p, x.double() * torch.tensor(value).float().double())


# --------------------------------------------------------------------------------------------------------------------- losses
def _loss_operands(ops, N, K, HW):
    zw, zs = ops.randn(N, K, HW, 1, scale=2.0), ops.randn(N, K, HW, 1, scale=2.0)
    t = torch.randint(0, K + 1, (N, HW, 1), generator=ops.g, device=_dev())
    mask = (ops.rand(N, 1, HW, 1) > 0.3).float()
    return _b(zw), _b(zs), _b(t), _b(mask)


def _argmax(key, run):
    """pp_argmax_channels: first maximum wins"""
    _, _, a = key
    _, N, C, HW = a[:4]
    ops = _DOps(key)
    x = ops.randn(N, C, HW)
    x[0, 0, 0] = x[0, C - 1, 0] = 9.0
    t = torch.randint(0, C, (N, HW), generator=ops.g, device=_dev())
    x[1 % N, :, 1:] = F.one_hot(t[1 % N, 1:], C).t().float()              # a one-hot plane, as the scribbles are
    x = _b(x)
    out = _full((N, HW), -1, dtype=torch.int64)
    run.K.pp_argmax_channels(x.data_ptr(), N, C, HW, out.data_ptr(), run.st)
    _flag(run, 'argmax bit-identical', torch.equal(out, x.argmax(1)))


def _seg64(zw, zs, t, mask, K, ignore, do_ent, variant, detach):
    """(pce, ent, cr) in float64 with autograd leaves (tests/test_gpu_ops.py::test_seg_losses)"""
    zwr = zw.double().requires_grad_(True)
    zsr = zs.double().requires_grad_(True) if variant else None
    m = mask.double() if mask is not None else None
    pce = O.partial_cross_entropy_loss(zwr, t, ignore)
    ent = O.entropy_minimization_loss(zwr, m) if do_ent else None
    cr = None
    if variant:
        pw = torch.softmax(zwr, 1)
        if detach:
            pw = pw.detach()
        cr = {1: lambda: O.soft_label_cross_entropy_loss(zsr, pw, m), 2: lambda: O.l1_loss(torch.softmax(zsr, 1), pw, m),
              3: lambda: O.l2_loss(torch.softmax(zsr, 1), pw, m), 4: lambda: O.kl_loss(zsr, zwr, m)}[variant]()
    return zwr, zsr, pce, ent, cr


def _scalar(run, label, got, ref, tol=TOL_LOSS, floor=1.0):
    """|got - ref| < tol * max(floor, |ref|): test_seg_losses and the CRF tests bound a loss value with floor 1, test_aux_pce and
    test_memory_update_and_ce purely relatively (floor 0)"""
    ref = ref.detach().reshape(1).double()
    mag = ref.abs().clamp_min(floor)
    run.res.append((label, got.reshape(1).double() - ref + mag, mag, tol, False))


def _seg_losses(key, run):
    """pp_seg_losses_fwd (+ pp_losses_finalize for the values) / pp_seg_losses_bwd"""
    _, name, a = key
    lib = _L()
    bwd = name.endswith('_bwd')
    _, lsp, _, mp, N, K, HW, ignore, do_ent, variant = a[:10]
    ops = _DOps(key)
    zw, zs, t, mask = _loss_operands(ops, N, K, HW)
    variant_ref = variant if lsp else 0
    mask = mask if mp else None
    sums = _zeros(6, dtype=torch.float64)
    nws = lib.pp_seg_losses_workspace(N, HW)
    ws = _ws(nws)
    fwd_table = lib if bwd else run.K
    fwd_table.pp_seg_losses_fwd(zw.data_ptr(), zs.data_ptr() if lsp else None, t.data_ptr(), _p(mask), N, K, HW, ignore, do_ent, variant,
                                sums.data_ptr(), ws.data_ptr(), nws, run.st)
    detach = a[10] if bwd else 0
    zwr, zsr, pce, ent, cr = _seg64(zw, zs, t, mask, K, ignore, do_ent, variant_ref, detach)
    if not bwd:
        lp, le, lc = (_zeros(()) for _ in range(3))
        lib.pp_losses_finalize(sums.data_ptr(), 1 if mp else 0, lp.data_ptr(), le.data_ptr() if do_ent else None,
                               lc.data_ptr() if variant_ref else None, run.st)
        _scalar(run, 'loss_pce', lp, pce)
        if do_ent:
            _scalar(run, 'loss_ent', le, ent)
        if variant_ref:
            _scalar(run, 'loss_cr', lc, cr)
        return
    _, gpp, gep, gcp, gscale, _, dsp = a[11:18]
    gw = dict(pce=0.7, ent=0.3, cr=1.9)
    gs = {k: _b(torch.tensor(v)) for k, v in gw.items()}
    dzw = _full(zw.shape, 7.0)
    dzs = _full(zs.shape, 7.0) if dsp else None
    run.K.pp_seg_losses_bwd(zw.data_ptr(), zs.data_ptr() if lsp else None, t.data_ptr(), _p(mask), N, K, HW, ignore, do_ent, variant, detach,
                            sums.data_ptr(), gs['pce'].data_ptr() if gpp else None, gs['ent'].data_ptr() if gep else None,
                            gs['cr'].data_ptr() if gcp else None, gscale, dzw.data_ptr(), _p(dzs), run.st)
    total = pce * (gw['pce'] if gpp else 0.0)
    if do_ent and gep:
        total = total + gw['ent'] * ent
    if variant_ref and gcp:
        total = total + gw['cr'] * cr
    (total * gscale).backward()
    _flag(run, 'gradients finite', bool(torch.isfinite(dzw).all()) and (dzs is None or bool(torch.isfinite(dzs).all())))
    run.check('dlogits_w', dzw, zwr.grad, act=False)
    if dzs is not None:
        if zsr is not None and zsr.grad is not None:
            run.check('dlogits_s', dzs, zsr.grad, act=False)
        elif variant:       # a consistency variant without an upstream gradient: the kernel stores its zero gradient
            _flag(run, 'dlogits_s zero without a consistency gradient', bool((dzs == 0).all()))
        else:               # no consistency loss: the buffer is not written
            _flag(run, 'dlogits_s untouched without a consistency loss', bool((dzs == 7.0).all()))


def _losses_finalize(key, run):
    """pp_losses_finalize: quotients of the double sums, denominators clamped at 1e-8 under a mask"""
    _, _, a = key
    _, has_mask, lpp, lep, lcp = a[:5]
    ops = _DOps(key)
    sums = _b(ops.rand(6).double() * 100 + 1)
    outs = [_full((), 7.0) if p else None for p in (lpp, lep, lcp)]
    run.K.pp_losses_finalize(sums.data_ptr(), has_mask, *(_p(o) for o in outs), run.st)
    for i, (lab, o) in enumerate(zip(('loss_pce', 'loss_ent', 'loss_cr'), outs)):
        if o is not None:
            _scalar(run, lab, o, sums[2 * i] / sums[2 * i + 1])


def _aux_pce(key, run):
    """pp_aux_pce_fwd / pp_aux_pce_bwd (tests/test_gpu_ops.py::test_aux_pce)"""
    _, name, a = key
    lib = _L()
    bwd = name.endswith('_bwd')
    if bwd:
        _, _, ignore, _, gscale, _, _, N, K, h, w, H, W = a[:13]
    else:
        _, N, K, h, w, H, W, _, ignore = a[:9]
        gscale = 1.0
    ops = _DOps(key)
    lo = ops.randn(N, K, h, w)
    t = torch.randint(0, K, (N, H, W), generator=ops.g, device=_dev())
    t[ops.rand(N, H, W) > 0.1] = ignore
    lo, t = _b(lo), _b(t)
    lor = lo.double().requires_grad_(True)
    up = F.interpolate(lor, size=(H, W), mode='bilinear', align_corners=True)
    loss = O.partial_cross_entropy_loss(up, t, ignore)
    upd = _full((N, K, H, W), 7.0)
    sums = _zeros(2, dtype=torch.float64)
    nws = 16 * min(1024, -(-N * H * W // 256))          # the header: two doubles per block of the grid, nothing more
    ws = _ws(nws)
    (lib if bwd else run.K).pp_aux_pce_fwd(lo.data_ptr(), N, K, h, w, H, W, t.data_ptr(), ignore, upd.data_ptr(), sums.data_ptr(),
                                           ws.data_ptr(), nws, run.st)
    if not bwd:
        lv = _zeros(())
        lib.pp_losses_finalize(sums.data_ptr(), 0, lv.data_ptr(), None, None, run.st)
        run.check('logits_up', upd, up.detach(), TOL_LOSS, act=False)
        _scalar(run, 'loss_aux', lv, loss, floor=0.0)
        return
    g = _b(torch.tensor(0.01))
    dlo = _full((N, K, h, w), 7.0)
    run.K.pp_aux_pce_bwd(upd.data_ptr(), t.data_ptr(), ignore, g.data_ptr(), gscale, sums.data_ptr(), dlo.data_ptr(), N, K, h, w, H, W,
                         run.st)
    (0.01 * gscale * loss).backward()
    run.check('dlo', dlo, lor.grad, act=False)


def _memory_update(key, run):
    """pp_memory_update (tests/test_gpu_ops.py::test_memory_update_and_ce; oracle/pacing_oracle.py::memory_update in float64)"""
    _, _, a = key
    _, ld, hid, h, w, _, K, H, W, _, mom, cosine = a[:12]
    lib = _L()
    ops = _DOps(key)
    feat = ops.r(ops.randn(1, h, w, hid))
    t = torch.randint(0, K, (1, H, W), generator=ops.g, device=_dev())
    t[ops.rand(1, H, W) > 0.05] = K
    t[t == K - 1] = K                                       # the last class is absent from sample 0
    scb = _b(F.one_hot(t, K + 1).permute(0, 3, 1, 2).float())
    bank = torch.zeros(K, hid, 1, 1, device=_dev())
    bank[1 % K, :, 0, 0] = ops.randn(hid)                   # visited before; the others are first visits
    bank[K - 1, :, 0, 0] = ops.randn(hid)
    ref = bank.double().clone()
    args = SimpleNamespace(num_classes=K, hid_ch=hid, ensemble_mode='cosine_similarity' if cosine else 'mean', epoch=1,
                           update_momentum=float(mom))       # ramp_up_mo(0, 1, m) == m
    O.memory_update(ref, feat.double().permute(0, 3, 1, 2), scb.double(), 0, args)
    bd = _f32(run, bank)
    nws = lib.pp_memory_update_workspace(K, hid)
    ws = _ws(nws)
    run.K.pp_memory_update(run.d(ops.pad(feat, ld)).data_ptr(), ld, hid, h, w, scb.data_ptr(), K, H, W, bd.data_ptr(), mom, cosine,
                           ws.data_ptr(), nws, run.st)
    run.check('bank', bd, ref, TOL_LOSS, act=False)
    _flag(run, 'row of an absent class untouched', torch.equal(bd[K - 1], bank[K - 1]))


def _memory_ce(key, run):
    """pp_memory_ce_fwd / pp_memory_ce_bwd"""
    _, name, a = key
    _, _, K, hid = a[:4]
    ops = _DOps(key)
    bank, wfc = _b(ops.randn(K, hid)), _b(ops.randn(K, hid))
    wr = wfc.double().requires_grad_(True)
    loss = O.cross_entropy_loss(bank.double() @ wr.t(), torch.arange(K, device=_dev()))
    if name.endswith('_fwd'):
        lv = _full((), 7.0)
        run.K.pp_memory_ce_fwd(bank.data_ptr(), wfc.data_ptr(), K, hid, lv.data_ptr(), run.st)
        _scalar(run, 'loss_memory', lv, loss, floor=0.0)
        return
    _, gscale, _, acc = a[4:8]
    g = _b(torch.tensor(1.5))
    prior = ops.randn(K, hid)
    dw = _b(prior) if acc else _full((K, hid), 7.0)
    run.K.pp_memory_ce_bwd(bank.data_ptr(), wfc.data_ptr(), K, hid, g.data_ptr(), gscale, dw.data_ptr(), acc, run.st)
    (1.5 * gscale * loss).backward()
    run.check('dwfc', dw, wr.grad + (prior.double() if acc else 0), act=False)


def _crf(key, run):
    """pp_crf_loss_fwd / pp_crf_loss_bwd against tests/_crf_reference.py (tolerances of tests/test_gpu_crf.py)"""
    _, name, a = key
    lib = _L()
    from tests._crf_reference import crf_loss_and_grad, smooth_image
    ops = _DOps(key)
    if name.endswith('_bwd'):
        _, _, has_mask, _, gscale, _, n = a[:7]
        unit, prior = _b(ops.randn(n)), ops.randn(n)
        sums = _b(torch.tensor([3.0, 1000.0 if has_mask else float(n)], dtype=torch.float64))
        g = _b(torch.tensor(0.3))
        dl = _b(prior)
        run.K.pp_crf_loss_bwd(unit.data_ptr(), sums.data_ptr(), has_mask, g.data_ptr(), gscale, dl.data_ptr(), n, run.st)
        run.check('dlogits', dl, prior.double() + gscale * 0.3 * (-2.0 / float(sums[1])) * unit.double(), act=False)
        return
    _, _, mp, N, K, C, H, W, radius, dilation, sxy, srgb, up = a[:13]
    z, mask = _b(ops.randn(N, K, H, W, scale=2.0)), (_b((ops.rand(N, 1, H, W) > 0.3).float()) if mp else None)
    img = _b(smooth_image(N, C, H, W, 5))
    ref_loss, ref_grad = crf_loss_and_grad(z.cpu(), img.cpu(), mask.cpu() if mp else None, radius=radius, dilation=dilation,
                                           sigma_xy=sxy, sigma_rgb=srgb)
    unit = _full((N, K, H, W), 7.0) if up else None
    sums = _zeros(2, dtype=torch.float64)
    nws = lib.pp_crf_loss_workspace(N, H, W)
    ws = _ws(nws)
    run.K.pp_crf_loss_fwd(z.data_ptr(), img.data_ptr(), _p(mask), N, K, C, H, W, radius, dilation, sxy, srgb, _p(unit), sums.data_ptr(),
                          ws.data_ptr(), nws, run.st)
    D = max(float(sums[1]), 1e-8) if mp else float(sums[1])
    _scalar(run, 'loss_crf', (sums[0] / D).float(), ref_loss.to(_dev()))
    if up:
        run.check('unit gradient', unit.double() * (-2.0 / D), ref_grad.to(_dev()), act=False)


ADAPTERS = {
    'pp_bn_train_stats': _bn_stats, 'pp_bn_stats_sums': _bn_stats,
    'pp_bn_train_finalize': _bn_finalize, 'pp_bn_train_finalize_lazy': _bn_finalize, 'pp_bn_eval_coeffs': _bn_eval_coeffs,
    'pp_bn_eval_coeffs_batch': _bn_eval_coeffs_batch, 'pp_bn_lrelu_fwd': _bn_fwd, 'pp_bn_lrelu_fwd_pool': _bn_fwd,
    'pp_bn_lrelu_bwd': _bn_bwd, 'pp_bn_lrelu_bwd_amax': _bn_bwd, 'pp_bn_lrelu_bwd_eval': _bn_bwd, 'pp_bn_lrelu_bwd_pool': _bn_bwd,
    'pp_bn_lrelu_bwd_eval_pool': _bn_bwd, 'pp_bn_lrelu_bwd_apply': _bn_bwd, 'pp_bn_lrelu_bwd_sums': _bn_bwd_sums,
    'pp_gn_stats': _gn_stats, 'pp_gn_lrelu_bwd': _gn_bwd, 'pp_gn_lrelu_bwd_pool': _gn_bwd, 'pp_lazy_materialize': _lazy_materialize,
    'pp_stride2_gather': _stride2, 'pp_stride2_scatter': _stride2, 'pp_maxpool2_fwd': _maxpool, 'pp_maxpool2_bwd': _maxpool,
    'pp_bilinear_fwd': _bilinear, 'pp_bilinear_bwd': _bilinear, 'pp_copy_slab': _copy_slab, 'pp_channel_scale': _channel_scale,
    'pp_pack_conv3x3_weights_f16x3_batch': _pack_batch, 'pp_wino_pack_weights_f16x3_batch': _pack_batch, 'pp_scale': _scale,
    'pp_scale_guard': _scale, 'pp_pack_image_nchw_to_nhwc': _pack_image, 'pp_pack_conv3x3_weights': _pack_weights, 'pp_wino_pack_weights': _pack_weights,
    'pp_argmax_channels': _argmax, 'pp_seg_losses_fwd': _seg_losses, 'pp_seg_losses_bwd': _seg_losses,
    'pp_losses_finalize': _losses_finalize, 'pp_aux_pce_fwd': _aux_pce, 'pp_aux_pce_bwd': _aux_pce,
    'pp_memory_update': _memory_update, 'pp_memory_ce_fwd': _memory_ce, 'pp_memory_ce_bwd': _memory_ce,
    'pp_crf_loss_fwd': _crf, 'pp_crf_loss_bwd': _crf,
}


def replay(key, table=None):
    """[(label, error / tolerance)] of one launch shape: replay() of the convolution census with this module's adapters"""
    return _replay(key, ADAPTERS, table)


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope='module')
def census():
    """{(storage, entry, launch shape): configurations}: everything in the shared recording the convolution census does not own"""
    from tests._launch_census import record
    return {key: cfgs for key, cfgs in record().items() if not _is_conv_launch(key[1])}


def test_census_holds_what_the_dispatch_promises(census):
    """Not vacuous: the recording contains the launches the engine's rules send these configurations to."""
    def has(cfg_prefix, storage, names, pred=lambda n, a: True):
        return any(s == storage and n in names and pred(n, a) and any(c.startswith(cfg_prefix) for c in cfgs)
                   for (s, n, a), cfgs in census.items())
    assert has('256/os8', 'fp32', ('pp_bilinear_bwd',), lambda n, a: a[6] == 128)         # RB = 16, the largest launch
    assert has('224/os8/4cls', 'fp32', ('pp_bilinear_bwd',), lambda n, a: a[6] == 28)
    assert has('256/os8', 'fp32', ('pp_bn_lrelu_bwd_pool', 'pp_bn_lrelu_bwd_eval_pool'))
    assert has('256/os8/train-BN', 'fp32', ('pp_bn_lrelu_bwd_pool',), lambda n, a: a[22] == 2)      # weak + strong: two groups
    assert has('256/os8', 'fp32', ('pp_bn_train_finalize_lazy',)) and has('256/os8', 'fp32', ('pp_bn_train_finalize',))
    for n in ('pp_bn_stats_sums', 'pp_bn_lrelu_bwd_sums', 'pp_bn_lrelu_bwd_apply'):
        assert has('256/sync_bn', 'fp32', (n,)), n
    # the launches that go through engine.py's module-level table, not a plan's
    assert has('256/os8/eval-BN', 'fp32', ('pp_bn_eval_coeffs_batch',), lambda n, a: a[1] >= 10)
    assert has('256/os8', 'fp32', ('pp_pack_conv3x3_weights_f16x3_batch',)) and has('256/os8', 'fp32', ('pp_wino_pack_weights_f16x3_batch',))
    for n in ('pp_gn_stats', 'pp_gn_lrelu_bwd', 'pp_gn_lrelu_bwd_pool'):
        assert has('256/groupnorm', 'fp32', (n,)), n
    assert has('256/groupnorm', 'fp32', ('pp_bn_lrelu_fwd', 'pp_bn_lrelu_fwd_pool'), lambda n, a: a[-3] == 4)      # one row per image
    assert has('256/strided', 'fp32', ('pp_stride2_gather',)) and has('256/strided', 'fp32', ('pp_stride2_scatter',))
    for kind in ('fp16', 'bf16'):
        for n in ('pp_bn_train_finalize_lazy', 'pp_bn_lrelu_fwd', 'pp_bn_lrelu_bwd_pool', 'pp_bn_lrelu_bwd_eval', 'pp_bilinear_fwd',
                  'pp_bilinear_bwd', 'pp_maxpool2_fwd', 'pp_memory_update'):
            assert has(f'256/{kind}', kind, (n,)), (kind, n)
    for n in ('pp_argmax_channels', 'pp_seg_losses_fwd', 'pp_seg_losses_bwd', 'pp_losses_finalize', 'pp_aux_pce_fwd', 'pp_aux_pce_bwd',
              'pp_memory_ce_fwd', 'pp_memory_ce_bwd', 'pp_copy_slab'):
        assert any(k[1] == n for k in census), n


def _report(keys, cfgs_of):
    """Replay `keys`; print the worst error / tolerance per entry point; return (failures, entry points without an adapter)."""
    worst = defaultdict(float)
    failures, missing = [], set()
    for key in keys:
        try:
            res = replay(key)
        except KeyError as e:
            missing.add(str(e.args[0]))
            continue
        entry = key[1] + {'fp32': '', 'fp16': '_h16', 'bf16': '_bf16'}[key[0]]
        for label, ratio in res:
            worst[entry] = max(worst[entry], ratio)
            if not ratio <= 1.0:
                failures.append((ratio, entry, label, key[2], cfgs_of(key)))
    for e in sorted(worst):
        print(f'  worst error / tolerance  {e:42s} {worst[e]:.3g}')
    failures.sort(key=lambda f: -f[0] if f[0] == f[0] else -math.inf)
    return failures, missing


def test_every_recorded_stream_launch_matches_float64(census):
    """Replay every distinct launch; list every failing one, worst first, with the configurations that produced it."""
    from tests._launch_census import record
    per_cfg = defaultdict(int)
    for cfgs in census.values():
        for c in cfgs:
            per_cfg[c] += 1
    print(f'\nstream census: {len(census)} distinct launches ({len(record())} recorded with the convolution family)')
    for c in sorted(per_cfg):
        print(f'  {c:28s} {per_cfg[c]:4d} distinct launches')
    failures, missing = _report(sorted(census, key=repr), lambda key: sorted(census[key]))
    assert not missing, f'recorded launches of entry points neither census owns: {sorted(missing)}'
    assert not failures, '\n'.join(f'{r:.3g} x tol  {e}  {lab}  args={a}  from {cfgs}' for r, e, lab, a, cfgs in failures)


def _batch_config_names():
    from tests._launch_census import batch_configs
    return sorted(batch_configs())


@pytest.mark.parametrize('cfg', _batch_config_names())
def test_batch_recording_matches_float64(cfg):
    """The other half of test_batch_recording_matches_float64 of the convolution census: the norm, spatial and loss launches of the
    batch recordings (batch 3 and 12, 16-bit storage at batch 3, the Control plan at batch 8) through the same replay."""
    from tests._launch_census import batch_configs, record_batches
    from tests.test_gpu_conv_census import _of_config
    variant = batch_configs()[cfg][4]
    mine = {key: cfgs for key, cfgs in _of_config(record_batches(), cfg).items() if not _is_conv_launch(key[1])}
    at = {'pp_bn_lrelu_bwd': 18, 'pp_bn_lrelu_bwd_amax': 18, 'pp_bn_lrelu_bwd_pool': 22}       # where the statistics groups stand
    groups = {a[at[n]] for (_, n, a) in mine if n in at}
    print(f'\n{cfg}: {len(mine)} distinct stream launches, statistics groups of the train-mode BatchNorm backward {sorted(groups)}')
    # not vacuous: the BatchNorm backward is there, in two statistics groups (weak and strong view) or, in the Control plan, one
    assert any(n.startswith('pp_bn_lrelu_bwd') for (_, n, _) in mine), sorted({k[1] for k in mine})
    assert (groups == {1}) if variant == 'control' else (2 in groups), (cfg, groups)
    failures, missing = _report(sorted(mine, key=repr), lambda key: sorted(mine[key]))
    assert not missing, f'recorded launches of entry points neither census owns: {sorted(missing)}'
    assert not failures, '\n'.join(f'{r:.3g} x tol  {e}  {lab}  args={a}  from {cfgs}' for r, e, lab, a, cfgs in failures)


# ------------------------------------------------------------------------------------------------- launches the network never makes
def _bil(name, C, N, Hi, Wi, Ho, Wo, acc=0):
    if name == 'pp_bilinear_fwd':
        return (name, ('p', C + 8, 'p', C + 4, C, N, Hi, Wi, Ho, Wo, 'p'))
    return (name, ('p', C + 4, 'p', C + 8, C, N, Hi, Wi, Ho, Wo, acc, 'p'))


# (Hi, Wi, Ho, Wo, C, N): pp_bilinear_bwd takes the column walker when 2 / scale <= 4.1 in both dimensions (x2: Hi >= 22)
BILINEAR_EDGES = {
    'RB8-last-band-of-4-odd-Wi': (36, 23, 72, 46, 4, 1),
    'RB16-last-band-of-2-27-row-blocks': (130, 24, 260, 48, 8, 3),
    'first-size-on-the-walker-side': (22, 22, 44, 44, 4, 1),
    'last-size-on-the-general-side': (20, 20, 40, 40, 4, 1),
    'non-integer-factor-inside-the-walker-range': (40, 40, 60, 60, 4, 1),
    'downscale-untouched-inputs': (33, 20, 16, 7, 4, 2),
}
# (C, P_per_group, groups): col_plan's rows = 256 / (C / 4), chunk and nblk; fin_reduce2 unrolls four rows while nblk > 192
NORM_EDGES = {
    'nblk256-all-slices-unrolled': (1024, 2048, 1),
    'nblk250-unrolled-and-tail-slices': (1024, 2000, 2),
    'rows1-idle-lanes-C516': (516, 300, 1),
    'rows1-idle-lanes-C1020-two-groups': (1020, 300, 2),
    'rows32-nblk-above-192-ragged-last-chunk': (32, 49408 + 17, 1),
    'fewer-pixels-than-rows': (12, 5, 2),
}


def _norm_edge_keys(C, P, G):
    ld, p = C + 4, 'p'
    bwd = (p, ld, p, C + 8, p, p, p, p, p, 1, p, ld, p, p, p, 1, C, P, G, SLOPE, p, 'sz')
    return [
        ('pp_bn_train_stats', (p, ld, C, P, G, EPS, MOM, p, p, p, p, p, p, p, p, p, p, 'sz', p)),
        ('pp_bn_stats_sums', (p, ld, C, P, G, p, p, 'sz', p)),
        ('pp_bn_lrelu_bwd', bwd + (p,)),
        ('pp_bn_lrelu_bwd', bwd[:9] + (0,) + bwd[10:15] + (0,) + bwd[16:] + (p,)),            # training = 0, stored not accumulated
        ('pp_bn_lrelu_bwd_amax', bwd + (p, p)),
        ('pp_bn_lrelu_bwd_eval', (p, ld, p, C + 8, p, p, p, p, ld, p, p, p, 0, C, P * G, SLOPE, p, 'sz', p, p)),
        ('pp_bn_lrelu_bwd_sums', (p, ld, p, C + 8, p, p, p, p, C, P, G, SLOPE, p, p, 'sz', p)),
        ('pp_bn_lrelu_bwd_apply', (p, ld, p, C + 8, p, p, p, p, p, 1, p, p, P, p, ld, p, p, p, 0, C, P, G, SLOPE, p, 'sz', p, p)),
    ]


def _edge_cases():
    cases = []
    for tag, (Hi, Wi, Ho, Wo, C, N) in BILINEAR_EDGES.items():
        cases.append((f'bilinear_fwd/{tag}', _bil('pp_bilinear_fwd', C, N, Hi, Wi, Ho, Wo)))
        for acc in (0, 1):
            cases.append((f'bilinear_bwd/{tag}/acc{acc}', _bil('pp_bilinear_bwd', C, N, Hi, Wi, Ho, Wo, acc)))
    for tag, (C, P, G) in NORM_EDGES.items():
        for k in _norm_edge_keys(C, P, G):
            cases.append((f'{k[0][3:]}/{tag}' + ('/eval-stats' if k[0] == 'pp_bn_lrelu_bwd' and k[1][9] == 0 else ''), k))
    p, C = 'p', 32
    # the "rows > H * W" branch of the pooled forms: 2 x 2 images, one and two groups
    for G in (1, 2):
        cases.append((f'bn_lrelu_fwd_pool/2x2/groups{G}', ('pp_bn_lrelu_fwd_pool', (p, C + 4, p, p, p, C + 8, p, C + 12, C, 2 * G, 2, 2, G, SLOPE, p))))
        cases.append((f'bn_lrelu_bwd_pool/2x2/groups{G}', ('pp_bn_lrelu_bwd_pool', (p, C + 4, p, C + 12, p, C + 8, p, p, p, p, p, 1, p, C + 4, p, p, p, 1,
                                                                                C, 2 * G, 2, 2, G, SLOPE, p, 'sz', p, p))))
    cases.append(('bn_lrelu_bwd_eval_pool/2x2', ('pp_bn_lrelu_bwd_eval_pool', (p, C + 4, p, C + 12, p, C + 8, p, p, p, p, C + 4, p, p, p, 0, C, 2, 2, 2,
                                                                              SLOPE, p, 'sz', p, p))))
    cases.append(('maxpool2_bwd/three-lds/acc1', ('pp_maxpool2_bwd', (p, 16, p, 20, p, 24, 12, 2, 6, 10, 1, p))))
    for acc in (0, 1):
        cases.append((f'copy_slab/ld_x!=ld_y/acc{acc}', ('pp_copy_slab', (p, 20, p, 28, 12, 1031, acc, p))))
        cases.append((f'channel_scale/ld_x!=ld_y/acc{acc}', ('pp_channel_scale', (p, 20, p, 28, p, 12, 3, 345, acc, p))))
    cases.append(('lazy_materialize/two-groups-three-lds', ('pp_lazy_materialize', (p, 36, ('lazy', 40, 2), p, 44, 32, 4, 77, p))))
    cases.append(('bn_eval_coeffs_batch/17-layers', ('pp_bn_eval_coeffs_batch', (p, 17, EPS, p))))
    cases.append(('scale', ('pp_scale', (p, 100003, 2.0 ** -10, p))))
    cases.append(('scale_guard', ('pp_scale_guard', (p, 100003, 2.0 ** -10, p, p))))
    # the gated-CRF entries (no census configuration switches the loss on): tests/test_gpu_crf.py's bounds through the same gate
    cases.append(('crf_loss_fwd/masked', ('pp_crf_loss_fwd', (p, p, p, 1, 4, 1, 12, 10, 2, 1, 6.0, 0.1, p, p, p, 'sz', p))))
    cases.append(('crf_loss_fwd/no-mask-no-gradient', ('pp_crf_loss_fwd', (p, p, None, 2, 5, 1, 9, 11, 3, 2, 6.0, 0.1, None, p, p, 'sz', p))))
    cases.append(('crf_loss_bwd', ('pp_crf_loss_bwd', (p, p, 1, p, 1024.0, p, 481, p))))
    return cases


EDGES = _edge_cases()


@pytest.mark.parametrize('storage', ['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('tag,launch', EDGES, ids=[t for t, _ in EDGES])
def test_edge_launch_matches_float64(tag, launch, storage):
    """Hand-made launch shapes at the sizes where the kernels change path, through the adapters of the census."""
    res = replay((storage,) + launch)
    bad = [(lab, r) for lab, r in res if not r <= 1.0]
    print(f'{tag} [{storage}]: worst error / tolerance {max(r for _, r in res):.3g}')
    assert not bad, f'{tag} [{storage}] args={launch[1]}: ' + ', '.join(f'{lab} {r:.3g} x tol' for lab, r in bad)


def replayed_entry_points():
    """Every entry point, suffix included, that the recordings and the two edge tables replay in its own storage type."""
    from tests._launch_census import record, record_batches
    from tests.test_gpu_conv_census import EDGE_PARAMS
    suffix = {'fp32': '', 'fp16': '_h16', 'bf16': '_bf16'}
    seen = {n + suffix[s] for rec in (record(), record_batches()) for (s, n, _) in rec}
    seen |= {launch[0] + suffix[s] for _, launch, s in EDGE_PARAMS}
    seen |= {launch[0] + suffix[s] for _, launch in EDGES for s in ('fp32', 'fp16', 'bf16')}
    return seen


def test_twins_the_ownership_gate_counts_are_replayed():
    """tests/test_bounds_ownership.py counts a census adapter as the owner of its entry point's _h16 / _bf16 twins.  Here that is
    measured: every such twin is replayed in its storage type by a recording or an edge row, or -- the forms no 16-bit plan
    takes -- called under its own name by a case of the bounds table (tests/test_gpu_bounds.py)."""
    from pacingpseudo_amd._lib import _PROTOS
    from tests.test_gpu_bounds import owned_by_family
    from tests.test_gpu_conv_census import ADAPTERS as CONV
    seen = replayed_entry_points() | {e for entries in owned_by_family().values() for e in entries}
    twins = {b + x for b in set(CONV) | set(ADAPTERS) for x in ('_h16', '_bf16') if b + x in _PROTOS}
    assert not sorted(twins - seen), sorted(twins - seen)
    assert not [b for b in set(CONV) | set(ADAPTERS) if b not in seen]


# ------------------------------------------------------------------------------------------------------ the gate bites
class _Planted:
    """An entry-point table that calls ONE entry point wrongly (arguments rewritten by `mutate`), everything else unchanged."""

    def __init__(self, inner, name, mutate):
        self._inner, self._name, self._mutate = inner, name, mutate

    def __getattr__(self, n):
        fn = getattr(self._inner, n)
        if n != self._name:
            return fn
        return lambda *a: fn(*self._mutate(list(a)))


def _set(i, f):
    def mutate(a):
        a[i] = f(a)
        return a
    return mutate


def _one_group(a):                     # pp_bn_lrelu_bwd: all pixels as ONE statistics group (reads group 0's coefficient rows only)
    a[17], a[18] = a[17] * a[18], 1
    return a


PLANTS = {
    # every planted call stays inside the buffers the adapter allocated: a smaller stride, never a larger extent
    'bilinear_bwd-accumulate-dropped': (_bil('pp_bilinear_bwd', 4, 1, 36, 23, 72, 46, 1), _set(10, lambda a: 0), ('dx',)),
    'bn_lrelu_bwd-groups-merged': (_norm_edge_keys(32, 600, 2)[2], _one_group, ('dz',)),
    'bn_lrelu_fwd-ld_y-replaced-by-C': (('pp_bn_lrelu_fwd', ('p', 36, 'p', 'p', 'p', 40, 32, 600, 2, SLOPE, 'p')), _set(5, lambda a: a[6]),
                                        ('y', 'y canary')),
}


@pytest.mark.parametrize('plant', sorted(PLANTS))
def test_planted_mistake_fails_the_replay(plant):
    """The same replay with an entry-point table that makes one mistake must report error / tolerance > 1 (and a touched canary
    where the mistake moves the rows); with the honest table the same launch passes."""
    from pacingpseudo_amd._lib import lib
    launch, mutate, must_fail = PLANTS[plant]
    key = ('fp32',) + launch
    honest = dict(replay(key))
    assert all(r <= 1.0 for r in honest.values()), honest
    assert sum(label.endswith(' band') for label in honest) >= 2, 'no sentinel-band verdicts in the replay (an input and an output at least)'
    planted = dict(replay(key, table=_Planted(lib, launch[0], mutate)))
    for label in must_fail:
        assert planted[label] > 1.0, (plant, label, planted)
