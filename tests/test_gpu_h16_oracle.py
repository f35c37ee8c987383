"""16-bit storage (`--storage fp16 | bf16`) against an oracle that rounds where the engine stores.

tests/test_gpu_h16.py holds every `_h16` / `_bf16` entry point to its fp32 twin, and the whole step to the fp32 storage mode at
smoke-test bounds.  This module checks the wiring around the kernels -- which entry point a plan calls, the byte offsets of
16-bit slices, the concatenation halves, lazy buffers, the loss scale -- against the CPU oracle with
`pacing_oracle.StorageRounding` switched on.  The rounding sites come from the plan (`storage_sites`), not from fitting.

* Per layer, teacher-forced: each convolution's actual device input through the fp64 oracle layer, compared with the z and y the
  device stored; the max-pooled and up-sampled tensors likewise.
* Whole step: logits, losses and every parameter gradient against the rounded and against the unrounded oracle."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests.test_gpu_step import build_model, device_masks, device_pool_winners  # noqa: E402

KINDS = {'fp16': (torch.float16, 10, -14), 'bf16': (torch.bfloat16, 7, -126)}


@pytest.fixture(params=['fp16', 'bf16'])
def kind(request):
    return request.param


# ------------------------------------------------------------------------------------------------ the site map
def _split_k(L, h, w, plan) -> int:
    """Input channels of the first launch when the forward convolution of L runs as two split-K launches (conv_dispatch_f16x3 in
    pp_conv.hip: 128 < Cin <= 192, Cin % 64 == 0, and the one-row halo kernel takes Cin / 2 -- dil 1, Cout % 32 == 0,
    Cout <= 192, W % 32 == 0, H % 4 == 0).  The first launch stores its half-sum (bias included) in the 16-bit output buffer and
    the second adds to what it reads back."""
    if plan.conv[L.name].sel.kind != 'f16x3':
        return 0
    c = L.cin
    if not (128 < c <= 192 and c % 64 == 0):
        return 0
    half_ok = (L.dil == 1 and (c // 2) % 32 == 0 and c // 2 <= 96 and L.cout % 32 == 0 and L.cout <= 192 and w % 32 == 0 and h % 4 == 0)
    return c // 2 if half_ok else 0


def storage_sites(model, training: bool) -> dict:
    """pacing_oracle.StorageRounding sites of the last forward of `model` (a ConsistencyRegulr in 16-bit storage), read from the plan:

    * lazy output (plan.lazy_out, train mode): the buffer holds the rounded z, y is never stored (its consumers evaluate it in
      fp32 on load);
    * own z buffer (plan.zbuf): z and y are stored (train mode); the eval-mode fused epilogue stores y only;
    * split-K: the first half-sum is stored (_split_k);
    * activation gradients: every dz (except the first layer's, whose BatchNorm backward feeds the weight gradient directly),
      every dy, the up-sampled, pooled and concatenated tensors' gradients;
    * encoder stage outputs (the skip half of plan.cat): several consumers.  Where the next stage max-pools, the BatchNorm
      backward adds the pooled gradient to the skip gradient in fp32; otherwise the consumers add into one 16-bit buffer in
      the engine's order -- decoder (writes first), auxiliary bottleneck (strong view; accumulates), next encoder stage
      (accumulates): round(round(round(g_dec) + g_aux) + g_next).

    Not reproduced (the bounds absorb them): shapes whose convolution runs without a fused BatchNorm epilogue store z before the
    statistics / the eval-mode apply pass read it (pp_conv3x3_fwd_bn; none at 256 x 256, some 28 x 28 layers at 224 x 224 in
    train mode, where the statistics then see the rounded z); the operand split inside the Winograd domain and the fp32
    accumulation order of every kernel.  Any buffer kind or layout this function does not know raises."""
    from pacingpseudo_amd import engine as E
    eng = model.engine
    plan = eng.last_plan
    if not plan.h16:
        raise ValueError('storage_sites: the last plan is not a 16-bit storage plan')
    if not (E.FUSE_BN and E.FUSE_POOL_BWD and E.FUSE_WG1) or eng.sync_bn or eng.comm is not None:
        raise NotImplementedError('storage_sites knows the default single-process plan only')
    if any(L.gn or L.stride != 1 for L in eng.layers):
        raise NotImplementedError('storage_sites: GroupNorm / strided layers')
    sites = {'input': 'F'}
    enc_out_layers = {eng.enc_layers[k][1].name: k for k in range(1, 7)}

    def layer(L, p, h, w, dz_stored=True):
        lazy = training and plan.lazy_out[L.name]
        if not lazy and L.name not in plan.zbuf and training:
            raise NotImplementedError(f'{L.name}: train-mode layer without a z buffer and not lazy')
        sites[p + ':z'] = ('F' if training else '') + ('B' if dz_stored else '')
        multi = L.name in enc_out_layers
        sites[p + ':y'] = ('' if lazy else 'F') + ('' if multi else 'B')
        sites[p + ':split'] = _split_k(L, h, w, plan)

    for L in eng.layers:
        h, w = plan._layer_hw(eng, L)
        first = L is eng.layers[0]
        if first and L.cin != 1:
            raise NotImplementedError('storage_sites: the first layer is expected to have one input channel')
        layer(L, 'backbone.' + L.name, h, w, dz_stored=not first)
    decs = eng.backbone.dec_blocks()
    aux_stages = set(plan.aux['stages']) if plan.aux is not None else set()
    if plan.aux is not None:
        if not plan.aux['alias_cat5'] or 'drop_in' in plan.aux:
            raise NotImplementedError('storage_sites: the auxiliary input must alias cat5 and have no Dropout2d copies')
        LA = eng.aux_layer
        layer(LA, 'aux_path.layer_bottleneck', plan.aux['h'], plan.aux['w'])
        sites['aux_path.layer_bottleneck:y'] = 'FB'
        if sites['aux_path.layer_bottleneck:split']:
            raise NotImplementedError('storage_sites: split-K auxiliary bottleneck')
        del sites['aux_path.layer_bottleneck:split']
    for k in range(1, 7):
        if k in plan.pooled:
            sites[f'backbone.enc_block{k}.pooling'] = 'B'
        nxt_pools = k < 6 and (k + 1) in plan.pooled
        if nxt_pools:
            sites[f'backbone.enc_block{k}'] = 'fused'
        else:
            sites[f'backbone.enc_block{k}'] = ['dec'] + (['aux'] if k in aux_stages else []) + (['next'] if k < 6 else [])
    for k in (5, 4, 3, 2, 1):
        d = decs[k]
        if d.trans:
            raise NotImplementedError('storage_sites: transposed-convolution decoder')
        sites[f'backbone.dec_block{k}.up'] = '' if d.identity_up else 'FB'
        sites[f'backbone.dec_block{k}.cat'] = 'B'
    return sites


def rounding_for(model, kind, training):
    return O.StorageRounding(KINDS[kind][0], model.engine.last_plan.loss_scale, storage_sites(model, training))


def _setup(kind, size, num_classes, bn_eval, seed=11):
    args = O.full_flags(num_classes=num_classes, ignored_index=num_classes)
    args.storage = kind
    torch.manual_seed(1)
    model = build_model(args)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batch = O.synthetic_batch(2, size, size, num_classes=num_classes, seed=seed, keep=0.03)
    model.train()
    if bn_eval:
        model.eval()
    return args, model, sd, batch


def _device_step(model, batch, args):
    out = model({k: v.cuda() for k, v in batch.items() if k != 'label'}, mode='train', step=0)
    loss = sum(out[k] * wt for k, wt in O.loss_weights(args, 0).items())      # the oracle's train_step weighting
    loss.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().double().cpu() for k, v in out.items()},
            {n: q.grad.detach().double().cpu() for n, q in model.named_parameters() if q.grad is not None})


# ------------------------------------------------------------------------------------------------ per layer, teacher-forced
def r16(t, kind):
    """fp64 / fp32 -> fp32 -> the 16-bit type, as a float64 tensor."""
    return t.float().to(KINDS[kind][0]).double()


def ulp16(t, kind):
    """Unit in the last place of the 16-bit type at |t| (subnormal spacing below its smallest normal number)."""
    _, mant, emin = KINDS[kind]
    a = t.abs().double().clamp_min(2.0 ** emin)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - mant)


def nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def lrelu32(t):
    """LeakyReLU as the kernels evaluate it on an fp32 pre-activation (slope 0.01 as an fp32 number)."""
    t = t.float()
    return torch.where(t > 0, t, t * torch.tensor(SLOPE, dtype=torch.float32)).double()


def logical_input(v):
    """fp64 NCHW values a consumer of view v computes with: where the buffer is lazy, lrelu(fma(z, scale, shift)) in fp32 from the
    raw z and the coefficient rows (View.values() would round them to 16 bits)."""
    raw = v.torch().double()
    if not v.lazy:
        return nchw64(raw)
    rows = v.coef_rows().double().cpu()                  # (groups, 3, C): scale, shift, slope
    raw = nchw64(raw)
    n = v.N // v.cg
    out = []
    for g in range(v.cg):
        t = (raw[g * n:(g + 1) * n] * rows[g, 0][None, :, None, None] + rows[g, 1][None, :, None, None]).float()
        out.append(torch.where(t > 0, t, t * rows[g, 2][None, :, None, None].float()).double())
    return torch.cat(out)


def _conv64(x, w, b, dil, c1, kind, wino=False):
    """The layer's convolution in fp64 -- split-K: the first launch's half-sum (bias included) rounded as it is stored -- and how
    far the device's z may be from it before the final store: the fp32 accumulation noise, 2^-22 conv(|x|, |w|) + |b| (2^-18 on
    the Winograd path: its F(4x4,3x3) transforms add in fp32 terms several times larger than the result, and its operands are
    split inside the transformed domain), plus one ulp of the split-K half-sum (fp32 noise may put it on the other side of a
    rounding midpoint than the fp64 value)."""
    z1 = F.conv2d(x[:, :c1], w[:, :c1], b, 1, dil, dil) if c1 else None
    z = r16(z1, kind) + F.conv2d(x[:, c1:], w[:, c1:], None, 1, dil, dil) if c1 else F.conv2d(x, w, b, 1, dil, dil)
    tol = (2.0 ** -18 if wino else 2.0 ** -22) * F.conv2d(x.abs(), w.abs(), b.abs(), 1, dil, dil)
    if c1:
        tol = tol + ulp16(z1, kind)
    return z, tol


SLOPE = 1e-2
# share of the elements of a stored tensor that may differ from the prediction at all (only values within fp32 noise of a
# rounding midpoint of the 16-bit type should): about 3x the worst layer measured on the MI355X -- fp16 8.9e-3 (train BN, the
# Winograd layers; 1.2e-3 elsewhere) / 5.2e-4 (eval), bf16 1.4e-3 / 1.6e-4 (parity report rows 'storage_oracle_per_layer_*')
MAX_SHARE = {('fp16', False): 2.7e-2, ('fp16', True): 1.6e-3, ('bf16', False): 4.3e-3, ('bf16', True): 5e-4}
# the prediction WITHOUT the z rounding (train mode) / without the split-K half-sum rounding must differ in at least this share
# (measured: 0.33 - 0.44 on every train-mode layer; 0.27 on dec_block2.conv_layer1 without its half-sum rounding)
MIN_SENSITIVE_SHARE = 0.1


@pytest.mark.timeout(900)
@pytest.mark.parametrize('bn_eval', [False, True])
def test_per_layer_forward_teacher_forced(kind, bn_eval):
    """Full widths, full flags, 2 images per view, 256 x 256, 5 classes.  For every backbone convolution: the device's own input
    (L.x; a lazy input evaluated in fp32 from z and the coefficient rows) through the layer in fp64, rounded where storage_sites
    says the device stores, against what the device stored, element by element (n = the fp32 accumulation-noise scale):

      z (train):  |z_dev - r16(z)| <= ulp16(z) + n, and only a small share of the elements differ at all;
      y:          |y_dev - r16(lrelu(r16(z) scale + shift))| <= ulp16(y) + |scale| (ulp16(z) + n) (+ |pre| within that distance
                  of the kink), with the device's coefficient rows -- first checked against fp64 statistics of z -- and the same
                  share bound.  (Eval mode: no z is stored; the prediction is r16(lrelu(z scale + shift)).)

    Sensitivity, in the test: on at least one layer the prediction without the z rounding (train mode), and on the split-K layer
    the prediction without the half-sum rounding, differ from the device in many more elements than the bound allows, while the
    rounded predictions stay inside it.  The max-pooled tensors must be bit-exact, the bilinear halves of the concatenations
    within one ulp with the same share bound."""
    args, model, sd, batch = _setup(kind, 256, 5, bn_eval)
    training = not bn_eval
    _device_step(model, batch, args)                    # (a forward without gradients would run a forward-only fp32 plan)
    eng, plan = model.engine, model.engine.last_plan
    sites = storage_sites(model, training)
    share_max = MAX_SHARE[(kind, bn_eval)]
    rows, sensitive = [], []
    for L in eng.layers:
        p = 'backbone.' + L.name
        x = logical_input(L.x)[:, :L.cin]
        w, b = sd[p + '.conv.weight'].double(), sd[p + '.conv.bias'].double()
        c1 = sites[p + ':split']
        z, noise = _conv64(x, w, b, L.dil, c1, kind, plan.conv[L.name].sel.kind == 'wino')
        coef = plan.coef[L.name].double().cpu()          # (4, groups, C): mean, invstd, scale, shift
        n = z.shape[0] // L.groups
        per_img = lambda r: torch.cat([r[g][None, :, None, None].expand(n, -1, -1, -1) for g in range(L.groups)])  # noqa: E731
        sc, sh = per_img(coef[2]), per_img(coef[3])
        zr = r16(z, kind)
        row = dict(layer=L.name, split=c1)
        if training:
            for g in range(L.groups):
                zg = z[g * n:(g + 1) * n]
                mean, inv = zg.mean((0, 2, 3)), torch.rsqrt(zg.var((0, 2, 3), unbiased=False) + O.BN_EPS)
                assert float((mean - coef[0, g]).abs().max()) <= 1e-4 * float(zg.std()) + 1e-6, (L.name, 'mean')
                assert float(((inv - coef[1, g]) / inv).abs().max()) < 1e-4, (L.name, 'invstd')
            zdev = nchw64(L.y.torch() if plan.lazy_out[L.name] else plan.zbuf[L.name])
            ez = (zdev - zr).abs()
            row['z_err'] = float((ez / (ulp16(zr, kind) + noise)).max())
            row['z_share'] = float((ez > 0).double().mean())
            if c1:
                row['z_share_without_split_rounding'] = float(((zdev - r16(_conv64(x, w, b, L.dil, 0, kind)[0], kind)).abs() > 0).double().mean())
        if not (training and plan.lazy_out[L.name]):
            ydev = nchw64(L.y.torch())
            pre = zr * sc + sh if training else z * sc + sh
            pred = r16(lrelu32(pre), kind)
            dist = sc.abs() * ((ulp16(zr, kind) if training else 0.0) + noise)
            near = pre.abs() <= 2 * dist + ulp16(pre, kind)
            ey = (ydev - pred).abs()
            bound = ulp16(torch.maximum(pred.abs(), ydev.abs()), kind) + dist + torch.where(near, pre.abs(), torch.zeros_like(pre))
            row['y_err'] = float((ey / bound).max())
            row['y_share'] = float((ey > 0).double().mean())
            if training:
                row['y_share_without_z_rounding'] = float(((ydev - r16(lrelu32(z * sc + sh), kind)).abs() > 0).double().mean())
                if row['y_share_without_z_rounding'] > MIN_SENSITIVE_SHARE:
                    sensitive.append(L.name)
        rows.append(row)
    pools = {}
    for k, pv in plan.pooled.items():                   # a maximum of stored values: bit-exact
        pools[k] = bool(torch.equal(nchw64(pv.torch()), F.max_pool2d(nchw64(plan.enc_out[k - 1].values()), 2, 2)))
    ups = {}
    for k, dd in eng.backbone.dec_blocks().items():
        if dd.identity_up:
            continue
        src = logical_input(plan.low_src[k])
        size = (plan.cat[k].H, plan.cat[k].W)
        ref = r16(F.interpolate(src, size=size, mode='bilinear', align_corners=True), kind)
        # (fp32 source coordinates: their absolute error grows with the input size and moves the interpolation weights)
        noise = 2.0 ** -22 * (src.shape[2] + src.shape[3]) * F.interpolate(src.abs(), size=size, mode='bilinear', align_corners=True)
        e = (nchw64(plan.cat[k].torch()[..., :dd.up_ch]) - ref).abs()
        ups[k] = (float((e / (ulp16(ref, kind) + noise)).max()), float((e > 0).double().mean()))
    G._report(dict(kind='storage_oracle_per_layer_' + kind, tag=f'5-class 256x256 full width, bn_eval={bn_eval}', max_share=share_max,
                   layers=rows, sensitive_layers=sensitive, pools_exact=pools, upsample_err_ulp_share=ups))
    for row in rows:
        assert row.get('z_err', 0.0) <= 1.0 and row.get('y_err', 0.0) <= 1.0, row
        assert row.get('z_share', 0.0) <= share_max and row.get('y_share', 0.0) <= share_max, row
        if row['split'] and training:
            assert row['z_share_without_split_rounding'] > MIN_SENSITIVE_SHARE, row
    assert all(pools.values()), pools
    assert all(e <= 1.0 and sh_ <= share_max for e, sh_ in ups.values()), ups
    if training:
        assert sensitive, 'no layer shows the z rounding: the per-layer check would not see it missing'


# ------------------------------------------------------------------------------------------------ the whole step
# Bounds against the ROUNDED oracle, per (kind, eval-mode BatchNorm): about 3x the worst value measured on the MI355X over the
# geometries of that mode (parity report rows 'storage_oracle_step_*', profiles/r07_h16_oracle_parity_report.jsonl).
# Measured, train / eval BN -- logits (max-norm, the aux logits included): fp16 9.5e-3 / 9.5e-4, bf16 7.1e-2 / 7.8e-3;
# losses: fp16 4.3e-5 / 1.2e-7, bf16 4.4e-4 / 3.6e-7; worst parameter gradient (relative L2): fp16 2.3e-2 / 1.1e-2,
# bf16 7.6e-2 / 9.1e-3.
TOL_LOGITS = {('fp16', False): 2.8e-2, ('fp16', True): 2.8e-3, ('bf16', False): 2e-1, ('bf16', True): 2.3e-2}
TOL_LOSS = {('fp16', False): 1.3e-4, ('fp16', True): 4e-7, ('bf16', False): 1.3e-3, ('bf16', True): 1.1e-6}
TOL_GRAD = {('fp16', False): 7e-2, ('fp16', True): 3.2e-2, ('bf16', False): 2.2e-1, ('bf16', True): 2.7e-2}
# unrounded / rounded error (relative L2) of the backbone logits of both views.  Measured 1.9 - 2.5 in train-mode BN, 1.7 - 1.9
# in eval mode -- not an order of magnitude: a rounding is a step function, so an fp32-level difference that puts one element on
# the other side of a midpoint becomes a whole ulp there, and such differences multiply from layer to layer.  Two oracles that
# differ only in their own arithmetic (fp32 against fp64) diverge the same way; the per-layer test above
# is the one that tells a mis-modelled store from this.
MIN_GAIN = {False: 1.5, True: 1.4}


def _oracle_step(model, sd, batch, args, training, rounding):
    """One oracle step (fp32) on the start state, with the device's LeakyReLU branches and pool winners."""
    O.MASKS = device_masks(model)
    O.POOLS = device_pool_winners(model)
    O.STORAGE = rounding
    try:
        out, grads, _ = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training)
        stats = (sum(n for _, n, _ in O.MASK_STATS), sum(n for _, n, _ in O.POOL_STATS))
    finally:
        O.MASKS = O.POOLS = O.STORAGE = None
    return out, grads, stats


def _errors(dev_out, dev_grads, out, grads, training):
    e = {}
    for k in ('segmentation/logits', 'segmentation/logits_strong', 'logits_aux_cls'):
        e[k] = G.rel_err(dev_out[k].numpy(), out[k].double().numpy())
        e[k + ' (rel L2)'] = float((dev_out[k] - out[k].double()).norm() / out[k].double().norm())
    for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'):
        e[k] = abs(float(dev_out[k]) - float(out[k]))
    worst, wk = 0.0, None
    for k, g in grads.items():
        if g is None or (training and G.is_bias_before_bn(k)):
            continue
        ref = g.double()
        nrm = float(ref.norm())
        if nrm == 0.0:
            continue
        r = float((dev_grads[k] - ref).norm()) / nrm
        if r > worst:
            worst, wk = r, k
    e['grad_worst'], e['grad_worst_key'] = worst, wk
    return e


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('size,num_classes,bn_eval', [(256, 5, False), (224, 2, False), (256, 5, True)])
def test_training_step_against_the_rounded_oracle(kind, size, num_classes, bn_eval):
    """The geometries of test_training_step_in_16_bit_storage, one step each: logits, the five losses and every parameter
    gradient (LeakyReLU branches and max-pool winners aligned with the device's) against the oracle rounded at the plan's
    storage sites, and the same against the unrounded oracle; the first must be well below the second."""
    args, model, sd, batch = _setup(kind, size, num_classes, bn_eval)
    training = not bn_eval
    dev_out, dev_grads = _device_step(model, batch, args)
    rounding = rounding_for(model, kind, training)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, max(threads, 8)))
    try:
        r_out, r_grads, r_stats = _oracle_step(model, sd, batch, args, training, rounding)
        u_out, u_grads, u_stats = _oracle_step(model, sd, batch, args, training, None)
    finally:
        torch.set_num_threads(threads)
    missing = set(k for k, v in rounding.sites.items() if not k.endswith(':split')) - rounding.seen
    assert not missing, f'sites of the plan the oracle never reached: {sorted(missing)}'
    er = _errors(dev_out, dev_grads, r_out, r_grads, training)
    eu = _errors(dev_out, dev_grads, u_out, u_grads, training)
    G._report(dict(kind='storage_oracle_step_' + kind, tag=f'{num_classes}-class {size}x{size} full width, bn_eval={bn_eval}',
                   vs_rounded_oracle=er, vs_unrounded_oracle=eu,
                   branches_realigned=dict(rounded=r_stats, unrounded=u_stats), loss_scale=model.engine.last_plan.loss_scale))
    m = (kind, bn_eval)
    for k in ('segmentation/logits', 'segmentation/logits_strong', 'logits_aux_cls'):
        assert er[k] < TOL_LOGITS[m], (k, er[k])
    for k in ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory'):
        assert er[k] < TOL_LOSS[m], (k, er[k])
    assert er['grad_worst'] < TOL_GRAD[m], (er['grad_worst'], er['grad_worst_key'])
    for k in ('segmentation/logits (rel L2)', 'segmentation/logits_strong (rel L2)'):
        assert eu[k] > MIN_GAIN[bn_eval] * er[k], (k, er[k], eu[k])
