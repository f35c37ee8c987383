"""GroupNorm blocks (--norm_op group) on the GPU: the kernels against fp64 torch, the whole step against the CPU oracle with its
normaliser patched to F.group_norm, and the properties that follow from per-image statistics.

Run on the GPU box:  python -m pytest tests/test_gpu_groupnorm.py -m gpu -q
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests.test_gpu_step import device_masks, device_pool_winners, iteration, oracle_with_device_branches  # noqa: E402,F401

SLOPE = 0.01


def dev():
    return torch.device('cuda', 0)


def build_gn_model(args, groups=8):
    from pacingpseudo_amd.models import ConsistencyRegulr
    return ConsistencyRegulr(
        kwargs_unet=dict(input_ch=args.input_ch, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=args.num_classes,
                         output_stride=args.output_stride, is_stride_conv=False, is_trans_conv=False, elab_end_points=True,
                         norm_op='group', norm_groups=groups),
        kwargs_aux_path=dict(num_classes=args.num_classes, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=args.hid_ch,
                             aux_drop_prob=args.aux_drop_prob, do_memory=args.do_memory, max_step=args.epoch,
                             update_momentum=args.update_momentum, ensemble_mode=args.ensemble_mode),
        args_parser=args).cuda()


@pytest.fixture
def gn_oracle(monkeypatch):
    """The oracle's block normaliser with GroupNorm for every prefix that has no running statistics (the GroupNorm holders);
    BatchNorm prefixes (the auxiliary bottleneck) fall through to the original."""
    orig = O._bn
    groups = {}

    def _bn(sd, prefix, x, training):
        if prefix + '.running_mean' in sd:
            return orig(sd, prefix, x, training)
        return F.group_norm(x, groups['G'], sd[prefix + '.weight'], sd[prefix + '.bias'], 1e-5)
    monkeypatch.setattr(O, '_bn', _bn)

    def set_groups(g):
        groups['G'] = g
    return set_groups


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------- kernels
def _gn_problem(G_, N, H, W, C=32, ld=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(N, H, W, ld)
    z[..., :C] = torch.randn(N, H, W, C, generator=g) * 1.7 + torch.randn(1, 1, 1, C, generator=g) * 0.8 + 0.3
    z[..., C:] = float('nan')                                  # outside the channel slice: never read
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    dy = torch.randn(N, H, W, ld, generator=g)
    dp = torch.randn(N, H // 2, W // 2, ld, generator=g)
    return z, gamma, beta, dy, dp


def _run_kernels(G_, N, H, W, z, gamma, beta, dy, dp, C=32, ld=40, pool=False):
    from pacingpseudo_amd._lib import lib, stream_ptr
    st = stream_ptr()
    HW = H * W
    zd, gd, bd, dyd, dpd = (t.to(dev()) for t in (z, gamma, beta, dy, dp))
    coef = torch.zeros(5, N, C, device=dev())
    mean, invstd, scale, shift, xbar = (coef[i].data_ptr() for i in range(5))
    nws = lib.pp_gn_workspace(C, HW, N)
    ws = torch.zeros(nws, dtype=torch.uint8, device=dev())
    lib.pp_gn_stats(zd.data_ptr(), ld, C, HW, N, G_, 1e-5, gd.data_ptr(), bd.data_ptr(), mean, invstd, xbar, scale, shift,
                    ws.data_ptr(), nws, st)
    y = torch.full((N, H, W, ld), 7.0, device=dev())
    lib.pp_bn_lrelu_fwd(zd.data_ptr(), ld, scale, shift, y.data_ptr(), ld, C, HW, N, SLOPE, st)
    dz = torch.full((N, H, W, ld), 5.0, device=dev())
    dg, db, dbc = (torch.full((C,), 9.0, device=dev()) for _ in range(3))
    amax = torch.full((1,), -1.0, device=dev())
    if pool:
        yp = torch.full((N, H // 2, W // 2, ld), 7.0, device=dev())
        y2 = torch.full((N, H, W, ld), 7.0, device=dev())
        lib.pp_bn_lrelu_fwd_pool(zd.data_ptr(), ld, scale, shift, y2.data_ptr(), ld, yp.data_ptr(), ld, C, N, H, W, N, SLOPE, st)
        assert torch.equal(y2[..., :C], y[..., :C])
        lib.pp_gn_lrelu_bwd_pool(dyd.data_ptr(), ld, dpd.data_ptr(), ld, zd.data_ptr(), ld, scale, shift, mean, invstd, xbar,
                                 gd.data_ptr(), dz.data_ptr(), ld, dg.data_ptr(), db.data_ptr(), dbc.data_ptr(), 0, C, N, H, W, G_,
                                 SLOPE, ws.data_ptr(), nws, amax.data_ptr(), st)
    else:
        yp = None
        lib.pp_gn_lrelu_bwd(dyd.data_ptr(), ld, zd.data_ptr(), ld, scale, shift, mean, invstd, xbar, gd.data_ptr(), dz.data_ptr(),
                            ld, dg.data_ptr(), db.data_ptr(), dbc.data_ptr(), 0, C, HW, N, G_, SLOPE, ws.data_ptr(), nws,
                            amax.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.all(y[..., C:] == 7.0) and torch.all(dz[..., C:] == 5.0), 'wrote outside the channel slice'
    return dict(y=y[..., :C].cpu(), yp=None if yp is None else yp[..., :C].cpu(), dz=dz[..., :C].cpu(), dg=dg.cpu(), db=db.cpu(),
                dbc=dbc.cpu(), amax=float(amax))


@pytest.mark.parametrize('G_,N,H,W,pool', [(1, 1, 24, 40, False), (8, 3, 24, 40, False), (32, 3, 64, 64, False),
                                           (8, 1, 64, 64, True), (32, 3, 24, 40, True), (1, 3, 64, 64, True)])
def test_groupnorm_kernels_against_fp64(G_, N, H, W, pool):
    C = 32
    z, gamma, beta, dy, dp = _gn_problem(G_, N, H, W)
    got = _run_kernels(G_, N, H, W, z, gamma, beta, dy, dp, pool=pool)
    # fp64 reference; the LeakyReLU branch of every element as the device took it (y > 0)
    z64 = z[..., :C].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    pre = F.group_norm(z64, G_, gamma.double(), beta.double(), 1e-5)
    ref_y = F.leaky_relu(pre, SLOPE)
    assert rel(got['y'].permute(0, 3, 1, 2), ref_y) < 1e-5
    mask = got['y'].permute(0, 3, 1, 2) > 0
    gy = dy[..., :C].double().permute(0, 3, 1, 2).clone()
    if pool:
        yd = got['y'].permute(0, 3, 1, 2)
        Nn, Cc, Hh, Ww = yd.shape
        win = yd.reshape(Nn, Cc, Hh // 2, 2, Ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Nn, Cc, Hh // 2, Ww // 2, 4)
        assert torch.equal(got['yp'].permute(0, 3, 1, 2), win.max(-1).values)
        idx = win.argmax(-1)                                       # first maximum: the device's winner
        add = torch.zeros(Nn, Cc, Hh // 2, Ww // 2, 4, dtype=torch.float64)
        add.scatter_(-1, idx[..., None], dp[..., :C].double().permute(0, 3, 1, 2)[..., None])
        gy += add.reshape(Nn, Cc, Hh // 2, Ww // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Nn, Cc, Hh, Ww)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z64.grad = None
    pre = F.group_norm(z64, G_, g64, b64, 1e-5)
    torch.where(mask, pre, pre * SLOPE).backward(gy)
    dz_ref = z64.grad
    assert rel(got['dz'].permute(0, 3, 1, 2), dz_ref) < 1e-4
    assert rel(got['dg'], g64.grad) < 1e-4
    assert rel(got['db'], b64.grad) < 1e-4
    # the conv-bias gradient: sum of dz per channel (exactly 0 in theory when every channel is its own group, so the scale is
    # also bounded below by the sum of |dz|)
    ref_b = dz_ref.sum((0, 2, 3))
    scale_b = max(float(ref_b.abs().max()), 1e-3 * float(dz_ref.abs().sum((0, 2, 3)).max()))
    assert float((got['dbc'].double() - ref_b).abs().max()) < 1e-4 * scale_b
    assert got['amax'] == float(got['dz'].abs().max())
    # deterministic: a second launch is bit-identical
    again = _run_kernels(G_, N, H, W, z, gamma, beta, dy, dp, pool=pool)
    for k in ('y', 'dz', 'dg', 'db', 'dbc'):
        assert torch.equal(got[k], again[k]), k


# ---------------------------------------------------------------------------------------------------------- whole step
def _small_args(**over):
    return O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], **over)


def _trainable(sd):
    return O.trainable_keys(sd)


@pytest.mark.parametrize('B,S,width', [(2, 64, 'small'), (4, 256, 'small'), (2, 64, 'full')])
def test_groupnorm_step_against_oracle(gn_oracle, B, S, width):
    """Full flags, small net (and once at the real widths 32..512, where the Winograd and split-fp16 kernels run): outputs,
    branch-aligned gradients (conv biases included: GroupNorm does not cancel them per channel) and post-Adam weights against
    the oracle with F.group_norm blocks."""
    from pacingpseudo_amd.optim import FusedAdam
    gn_oracle(8)
    args = _small_args() if width == 'small' else O.full_flags()
    torch.manual_seed(1)
    model = build_gn_model(args)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert not any(k.endswith('norm_op.running_mean') for k in sd)
    batch = O.synthetic_batch(B, S, S, seed=3, keep=0.05)
    opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
    ref_out, _, ref_total = O.train_step({k: v.clone() for k, v in sd.items()}, batch, 0, args, training=True)
    rec, grads = iteration(model, opt, batch, args, 0)
    for k, v in ref_out.items():
        if k.startswith('_') or not torch.is_tensor(v):
            continue
        e = G.rel_err(rec[k].double().cpu().numpy(), v.numpy())
        assert e < 1e-4, f'{k}: rel err {e:.3e}'
    assert abs(float(rec['total_loss']) - ref_total) < 1e-4 * max(1.0, abs(ref_total))
    _, og, _ = oracle_with_device_branches(model, {k: v.clone() for k, v in sd.items()}, batch, 0, args, True)
    # conv biases whose gradient vanishes exactly: in front of the auxiliary bottleneck's train-mode BatchNorm, and in front of
    # a GroupNorm with one channel per group (C = 8 at init_ch 8: the per-image channel mean is removed, as in InstanceNorm)
    widths = {k.rsplit('.conv.', 1)[0]: v.shape[0] for k, v in sd.items() if k.endswith('.conv.weight')}
    zero = {k for k in og if k == 'aux_path.layer_bottleneck.1.bias' or (k.endswith('.conv.bias') and widths[k[:-10]] == 8)}
    tols = {'backbone.final_conv.bias': 1e-3}       # a sum over every pixel of largely cancelling loss gradients
    bad = []
    for k, v in og.items():
        if v is None:
            continue
        assert grads.get(k) is not None, k
        got = grads[k].double().cpu().numpy()
        if k in zero:
            assert np.max(np.abs(got)) < 2e-5, k
            continue
        e = G.rel_err(got, v.numpy())
        if not e < tols.get(k, 2e-4):
            bad.append((e, k))
    assert not bad, sorted(bad, reverse=True)[:8]
    gb = grads['backbone.enc_block3.conv_block.conv_layer1.conv.bias']
    assert float(gb.abs().max()) > 1e-6                             # with two or more channels per group the conv bias does learn
    # post-Adam weights: the oracle's Adam on the start state with the device gradients
    adam = O.AdamState()
    post = {k: v.clone() for k, v in sd.items()}
    adam.step(post, {k: (grads[k].cpu() if grads.get(k) is not None else None) for k in _trainable(sd)}, args.lr, args.wd)
    now = model.state_dict()
    for k in _trainable(sd):
        if grads.get(k) is None:
            continue
        ref = post[k]
        assert float((now[k].cpu() - ref).abs().max()) <= 2e-7 * max(1.0, float(ref.abs().max())) + 1e-9, k


def test_groupnorm_per_image_independence():
    """An image's logits do not depend on the other images of the batch (per-image statistics), in train and eval mode."""
    from pacingpseudo_amd.models import UNet
    torch.manual_seed(1)
    net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, norm_op='group', norm_groups=8).cuda()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 1, 64, 64, generator=g)
    x2 = x.clone()
    x2[1:] = torch.randn(2, 1, 64, 64, generator=g) * 3 + 1
    for train in (True, False):
        net.train(train)
        with torch.no_grad():
            a = net(x.cuda())['segmentation/logits'].clone()
            b = net(x2.cuda())['segmentation/logits'].clone()
            one = net(x[:1].cuda())['segmentation/logits'].clone()
        assert torch.equal(a[0], b[0])
        assert not torch.equal(a[1], b[1])
        assert rel(one[0], a[0]) < 1e-5


def test_groupnorm_control_train_equals_eval():
    """--session Control (no auxiliary path): no BatchNorm layer is left, so train- and eval-mode logits are bit-identical."""
    args = O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    torch.manual_seed(1)
    model = build_gn_model(args)
    b = {k: v.cuda() for k, v in O.synthetic_batch(2, 64, 64, seed=4, keep=0.05).items() if k != 'label'}
    model.train()
    with torch.no_grad():
        t = model(b, mode='val')['segmentation/logits'].clone()
    model.eval()
    with torch.no_grad():
        e = model(b, mode='val')['segmentation/logits'].clone()
    assert torch.equal(t, e)


def test_groupnorm_steps_are_deterministic_and_graph_replay_matches():
    """Two eager steps from the same state are bit-identical, and so is a GraphedStep replay."""
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    from tests.test_gpu_graph import _eager_step, _loss_fn
    args = _small_args()
    f = _loss_fn(args)
    b = {k: v.cuda() for k, v in O.synthetic_batch(2, 64, 64, seed=5, keep=0.05).items() if k != 'label'}
    runs = {}
    for tag in ('eager1', 'eager2', 'graph'):
        torch.manual_seed(1)
        model = build_gn_model(args)
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)
        gs = GraphedStep(model, opt, f, warmup=1) if tag == 'graph' else None
        model.train()
        losses = []
        for _ in range(3):
            if gs is None:
                losses.append(_eager_step(model, opt, f, b, 0))
            else:
                loss, _ = gs(b, 0)
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        runs[tag] = (torch.stack(losses).cpu(), {k: v.detach().clone() for k, v in model.state_dict().items()})
        if gs is not None:
            assert gs.replays == 2, gs.replays
    for tag in ('eager2', 'graph'):
        assert torch.equal(runs['eager1'][0], runs[tag][0]), tag
        for k, v in runs['eager1'][1].items():
            assert torch.equal(v, runs[tag][1][k]), (tag, k)


def test_groupnorm_train_and_inference_cli(tmp_path):
    """train_chaos.py --norm_op group writes a GroupNorm checkpoint; inference.py --norm_op group evaluates it, and without
    the flag the mismatch is reported by name."""
    import glob
    import os
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'out')
    vd = train_main(['--tag', 'gn', '--session', 'Experiment', '--root', root, '--synthetic', '16', '--epoch', '1', '--batch_size', '4',
                     '--image_size', '64', '--num_workers', '0', '--cpu_input', '--do_loss_ent', '--do_decoder_consistency',
                     '--do_aux_path', '--do_memory', '--norm_op', 'group', '--norm_groups', '4'])
    assert np.isfinite(vd).all()
    ck = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-gn', 'ckps', 'ckp_0.pth'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu')
    assert 'backbone.enc_block1.conv_block.conv_layer1.norm_op.weight' in sd
    assert not any(k.startswith('backbone.') and 'running' in k for k in sd)
    common = ['--fold', '1', '--checkpoint_file', ck[0], '--dataset', 'chaost1', '--root', str(tmp_path / 'inf'), '--synthetic', '4',
              '--image_size', '64', '--batch_size', '2', '--num_workers', '0']
    dicearr, hd95arr = I.main(common + ['--norm_op', 'group', '--norm_groups', '4'])
    assert dicearr.shape == (4, 5)
    with pytest.raises(ValueError, match='--norm_op'):
        I.main(common)


def test_groupnorm_refuses_16bit_storage():
    args = _small_args()
    args.storage = 'bf16'
    with pytest.raises(NotImplementedError):
        build_gn_model(args)
