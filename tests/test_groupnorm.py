"""GroupNorm blocks (--norm_op group) without a GPU: module tree and state_dict keys, seeded initialisation, the flags of the
three drivers, the refusals, and the oracle with its normaliser patched to F.group_norm against nn.GroupNorm + autograd."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import pacing_oracle as O


def _unet(**kw):
    from pacingpseudo_amd.models import UNet
    return UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, **kw)


def test_group_norm_module_tree_and_keys():
    net = _unet(norm_op='group', norm_groups=8)
    bn = _unet()
    layers = [m for m in net.modules() if type(m).__name__ == 'ConvLayer']
    assert len(layers) == 22
    for m in layers:
        assert type(m.norm_op) is nn.GroupNorm and m.norm_op.num_groups == 8 and m.norm_op.affine
        assert m.norm_op.num_channels == m.conv.out_channels and m.norm_op.eps == 1e-5
    sd, sb = net.state_dict(), bn.state_dict()
    assert not any('running' in k or 'num_batches_tracked' in k for k in sd)
    assert set(sd) == {k for k in sb if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    assert 'enc_block1.conv_block.conv_layer1.norm_op.weight' in sd and 'dec_block1.conv_block.conv_layer2.norm_op.bias' in sd
    assert net.norm_kind == 'group' and bn.norm_kind == 'batch'


def test_group_norm_keeps_the_seeded_weights():
    """GroupNorm holders are built where BatchNorm's were and draw nothing from the generator: the same seed gives the same
    convolution weights as the BatchNorm network."""
    torch.manual_seed(5)
    a = _unet(norm_op='group', norm_groups=4).state_dict()
    torch.manual_seed(5)
    b = _unet().state_dict()
    for k, v in a.items():
        assert torch.equal(v, b[k]), k
    torch.manual_seed(5)
    c = _unet(norm_op='group', norm_groups=4).state_dict()
    assert all(torch.equal(v, c[k]) for k, v in a.items())


def test_conv_layer_takes_the_reference_callable():
    from pacingpseudo_amd.models.unet import ConvLayer
    m = ConvLayer(8, 16, norm_op=functools.partial(nn.GroupNorm, 4))
    assert type(m.norm_op) is nn.GroupNorm and m.norm_op.num_groups == 4
    assert type(ConvLayer(8, 16).norm_op) is nn.BatchNorm2d
    with pytest.raises(NotImplementedError):
        ConvLayer(8, 16, norm_op=nn.InstanceNorm2d)
    with pytest.raises(NotImplementedError):
        ConvLayer(8, 16, norm_op=functools.partial(nn.GroupNorm, 4, affine=False))


def test_group_count_must_divide_every_width():
    with pytest.raises(ValueError, match='norm_groups'):
        _unet(norm_op='group', norm_groups=3)
    with pytest.raises(ValueError, match='norm_groups'):
        _unet(norm_op='group', norm_groups=16)          # init_ch 8
    with pytest.raises(ValueError):
        _unet(norm_op='layer')
    _unet(norm_op='group', norm_groups=1)
    _unet(norm_op='group', norm_groups=8)


def test_strided_variant_is_refused():
    from pacingpseudo_amd.models import UNet
    with pytest.raises(NotImplementedError):
        UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=16, is_stride_conv=True, is_trans_conv=True,
             norm_op='group')


def test_consistency_model_passes_the_norm_through():
    from pacingpseudo_amd.models import ConsistencyRegulr
    args = O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    m = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, is_stride_conv=False,
                         is_trans_conv=False, elab_end_points=True, norm_op='group', norm_groups=8),
        kwargs_aux_path=dict(num_classes=5, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=16, aux_drop_prob=0.0,
                             do_memory=True, max_step=400, update_momentum=0.9, ensemble_mode='cosine_similarity'),
        args_parser=args)
    sd = m.state_dict()
    assert 'backbone.enc_block3.conv_block.conv_layer2.norm_op.weight' in sd
    assert not any(k.startswith('backbone.') and 'running' in k for k in sd)
    assert 'aux_path.layer_bottleneck.2.running_mean' in sd        # the auxiliary bottleneck keeps nn.BatchNorm2d
    assert all(L.gn for L in m.engine.layers) and not m.engine.aux_layer.gn
    args.storage = 'fp16'
    with pytest.raises(NotImplementedError, match='norm_op group'):
        ConsistencyRegulr(kwargs_unet=dict(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8, norm_op='group'),
                          kwargs_aux_path=dict(num_classes=5, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=16,
                                               aux_drop_prob=0.0, do_memory=True, max_step=400, update_momentum=0.9,
                                               ensemble_mode='cosine_similarity'),
                          args_parser=args)


def test_flags_and_defaults():
    from pacingpseudo_amd.inference import parser as inf_parser
    from pacingpseudo_amd.models.unet import norm_kwargs
    from pacingpseudo_amd.train import apply_dataset_preset, parser as train_parser
    from pacingpseudo_amd.upper_bound import parser as ub_parser
    for p, base in ((train_parser, ['--tag', 't']), (ub_parser, ['--tag', 't']),
                    (inf_parser, ['--fold', '0', '--checkpoint_file', 'x'])):
        a = p.parse_args(base)
        assert a.norm_op == 'batch' and a.norm_groups == 8
        assert norm_kwargs(a) == {}
        a = p.parse_args(base + ['--norm_op', 'group', '--norm_groups', '4'])
        assert norm_kwargs(a) == dict(norm_op='group', norm_groups=4)
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--norm_op', 'instance'])
    # the abbreviation an existing test relies on still resolves
    ns = apply_dataset_preset(train_parser.parse_args(['--tag', 't', '--dataset', 'acdc', '--image_s', '192']))
    assert ns.image_size == 192


def test_mismatched_checkpoint_names_the_flag():
    from pacingpseudo_amd.inference import load_backbone
    from pacingpseudo_amd.models.unet import checkpoint_norm_kind
    gn, bn = _unet(norm_op='group'), _unet()
    assert checkpoint_norm_kind(gn.state_dict()) == 'group' and checkpoint_norm_kind(bn.state_dict()) == 'batch'
    full = {'backbone.' + k: v for k, v in gn.state_dict().items()}
    full['aux_path.layer_bottleneck.2.running_mean'] = torch.zeros(4)
    assert checkpoint_norm_kind(full) == 'group'
    with pytest.raises(ValueError, match='--norm_op group'):
        load_backbone(_unet(), gn.state_dict())
    with pytest.raises(ValueError, match='--norm_op batch'):
        load_backbone(_unet(norm_op='group'), bn.state_dict())
    load_backbone(_unet(norm_op='group'), full)                   # the matching kind loads (full-model checkpoint)


@pytest.fixture
def gn_oracle(monkeypatch):
    orig = O._bn

    def _bn(sd, prefix, x, training):
        if prefix + '.running_mean' in sd:
            return orig(sd, prefix, x, training)
        return F.group_norm(x, 4, sd[prefix + '.weight'], sd[prefix + '.bias'], 1e-5)
    monkeypatch.setattr(O, '_bn', _bn)


def test_patched_oracle_matches_group_norm_modules(gn_oracle):
    """The oracle's U-Net with the patched normaliser = the same network assembled from nn modules (nn.GroupNorm), forward and
    autograd gradients, in fp64."""
    torch.manual_seed(2)
    net = _unet(norm_op='group', norm_groups=4).double()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k in sd:                                                # non-trivial affine parameters
        if '.norm_op.' in k:
            sd[k] += torch.randn_like(sd[k]) * 0.1
    net.load_state_dict(sd)
    args = O.default_args(init_ch=8, max_ch=64)
    x = torch.randn(2, 1, 32, 32, dtype=torch.float64)

    def layer(m, t):
        return F.leaky_relu(m.norm_op(m.conv(t)), 0.01)

    def dconv(b, t):
        return layer(b.conv_block.conv_layer2, layer(b.conv_block.conv_layer1, t))

    def modules_forward(t):
        skips = []
        for e in net.enc_blocks():
            if e.pooling is not None:
                t = F.max_pool2d(t, 2, 2)
            t = dconv(e, t)
            skips.append(t)
        low = skips[5]
        for k in (5, 4, 3, 2, 1):
            d = net.dec_blocks()[k]
            up = F.interpolate(low, scale_factor=d.scale, mode='bilinear', align_corners=True)
            low = dconv(d, torch.cat((up, skips[k - 1]), 1))
        return F.conv2d(low, net.final_conv.weight, net.final_conv.bias)

    ref = modules_forward(x)
    sd_o = {'backbone.' + k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    got = O.unet_forward(sd_o, x, args, True)['segmentation/logits']
    assert float((got - ref).abs().max()) < 1e-10 * float(ref.abs().max())
    w = torch.randn_like(ref)
    (ref * w).sum().backward()
    (got * w).sum().backward()
    params = dict(net.named_parameters())
    for k, p in params.items():
        assert float((sd_o['backbone.' + k].grad - p.grad).abs().max()) <= 1e-9 * max(1.0, float(p.grad.abs().max())), k
