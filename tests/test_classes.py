"""Class counts beyond the reference's data sets (no GPU): the modules build for 1 <= K <= 32 and refuse K > 32 before any
buffer exists; the drivers' flags take the class count as given; the 16-bit headers match the sources."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aux_kwargs(K):
    from pacingpseudo_amd.data import full_flags
    return dict(num_classes=K, feat_stage=full_flags().feat_stage, feat_ch=[64, 64], hid_ch=16, aux_drop_prob=0.0,
                do_memory=True, max_step=10, update_momentum=0.9, ensemble_mode='cosine_similarity')


def _model(K):
    from pacingpseudo_amd.data import full_flags
    from pacingpseudo_amd.models import ConsistencyRegulr
    args = full_flags(num_classes=K, ignored_index=K, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    return ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                         elab_end_points=True),
        kwargs_aux_path=_aux_kwargs(K), args_parser=args)


@pytest.mark.parametrize('K', [1, 9, 17, 32])
def test_modules_build_up_to_32_classes(K):
    from pacingpseudo_amd.models import AuxPath, UNet
    net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, elab_end_points=True)
    assert net.final_conv.weight.shape[0] == K
    aux = AuxPath(**_aux_kwargs(K))
    assert aux.memory_bank.shape[0] == K and aux.fc_cls[1].weight.shape[0] == K
    m = _model(K)
    assert m.backbone.final_conv.weight.shape[0] == K


@pytest.mark.parametrize('K', [33, 64])
def test_more_than_32_classes_are_refused(K):
    from pacingpseudo_amd.models import AuxPath, UNet
    with pytest.raises(NotImplementedError, match=r'at most 32 classes.*--num_classes'):
        UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, elab_end_points=True)
    with pytest.raises(NotImplementedError, match=r'at most 32 classes.*--num_classes'):
        AuxPath(**_aux_kwargs(K))
    with pytest.raises(NotImplementedError, match='32'):
        _model(K)


def test_zero_classes_is_a_value_error():
    from pacingpseudo_amd.models import UNet
    with pytest.raises(ValueError, match='num_classes'):
        UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=0, output_stride=8)


def test_train_parser_takes_the_class_count_as_given():
    from pacingpseudo_amd.train import apply_dataset_preset, parser
    a = apply_dataset_preset(parser.parse_args(['--tag', 't', '--num_classes', '17', '--ignored_index', '17']))
    assert a.num_classes == 17 and a.ignored_index == 17
    from pacingpseudo_amd.upper_bound import parser as ub_parser
    b = apply_dataset_preset(ub_parser.parse_args(['--tag', 't', '--num_classes', '32', '--ignored_index', '32']))
    assert b.num_classes == 32 and b.ignored_index == 32


def test_inference_parser_has_num_classes():
    from pacingpseudo_amd.inference import parser
    a = parser.parse_args(['--fold', '1', '--checkpoint_file', 'x', '--num_classes', '17'])
    assert a.num_classes == 17
    assert parser.parse_args(['--fold', '1', '--checkpoint_file', 'x']).num_classes is None


def test_inference_refuses_a_checkpoint_of_another_class_count():
    import torch
    from pacingpseudo_amd.inference import load_backbone
    from pacingpseudo_amd.models import UNet
    src = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=17, output_stride=8)
    dst = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=5, output_stride=8)
    sd = {'backbone.' + k: v for k, v in src.state_dict().items()}
    with pytest.raises(ValueError, match='--num_classes 17'):
        load_backbone(dst, sd)
    load_backbone(UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=17, output_stride=8), sd)
    assert torch.equal(src.final_conv.weight, src.state_dict()['final_conv.weight'])


def test_16_bit_headers_match_the_sources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'gen_h16_header.py'), '--check'], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
