"""--cr_teacher {none,ema}: the host side of the mean-teacher consistency term (no GPU).  The flag and its cross-flag checks, the
resume comparison, and that the feature bound no new entry point: the teacher's forward runs the existing convolution,
normalisation and head kernels from a second weight source, its loss the existing fused loss kernels twice."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ['--tag', 'x']


def test_flag_parses_and_defaults_to_none():
    from pacingpseudo_amd.train import parse_args, parser
    assert parser.parse_args(BASE).cr_teacher == 'none'
    assert parse_args(BASE).cr_teacher == 'none'
    a = parse_args(BASE + ['--cr_teacher', 'ema', '--do_decoder_consistency', '--ema_decay', '0.99'])
    assert a.cr_teacher == 'ema' and a.detach_weak_cr is False
    # --detach_weak_cr is accepted beside it (it has nothing left to do: the teacher never receives a gradient)
    a = parse_args(BASE + ['--cr_teacher', 'ema', '--do_decoder_consistency', '--ema_decay', '0.9', '--detach_weak_cr'])
    assert a.cr_teacher == 'ema' and a.detach_weak_cr is True


def test_other_values_are_refused(capsys):
    from pacingpseudo_amd.train import parser
    with pytest.raises(SystemExit) as e:
        parser.parse_args(BASE + ['--cr_teacher', 'live'])
    assert e.value.code == 2 and '--cr_teacher' in capsys.readouterr().err


def test_upper_bound_driver_has_no_such_flag(capsys):
    from pacingpseudo_amd.upper_bound import parser
    with pytest.raises(SystemExit) as e:
        parser.parse_args(BASE + ['--cr_teacher', 'ema'])
    assert e.value.code == 2 and 'cr_teacher' in capsys.readouterr().err


@pytest.mark.parametrize('argv,needs', [(['--do_decoder_consistency'], '--ema_decay'),
                                        (['--do_decoder_consistency', '--ema_decay', '0'], '--ema_decay'),
                                        (['--ema_decay', '0.99'], '--do_decoder_consistency'), ([], '--do_decoder_consistency')])
def test_ema_teacher_without_its_two_flags_is_refused_before_any_device_call(argv, needs, capsys, monkeypatch):
    """A usage error of the parser (exit status 2, the missing flag named), raised while parsing: no model, no optimizer and no
    device call exists yet -- torch.cuda.set_device and the model class are rigged to fail the test if they are reached."""
    import pacingpseudo_amd.models as M
    from pacingpseudo_amd import train

    def reached(*a, **k):
        raise AssertionError('the device was touched before the flags were refused')
    monkeypatch.setattr(torch.cuda, 'set_device', reached)
    monkeypatch.setattr(M, 'ConsistencyRegulr', reached)
    with pytest.raises(SystemExit) as e:
        train.train_main(BASE + ['--cr_teacher', 'ema', '--synthetic', '4'] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and '--cr_teacher ema' in err and needs in err, err


def test_attach_teacher_refuses_without_consistency_or_ema():
    """The model-level checks, on the CPU: no consistency term -> ValueError before anything else is looked at."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd.models import ConsistencyRegulr
    from pacingpseudo_amd.optim import FusedAdam
    args = O.default_args(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    assert not args.do_decoder_consistency
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=8, max_ch=64, num_classes=args.num_classes, output_stride=8, elab_end_points=True),
        kwargs_aux_path=dict(num_classes=args.num_classes, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=16,
                             aux_drop_prob=0.0, do_memory=False, max_step=args.epoch, update_momentum=0.9,
                             ensemble_mode=args.ensemble_mode),
        args_parser=args)
    opt = FusedAdam(model.parameters(), lr=1e-3, ema_decay=0.9)
    with pytest.raises(ValueError, match='--do_decoder_consistency'):
        model.attach_teacher(opt)
    assert model.engine.teacher is None
    assert model.attach_teacher(None) is model and model.engine.teacher is None and model.engine.teacher_key() is None
    # the key list of a training-mode forward grows by the teacher logits only while a teacher is attached
    args.do_decoder_consistency = True
    keys = model._expected_keys('train')
    assert 'segmentation/logits_teacher' not in keys
    model.engine.teacher = {}
    on = model._expected_keys('train')
    assert on == keys[:keys.index('segmentation/logits_strong') + 1] + ['segmentation/logits_teacher'] + keys[keys.index('segmentation/logits_strong') + 1:]
    assert 'segmentation/logits_teacher' not in model._expected_keys('val')


def test_ema_shadow_needs_ema_decay():
    from pacingpseudo_amd.optim import FusedAdam, FusedSGD
    p = torch.nn.Parameter(torch.zeros(4))
    for opt in (FusedAdam([p], lr=1e-3), FusedSGD([p], lr=1e-3, momentum=0.9)):
        with pytest.raises(ValueError, match='ema_decay is off'):
            opt.ema_shadow(object())


def test_resume_compares_the_flag_and_reads_an_older_file_as_none():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    assert resume.ABSENT_DEFAULTS['cr_teacher'] == 'none' and 'cr_teacher' not in resume.MAY_DIFFER
    common = BASE + ['--do_decoder_consistency', '--ema_decay', '0.99']
    none = resume.flag_dict(apply_dataset_preset(parse_args(common)))
    ema = resume.flag_dict(apply_dataset_preset(parse_args(common + ['--cr_teacher', 'ema'])))
    assert none['cr_teacher'] == 'none' and ema['cr_teacher'] == 'ema'
    resume.check_compatible(none, dict(none), 1, 1)
    resume.check_compatible(ema, dict(ema), 1, 1)
    with pytest.raises(resume.ResumeError, match=r"--cr_teacher \(saved 'none', now 'ema'\)"):
        resume.check_compatible(none, ema, 1, 1)
    with pytest.raises(resume.ResumeError, match=r"--cr_teacher \(saved 'ema', now 'none'\)"):
        resume.check_compatible(ema, none, 1, 1)
    # a state file written before the flag existed computed what 'none' computes
    old = {k: v for k, v in none.items() if k != 'cr_teacher'}
    resume.check_compatible(old, none, 1, 1)
    with pytest.raises(resume.ResumeError, match=r"--cr_teacher \(saved 'none', now 'ema'\)"):
        resume.check_compatible(old, ema, 1, 1)


def test_cli_keeps_every_reference_flag():
    from tests.test_host_logic import test_cli_keeps_every_reference_flag as check
    check()


def test_no_entry_point_was_added():
    """254 bound entry points, 254 exported symbols, library version 606: what the parent has.  The feature changed no device
    code, so the version did not move, and it declared nothing new in the header."""
    from pacingpseudo_amd import _lib
    assert len(_lib._PROTOS) == 254 and len(_lib.EXPORTED_SYMBOLS) == 254 and set(_lib._PROTOS) == set(_lib.EXPORTED_SYMBOLS)
    assert not [n for n in _lib._PROTOS if 'teacher' in n]
    assert _lib.MIN_LIB_VERSION == 606
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == 606
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    assert 'teacher' not in header


def test_functional_loss_is_exported_and_checks_its_arguments():
    import pacingpseudo_amd.losses as L
    from pacingpseudo_amd.losses.losses import _VARIANT
    f = L.teacher_consistency_loss
    z = torch.zeros(2, 5, 8, 8)
    with pytest.raises(TypeError, match='student_logits must be a 4-D float32 CUDA tensor'):
        f(z, z)
    assert sorted(_VARIANT) == sorted(['ce_loss', 'l1_loss', 'l2_loss', 'kl_loss', 'bikl_loss', 'js_loss', 'hard_ce_loss'])


def test_variant_zero_never_stores_the_strong_gradient():
    """The two-call loss leans on this: with cr_variant 0 the backward kernels leave dlogits_s alone, so the student call cannot
    overwrite what the teacher call writes there.  Both kernels store dzs under `if (variant)` and nowhere else."""
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_loss.hip')).read()
    body = src[src.index('void seg_losses_bwd_kernel('):src.index('extern "C" int pp_seg_losses_bwd(')]
    stores = [ln.strip() for ln in body.splitlines() if re.search(r'\bdzs\b.*=[^=]', ln) and 'const' not in ln and '__restrict__' not in ln]
    assert len(stores) == 2 and all(s.startswith('if (variant)') for s in stores), stores
