"""--ema_decay / ema_decay without a GPU: the three parsers, the optimizers' argument checks and state dicts, resume compatibility
with state files older than the flags, the C ABI of the new entry points and the host restatement of the warm-up weight."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('driver', ['train', 'upper_bound'])
def test_training_parsers_accept_the_flags(driver, capsys):
    """Default 0 (off) and interval 1; a decay outside [0, 1) or an interval below 1 is an argparse error (exit status 2)."""
    import importlib
    parser = importlib.import_module(f'pacingpseudo_amd.{driver}').parser
    a = parser.parse_args(['--tag', 'x'])
    assert a.ema_decay == 0.0 and a.ema_val_interval == 1
    a = parser.parse_args(['--tag', 'x', '--ema_decay', '0.999', '--ema_val_interval', '5'])
    assert a.ema_decay == 0.999 and a.ema_val_interval == 5
    for flag, bad in (('--ema_decay', '1'), ('--ema_decay', '-0.1'), ('--ema_decay', 'nan'), ('--ema_decay', '1.5'),
                      ('--ema_val_interval', '0')):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['--tag', 'x', flag, bad])
        assert e.value.code == 2
        assert flag in capsys.readouterr().err


def test_inference_parser_accepts_the_flag():
    from pacingpseudo_amd.inference import parser
    base = ['--fold', '1', '--checkpoint_file', 'runs/fold1']
    assert parser.parse_args(base).ema is False
    a = parser.parse_args(base + ['--ema', '--best_ckp'])
    assert a.ema is True and a.best_ckp is True


def _opt(cls, **kw):
    from pacingpseudo_amd import optim
    p = torch.nn.Parameter(torch.zeros(4))
    extra = dict(momentum=0.9) if cls == 'FusedSGD' else {}
    return getattr(optim, cls)([p], lr=1e-3, **extra, **kw)


@pytest.mark.parametrize('cls', ['FusedAdam', 'FusedSGD'])
def test_optimizers_validate_and_carry_ema_decay(cls):
    for bad in (0, 0.0, 1, 1.0, -0.5, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            _opt(cls, ema_decay=bad)
    assert _opt(cls).param_groups[0]['ema_decay'] is None
    assert _opt(cls, ema_decay=None).param_groups[0]['ema_decay'] is None
    on = _opt(cls, ema_decay=0.9)
    assert on.param_groups[0]['ema_decay'] == 0.9
    sd = on.state_dict()
    assert sd['param_groups'][0]['ema_decay'] == 0.9
    other = _opt(cls)
    other.load_state_dict(sd)
    assert other.param_groups[0]['ema_decay'] == 0.9
    # a state dict written before the key existed: off, whatever the optimizer was built with
    old = {'param_groups': [{k: v for k, v in sd['param_groups'][0].items() if k != 'ema_decay'}], 'slabs': []}
    on.load_state_dict(old)
    assert on.param_groups[0]['ema_decay'] is None
    # off: the context refuses without touching a device
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        with _opt(cls).ema_weights():
            pass


def test_resume_accepts_state_files_older_than_the_flags():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parser
    assert resume.ABSENT_DEFAULTS['ema_decay'] == 0.0 and resume.ABSENT_DEFAULTS['ema_val_interval'] == 1
    assert 'ema_decay' not in resume.MAY_DIFFER and 'ema_val_interval' in resume.MAY_DIFFER
    new = resume.flag_dict(apply_dataset_preset(parser.parse_args(['--tag', 'x'])))
    assert new['ema_decay'] == 0.0 and new['ema_val_interval'] == 1
    saved = {k: v for k, v in new.items() if k not in ('ema_decay', 'ema_val_interval')}
    resume.check_compatible(saved, new, 1, 1)                       # absent from the file = the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parser.parse_args(['--tag', 'x', '--ema_decay', '0.9'])))
    with pytest.raises(resume.ResumeError, match='--ema_decay'):
        resume.check_compatible(saved, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--ema_decay'):
        resume.check_compatible(dict(saved, ema_decay=0.99), on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--ema_decay'):
        resume.check_compatible(on, new, 1, 1)
    resume.check_compatible(on, dict(on, ema_val_interval=7), 1, 1)  # how often the average is looked at may change


def test_abi_has_the_ema_entry_points():
    """The names are bound (test_abi.py::test_header_and_binding_agree then forces the header to declare them with the same
    arity), the library exports them where it is built, and library and host side moved to a new version together."""
    import ctypes
    from pacingpseudo_amd import _lib
    names = ('pp_adam_step_ema', 'pp_sgd_momentum_step_ema', 'pp_ema_update', 'pp_slab_swap')
    for name in names:
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS and name not in _lib.H16_ENTRIES, name
    # the *_ema forms are the *_dev forms plus ema, ema_decay and the (nullable) coefficient pointer
    for base in ('pp_adam_step', 'pp_sgd_momentum_step'):
        dev, ema = _lib._PROTOS[base + '_dev'][1], _lib._PROTOS[base + '_ema'][1]
        assert list(ema) == list(dev[:-1]) + [_lib.vp, ctypes.c_double, _lib.vp, dev[-1]]
    assert _lib.MIN_LIB_VERSION >= 604
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read(), flags=re.S)
    for name in names:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
    if os.path.exists(_lib.LIB_PATH):
        dll = ctypes.CDLL(_lib.LIB_PATH)
        for name in names:
            assert hasattr(dll, name), name
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(f'`{name}`' in table for name in names)


@pytest.mark.parametrize('decay', [0.9, 0.999])
def test_host_restatement_of_the_warmup_weight(decay):
    """w(t, D) = (float)(1 - min(D, (1 + t) / (10 + t))), formed in double and rounded once: spelled out here with the struct
    module, independently of torch's conversion."""
    import struct
    from pacingpseudo_amd.optim import ema_warmup_weight
    for t in (0, 1, 9, 10 ** 4):
        d = min(decay, (1 + t) / (10 + t))
        want = struct.unpack('f', struct.pack('f', 1.0 - d))[0]
        got = ema_warmup_weight(t, decay)
        assert got == want, (t, decay, got, want)
    assert ema_warmup_weight(0, decay) == struct.unpack('f', struct.pack('f', 0.9))[0]      # the first update takes 90 % of p
    # past the warm-up the weight is the constant 1 - D
    past = next(t for t in range(10 ** 5) if (1 + t) / (10 + t) >= decay)
    assert ema_warmup_weight(past, decay) == ema_warmup_weight(past + 1000, decay)
    assert ema_warmup_weight(max(past - 1, 0), decay) >= ema_warmup_weight(past, decay)
