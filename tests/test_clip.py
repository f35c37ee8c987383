"""--clip_grad_norm / max_grad_norm without a GPU: the parsers, the optimizers' argument checks and state dicts, resume
compatibility with state files older than the flag, and the C ABI of the new entry points."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('driver', ['train', 'upper_bound'])
def test_parsers_accept_the_flag(driver, capsys):
    """H1: default 0 (off), inf parses, a negative value is an argparse error (exit status 2)."""
    import importlib
    parser = importlib.import_module(f'pacingpseudo_amd.{driver}').parser
    assert parser.parse_args(['--tag', 'x']).clip_grad_norm == 0.0
    assert parser.parse_args(['--tag', 'x', '--clip_grad_norm', '2.5']).clip_grad_norm == 2.5
    assert parser.parse_args(['--tag', 'x', '--clip_grad_norm', 'inf']).clip_grad_norm == math.inf
    for bad in ('-1', 'nan'):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['--tag', 'x', '--clip_grad_norm', bad])
        assert e.value.code == 2
        assert '--clip_grad_norm' in capsys.readouterr().err


def _opt(cls, **kw):
    from pacingpseudo_amd import optim
    p = torch.nn.Parameter(torch.zeros(4))
    extra = dict(momentum=0.9) if cls == 'FusedSGD' else {}
    return getattr(optim, cls)([p], lr=1e-3, **extra, **kw)


@pytest.mark.parametrize('cls', ['FusedAdam', 'FusedSGD'])
def test_optimizers_validate_and_carry_max_grad_norm(cls):
    """H2."""
    for bad in (0, 0.0, -1, float('nan')):
        with pytest.raises(ValueError):
            _opt(cls, max_grad_norm=bad)
    assert _opt(cls).param_groups[0]['max_grad_norm'] is None
    assert _opt(cls, max_grad_norm=None).param_groups[0]['max_grad_norm'] is None
    assert _opt(cls, max_grad_norm=math.inf).param_groups[0]['max_grad_norm'] == math.inf
    on = _opt(cls, max_grad_norm=1.5)
    sd = on.state_dict()
    assert sd['param_groups'][0]['max_grad_norm'] == 1.5
    other = _opt(cls)
    other.load_state_dict(sd)
    assert other.param_groups[0]['max_grad_norm'] == 1.5
    # a state dict written before the key existed: off, whatever the optimizer was built with
    old = {'param_groups': [{k: v for k, v in sd['param_groups'][0].items() if k != 'max_grad_norm'}], 'slabs': []}
    on.load_state_dict(old)
    assert on.param_groups[0]['max_grad_norm'] is None
    # off: the read side says so without touching a device
    assert other.last_grad_norm is None and other.last_clip_coef is None and _opt(cls).clip_stats() is None


def test_resume_accepts_state_files_older_than_the_flag():
    """H3."""
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parser
    new = resume.flag_dict(apply_dataset_preset(parser.parse_args(['--tag', 'x'])))
    assert new['clip_grad_norm'] == 0.0
    saved = {k: v for k, v in new.items() if k != 'clip_grad_norm'}
    resume.check_compatible(saved, new, 1, 1)                       # absent from the file = the parser default
    assert 'clip_grad_norm' not in resume.MAY_DIFFER
    on = resume.flag_dict(apply_dataset_preset(parser.parse_args(['--tag', 'x', '--clip_grad_norm', '1'])))
    with pytest.raises(resume.ResumeError, match='--clip_grad_norm'):
        resume.check_compatible(saved, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--clip_grad_norm'):
        resume.check_compatible(dict(saved, clip_grad_norm=2.0), on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--clip_grad_norm'):
        resume.check_compatible(on, new, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


def test_abi_has_the_clip_entry_points():
    """H4: the names are bound (test_abi.py::test_header_and_binding_agree then forces the header to declare them with the same
    arity), and library and host side moved to a new version together."""
    from pacingpseudo_amd import _lib
    for name in ('pp_grad_sumsq_rows', 'pp_grad_sumsq', 'pp_grad_clip_finalize', 'pp_adam_step_clip', 'pp_sgd_momentum_step_clip'):
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
    # the *_clip forms are the *_dev forms plus the coefficient pointer
    for base in ('pp_adam_step', 'pp_sgd_momentum_step'):
        dev, clip = _lib._PROTOS[base + '_dev'][1], _lib._PROTOS[base + '_clip'][1]
        assert list(clip) == list(dev[:-1]) + [_lib.vp, dev[-1]]
    assert _lib.MIN_LIB_VERSION > 602
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION
    # no activation operand: the 16-bit tables share the symbols
    assert 'pp_grad_sumsq' not in _lib.H16_ENTRIES and 'pp_adam_step_clip' not in _lib.H16_ENTRIES


def test_sumsq_rows_depend_on_n_alone():
    """The grid of the sum-of-squares pass (= its partial rows) is a pure function of n: the same n, the same summation tree."""
    from pacingpseudo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    rows = _lib.lib.pp_grad_sumsq_rows
    assert rows(0) == 0 and rows(1) == 1 and rows(4096) == 2
    assert rows(2 ** 20 + 5) == 257                 # ceil((n / 4 + 1) float4 / (256 threads x 4 loads in flight))
    assert max(rows(n) for n in (10 ** 7, 10 ** 9)) == 1024
