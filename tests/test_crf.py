"""--do_loss_crf without a GPU: the parser, the output keys, resume compatibility with state files older than the flags, the C ABI
of the three entry points, and the float64 comparison function of the GPU tests pinned against its own gather form."""
import os
import re

import pytest
import torch

from tests import _crf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_defaults_and_rejections(capsys):
    from pacingpseudo_amd.train import parse_args
    a = parse_args(['--tag', 'x'])
    assert a.do_loss_crf is False and a.loss_crf_weight == 0.1 and a.ramp_up_loss_crf is False
    assert (a.crf_radius, a.crf_dilation, a.crf_sigma_xy, a.crf_sigma_rgb) == (5, 1, 6.0, 0.1)
    on = parse_args(['--tag', 'x', '--do_loss_crf', '--crf_radius', '4', '--crf_dilation', '4', '--crf_sigma_xy', '3', '--crf_sigma_rgb',
                     '0.2', '--loss_crf_weight', '0.5', '--ramp_up_loss_crf'])
    assert on.do_loss_crf and on.ramp_up_loss_crf and (on.crf_radius, on.crf_dilation, on.crf_sigma_xy, on.crf_sigma_rgb) == (4, 4, 3.0, 0.2)
    for bad in (['--crf_radius', '0'], ['--crf_radius', '9'], ['--crf_dilation', '0'], ['--crf_dilation', '5'],
                ['--crf_radius', '5', '--crf_dilation', '4'],                       # r * d = 20 > 16
                ['--crf_sigma_xy', '0'], ['--crf_sigma_xy', '-1'], ['--crf_sigma_rgb', '0'], ['--crf_sigma_rgb', 'nan'],
                ['--crf_sigma_rgb', 'inf']):
        with pytest.raises(SystemExit) as e:
            parse_args(['--tag', 'x'] + bad)
        assert e.value.code == 2, bad
        assert '--crf_' in capsys.readouterr().err, bad


def test_upper_bound_driver_has_no_crf_flag():
    from pacingpseudo_amd.upper_bound import parser
    assert not any(o.startswith('--crf') or o == '--do_loss_crf' for a in parser._actions for o in a.option_strings)


def test_parameter_check_of_the_functional_form():
    from pacingpseudo_amd.losses.losses import check_crf_params
    assert check_crf_params() == dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    assert check_crf_params(8, 2, 1, 1, K=32, C=4)['radius'] == 8
    for kw in (dict(radius=0), dict(dilation=0), dict(sigma_xy=0.0), dict(sigma_rgb=-1.0), dict(sigma_rgb=float('nan')), dict(radius=2.5)):
        with pytest.raises(ValueError):
            check_crf_params(**kw)
    for kw in (dict(radius=9), dict(dilation=5), dict(radius=6, dilation=3), dict(K=33), dict(K=0), dict(C=5)):
        with pytest.raises(NotImplementedError):
            check_crf_params(**kw)


def test_expected_keys_with_and_without_the_flag():
    from pacingpseudo_amd.data import full_flags
    from pacingpseudo_amd.models.consistency_reglur_memory import _LOSS_KEYS, ConsistencyRegulr
    assert _LOSS_KEYS.index('loss_crf') == _LOSS_KEYS.index('loss_cr') + 1

    class M:
        _expected_keys = ConsistencyRegulr._expected_keys
    m = M()
    m.args = full_flags()                                          # a namespace without the attribute: the flag is off
    off = m._expected_keys('train')
    assert 'loss_crf' not in off
    m.args = full_flags(do_loss_crf=True)
    on = m._expected_keys('train')
    assert on == off[:off.index('segmentation/logits_strong') + 1] + ['loss_crf'] + off[off.index('segmentation/logits_strong') + 1:]
    assert 'loss_crf' not in m._expected_keys('val')
    m.args = full_flags(do_loss_crf=True, do_decoder_consistency=False, do_loss_ent=False, do_aux_path=False, do_memory=False)
    assert m._expected_keys('train') == ['segmentation/logits', 'loss_pce', 'loss_crf']


def test_resume_accepts_state_files_older_than_the_flags():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    names = ('do_loss_crf', 'loss_crf_weight', 'ramp_up_loss_crf', 'crf_radius', 'crf_dilation', 'crf_sigma_xy', 'crf_sigma_rgb')
    new = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x'])))
    for n in names:
        assert n not in resume.MAY_DIFFER and resume.ABSENT_DEFAULTS[n] == new[n], n
    saved = {k: v for k, v in new.items() if k not in names}
    resume.check_compatible(saved, new, 1, 1)                       # absent from the file = the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_crf'])))
    with pytest.raises(resume.ResumeError, match='--do_loss_crf'):
        resume.check_compatible(saved, on, 1, 1)
    other = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_crf', '--crf_radius', '3'])))
    with pytest.raises(resume.ResumeError, match='--crf_radius'):
        resume.check_compatible(on, other, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


def test_abi_has_the_crf_entry_points():
    """Header, binding and export name the three entry points with the same arity (test_abi.py compares all of them; this
    states the three by name), and library and host side moved to a new version together."""
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    for name in ('pp_crf_loss_workspace', 'pp_crf_loss_fwd', 'pp_crf_loss_bwd'):
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\b' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        assert len(m.group(1).split(',')) == len(_lib._PROTOS[name][1]), name
        assert name not in _lib.H16_ENTRIES                     # fp32 logits and image in every storage mode: one symbol
    assert _lib._PROTOS['pp_crf_loss_workspace'][0] is _lib.sz
    assert _lib.MIN_LIB_VERSION > 604
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert 'pp_crf_loss' not in open(os.path.join(ROOT, 'include', h)).read()


CASES = [   # (N, K, C, H, W, radius, dilation, masked, logit scale)
    (2, 2, 1, 12, 10, 1, 1, False, 1.0),
    (1, 5, 3, 14, 17, 3, 2, True, 1.0),
    (2, 17, 1, 9, 11, 2, 3, True, 1.0),
    (1, 32, 3, 8, 8, 5, 1, False, 1.0),
    (1, 5, 1, 16, 13, 5, 1, True, 120.0),       # probabilities exactly 0 or 1
    (1, 1, 1, 6, 7, 2, 1, False, 1.0),          # one class: the loss is identically 0
]


@pytest.mark.parametrize('case', CASES, ids=[f'K{c[1]}-C{c[2]}-{c[3]}x{c[4]}-r{c[5]}d{c[6]}{"-mask" if c[7] else ""}{"-sharp" if c[8] != 1 else ""}' for c in CASES])
def test_direct_form_agrees_with_its_gather_form(case):
    """The helper is pinned: autograd of the direct double sum and the closed gather form agree to 1e-12 (float64)."""
    N, K, C, H, W, r, d, masked, scale = case
    g = torch.Generator().manual_seed(100 + K + r)
    z = torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    x = R.smooth_image(N, C, H, W, seed=K)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    kw = dict(radius=r, dilation=d, sigma_xy=1.5 + r, sigma_rgb=0.1)
    loss, grad = R.crf_loss_and_grad(z, x, m, **kw)
    loss_g, grad_g, S = R.crf_gather_form(z, x, m, **kw)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert abs(float(loss - loss_g)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((grad - grad_g).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))
    if K == 1:
        assert abs(float(loss)) < 1e-15 and float(grad.abs().max()) < 1e-15
    else:
        assert float(loss) > 0 and float(S.max()) > 0                      # not a vacuous case
    if masked:
        assert float(grad[(m == 0).expand_as(grad)].abs().max()) == 0.0      # no gradient at a masked pixel
