"""--do_loss_nc without a GPU: the parser, the output keys, resume compatibility with state files older than the flags, the C ABI of
the three entry points, and the float64 comparison function of the GPU tests pinned against its own gather form and against the
properties a normalised cut has."""
import os
import re

import pytest
import torch

from tests import _nc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('do_loss_nc', 'loss_nc_weight', 'ramp_up_loss_nc', 'nc_radius', 'nc_dilation', 'nc_sigma_xy', 'nc_sigma_rgb')
ENTRIES = ('pp_nc_loss_workspace', 'pp_nc_loss_fwd', 'pp_nc_loss_bwd')


def test_parser_defaults_and_rejections(capsys):
    from pacingpseudo_amd.train import parse_args
    a = parse_args(['--tag', 'x'])
    assert a.do_loss_nc is False and a.loss_nc_weight == 0.1 and a.ramp_up_loss_nc is False
    assert (a.nc_radius, a.nc_dilation, a.nc_sigma_xy, a.nc_sigma_rgb) == (5, 1, 6.0, 0.1)
    on = parse_args(['--tag', 'x', '--do_loss_nc', '--nc_radius', '4', '--nc_dilation', '4', '--nc_sigma_xy', '3', '--nc_sigma_rgb',
                     '0.2', '--loss_nc_weight', '0.5', '--ramp_up_loss_nc'])
    assert on.do_loss_nc and on.ramp_up_loss_nc and (on.nc_radius, on.nc_dilation, on.nc_sigma_xy, on.nc_sigma_rgb) == (4, 4, 3.0, 0.2)
    assert on.loss_nc_weight == 0.5 and on.do_loss_crf is False and on.crf_radius == 5          # the CRF flags are their own
    both = parse_args(['--tag', 'x', '--do_loss_nc', '--do_loss_crf'])
    assert both.do_loss_nc and both.do_loss_crf
    for bad in (['--nc_radius', '0'], ['--nc_radius', '9'], ['--nc_dilation', '0'], ['--nc_dilation', '5'],
                ['--nc_radius', '5', '--nc_dilation', '4'],                       # r * d = 20 > 16
                ['--nc_sigma_xy', '0'], ['--nc_sigma_xy', '-1'], ['--nc_sigma_rgb', '0'], ['--nc_sigma_rgb', 'nan'],
                ['--nc_sigma_rgb', 'inf']):
        with pytest.raises(SystemExit) as e:
            parse_args(['--tag', 'x'] + bad)
        assert e.value.code == 2, bad
        assert '--nc_' in capsys.readouterr().err, bad


def test_upper_bound_driver_has_no_nc_flag():
    from pacingpseudo_amd.upper_bound import parser
    assert not any(o.startswith('--nc_') or '_nc' in o for a in parser._actions for o in a.option_strings)


def test_parameter_check_of_the_functional_form():
    from pacingpseudo_amd.losses.losses import check_nc_params
    assert check_nc_params() == dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    assert check_nc_params(8, 2, 1, 1, K=32, C=4)['radius'] == 8
    for kw in (dict(radius=0), dict(dilation=0), dict(sigma_xy=0.0), dict(sigma_rgb=-1.0), dict(sigma_rgb=float('nan')), dict(radius=2.5)):
        with pytest.raises(ValueError, match='normalised cut'):
            check_nc_params(**kw)
    for kw in (dict(radius=9), dict(dilation=5), dict(radius=6, dilation=3), dict(K=33), dict(K=0), dict(C=5)):
        with pytest.raises(NotImplementedError, match='normalised cut'):
            check_nc_params(**kw)
    import pacingpseudo_amd.losses as L
    from pacingpseudo_amd.losses.losses import normalized_cut_loss
    assert L.normalized_cut_loss is normalized_cut_loss


def test_expected_keys_with_and_without_the_flags():
    from pacingpseudo_amd.data import full_flags
    from pacingpseudo_amd.models.consistency_reglur_memory import _LOSS_KEYS, ConsistencyRegulr
    assert _LOSS_KEYS.index('loss_nc') == _LOSS_KEYS.index('loss_crf') + 1

    class M:
        _expected_keys = ConsistencyRegulr._expected_keys
    m = M()
    m.args = full_flags()                                          # a namespace without the attributes: both flags off
    off = m._expected_keys('train')
    cut = off.index('segmentation/logits_strong') + 1
    assert 'loss_nc' not in off and 'loss_crf' not in off
    m.args = full_flags(do_loss_nc=True)
    assert m._expected_keys('train') == off[:cut] + ['loss_nc'] + off[cut:]
    assert 'loss_nc' not in m._expected_keys('val')
    m.args = full_flags(do_loss_crf=True)                          # CRF alone: what it was
    assert m._expected_keys('train') == off[:cut] + ['loss_crf'] + off[cut:]
    m.args = full_flags(do_loss_crf=True, do_loss_nc=True)
    assert m._expected_keys('train') == off[:cut] + ['loss_crf', 'loss_nc'] + off[cut:]
    assert 'loss_nc' not in m._expected_keys('val')
    m.args = full_flags(do_loss_nc=True, do_decoder_consistency=False, do_loss_ent=False, do_aux_path=False, do_memory=False)
    assert m._expected_keys('train') == ['segmentation/logits', 'loss_pce', 'loss_nc']


def test_resume_accepts_state_files_older_than_the_flags():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    new = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x'])))
    for n in NAMES:
        assert n not in resume.MAY_DIFFER and resume.ABSENT_DEFAULTS[n] == new[n], n
    saved = {k: v for k, v in new.items() if k not in NAMES}
    resume.check_compatible(saved, new, 1, 1)                       # absent from the file = the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_nc'])))
    with pytest.raises(resume.ResumeError, match='--do_loss_nc'):
        resume.check_compatible(saved, on, 1, 1)
    other = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_nc', '--nc_radius', '3'])))
    with pytest.raises(resume.ResumeError, match='--nc_radius'):
        resume.check_compatible(on, other, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


def test_abi_has_the_nc_entry_points():
    """Header, binding and export name the three entry points with the same arity; fp32 only: one symbol in every storage mode."""
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    for name in ENTRIES:
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\b' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        assert len(m.group(1).split(',')) == len(_lib._PROTOS[name][1]), name
        assert name not in _lib.H16_ENTRIES
        assert name + '_h16' not in _lib._PROTOS and name + '_bf16' not in _lib._PROTOS
    assert _lib._PROTOS['pp_nc_loss_workspace'][0] is _lib.sz and len(_lib._PROTOS['pp_nc_loss_workspace'][1]) == 4
    assert len(_lib._PROTOS['pp_nc_loss_fwd'][1]) == 18 and len(_lib._PROTOS['pp_nc_loss_bwd'][1]) == 7
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert 'pp_nc_loss' not in open(os.path.join(ROOT, 'include', h)).read()


CASES = [   # (N, K, C, H, W, radius, dilation, masked, logit scale)
    (2, 2, 1, 12, 10, 1, 1, False, 1.0),
    (1, 5, 3, 14, 17, 3, 2, True, 1.0),
    (2, 17, 1, 9, 11, 2, 3, True, 1.0),
    (1, 32, 3, 8, 8, 5, 1, False, 1.0),
    (1, 5, 1, 16, 13, 5, 1, True, 120.0),       # probabilities exactly 0 or 1
    (1, 1, 1, 6, 7, 2, 1, False, 1.0),          # one class: A = V, the loss is 0
]


def _case_inputs(case):
    N, K, C, H, W, r, d, masked, scale = case
    g = torch.Generator().manual_seed(100 + K + r)
    z = torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    x = R.smooth_image(N, C, H, W, seed=K)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    return z, x, m, dict(radius=r, dilation=d, sigma_xy=1.5 + r, sigma_rgb=0.1)


@pytest.mark.parametrize('case', CASES, ids=[f'K{c[1]}-C{c[2]}-{c[3]}x{c[4]}-r{c[5]}d{c[6]}{"-mask" if c[7] else ""}{"-sharp" if c[8] != 1 else ""}' for c in CASES])
def test_direct_form_agrees_with_its_gather_form(case):
    """The helper is pinned: autograd of the direct double sum and the closed gather form agree to 1e-12 (float64)."""
    K, masked = case[1], case[7]
    z, x, m, kw = _case_inputs(case)
    loss, grad = R.nc_loss_and_grad(z, x, m, **kw)
    loss_g, grad_g, A, V = R.nc_gather_form(z, x, m, **kw)
    Ad, Vd = R.nc_assoc_vol(z, x, m, **kw)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert abs(float(loss - loss_g)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((grad - grad_g).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))
    assert float(((A - Ad).abs() / Vd.clamp_min(1e-30)).max()) <= 1e-12 and float(((V - Vd).abs() / Vd.clamp_min(1e-30)).max()) <= 1e-12
    nc = R.nc_terms(Ad, Vd)
    assert float(nc.min()) >= 0.0 and float(nc.max()) < 1.0                  # 0 <= NC_nc < 1 (A <= V, A > 0)
    assert bool((Ad <= Vd * (1 + 1e-12)).all())
    if K == 1:
        assert abs(float(loss)) < 1e-15 and float(grad.abs().max()) < 1e-15
    else:
        assert float(loss) > 0 and float(V.min()) > 1e-3 and float(grad.abs().max()) > 0      # not a vacuous case
    if masked:
        assert float(grad[(m == 0).expand_as(grad)].abs().max()) == 0.0      # no gradient at a masked pixel


def test_half_batches_average_to_the_whole_batch():
    """L is a mean over (image, class): two half-batches averaged are the whole batch; with the global count as `denominator` they
    add up to it (what a data-parallel rank contributes)."""
    g = torch.Generator().manual_seed(7)
    z = torch.randn(4, 5, 14, 12, generator=g, dtype=torch.float64)
    x = R.smooth_image(4, 1, 14, 12, seed=8)
    m = (torch.rand(4, 1, 14, 12, generator=g) < 0.7).float()
    kw = dict(radius=2, dilation=1, sigma_xy=3.0, sigma_rgb=0.1)
    whole = float(R.nc_loss_direct(z, x, m, **kw))
    halves = [float(R.nc_loss_direct(z[i:i + 2], x[i:i + 2], m[i:i + 2], **kw)) for i in (0, 2)]
    shares = [float(R.nc_loss_direct(z[i:i + 2], x[i:i + 2], m[i:i + 2], denominator=20.0, **kw)) for i in (0, 2)]
    print(f'whole batch {whole!r}, mean of the halves {sum(halves) / 2!r}')
    assert 0.3 < whole < 1.0
    assert abs(sum(halves) / 2 - whole) <= 1e-12 and abs(sum(shares) - whole) <= 1e-12


def _two_regions(col):
    """32 x 32, an intensity edge at column 16; a confident two-class prediction whose boundary lies at column `col`."""
    z = torch.zeros(1, 2, 32, 32)
    z[:, 0, :, :col] = 8.0
    z[:, 1, :, col:] = 8.0
    x = torch.zeros(1, 1, 32, 32)
    x[..., 16:] = 1.0
    return z, x


def test_a_cut_along_the_image_edge_is_cheap():
    """The property the loss is there for: a partition along the image's edge scores next to nothing, the same partition moved into
    a homogeneous region at least ten times as much."""
    kw = dict(radius=3, dilation=1, sigma_xy=4.0, sigma_rgb=0.1)
    on_edge = float(R.nc_loss_direct(*_two_regions(16), None, **kw))
    off_edge = [float(R.nc_loss_direct(*_two_regions(c), None, **kw)) for c in (10, 22)]
    print(f'boundary on the edge {on_edge:.3e}, at columns 10 / 22 {off_edge[0]:.3e} / {off_edge[1]:.3e}')
    assert 0.0 <= on_edge < 0.01
    assert min(off_edge) >= 10.0 * on_edge and min(off_edge) > 0.01


def test_inactive_class_adds_nothing():
    """A class whose volume is 0 in an image: NC = 0 there, no gradient to its logits, the other classes unaffected by the guard."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 5, 12, 11, generator=g, dtype=torch.float64)
    z[:, 3] = -1e4
    x = R.smooth_image(2, 1, 12, 11, seed=4)
    kw = dict(radius=2, dilation=1, sigma_xy=3.0, sigma_rgb=0.1)
    loss, grad = R.nc_loss_and_grad(z, x, None, **kw)
    loss_g, grad_g, A, V = R.nc_gather_form(z, x, None, **kw)
    assert float(V[:, 3].abs().max()) == 0.0 and float(grad[:, 3].abs().max()) == 0.0 and float(grad_g[:, 3].abs().max()) == 0.0
    assert abs(float(loss - loss_g)) <= 1e-12 and float((grad - grad_g).abs().max()) <= 1e-12
    assert 0.3 < float(loss) < 0.8                                  # four active classes of five: about (4/5) (1 - 1/4)
    zero = R.nc_loss_and_grad(z, x, torch.zeros(2, 1, 12, 11), **kw)
    assert float(zero[0]) == 0.0 and float(zero[1].abs().max()) == 0.0
