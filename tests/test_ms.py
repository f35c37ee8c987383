"""--do_loss_ms without a GPU: the parser, the output keys, resume compatibility with state files older than the flags, the argument
checks, the C ABI of the three entry points, and the float64 comparison functions of the GPU tests pinned against each other
(autograd of the direct definition against the analytic form the kernels evaluate)."""
import os
import re

import pytest
import torch

from tests import _ms_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('do_loss_ms', 'loss_ms_weight', 'ramp_up_loss_ms', 'ms_tv_weight')
ENTRIES = ('pp_ms_loss_workspace', 'pp_ms_loss_fwd', 'pp_ms_loss_bwd')


def _accepted(tv_weight=1.0, K=None, C=None):
    """Every case of this file lies inside what the loss accepts: the project's own check says so (and its limits are the issue's)."""
    from pacingpseudo_amd.losses import losses
    assert (losses.MS_MAX_CLASSES, losses.MS_MAX_CHANNELS) == (32, 4)
    return losses.check_ms_params(tv_weight, K=K, C=C)


def test_parser_defaults_and_rejections(capsys):
    from pacingpseudo_amd.train import parse_args, parser
    a = parse_args(['--tag', 'x'])
    assert a.do_loss_ms is False and a.loss_ms_weight == 0.1 and a.ramp_up_loss_ms is False and a.ms_tv_weight == 1.0
    on = parse_args(['--tag', 'x', '--do_loss_ms', '--loss_ms_weight', '0.5', '--ramp_up_loss_ms', '--ms_tv_weight', '0'])
    assert on.do_loss_ms and on.ramp_up_loss_ms and on.loss_ms_weight == 0.5 and on.ms_tv_weight == 0.0
    assert on.do_loss_crf is False and on.do_loss_nc is False                      # the other regularisers are their own
    every = parse_args(['--tag', 'x', '--do_loss_ms', '--do_loss_nc', '--do_loss_crf'])
    assert every.do_loss_ms and every.do_loss_nc and every.do_loss_crf
    for bad in (['--ms_tv_weight', '-0.5'], ['--ms_tv_weight', 'nan'], ['--ms_tv_weight', 'inf'], ['--ms_tv_weight', 'much']):
        with pytest.raises(SystemExit) as e:
            parse_args(['--tag', 'x'] + bad)
        assert e.value.code == 2, bad
        assert '--ms_tv_weight' in capsys.readouterr().err, bad
    helps = {o: a.help for a in parser._actions for o in a.option_strings}
    assert 'untuned' in helps['--loss_ms_weight'] and 'untuned' in helps['--ms_tv_weight']
    # the fully-supervised driver has no such flag
    from pacingpseudo_amd.upper_bound import parser as ub
    assert not any(o.startswith('--ms_') or '_ms' in o for a in ub._actions for o in a.option_strings)


def test_parameter_check_refuses_before_any_launch():
    """check_ms_params and the functional form refuse on a machine without a GPU: nothing is launched for a bad argument."""
    from pacingpseudo_amd.losses.losses import MS_MAX_CHANNELS, MS_MAX_CLASSES, check_ms_params
    assert check_ms_params() == dict(tv_weight=1.0)
    assert (MS_MAX_CLASSES, MS_MAX_CHANNELS) == (32, 4)
    assert check_ms_params(0, K=MS_MAX_CLASSES, C=MS_MAX_CHANNELS) == dict(tv_weight=0.0) and check_ms_params(2.5, K=1, C=1) == dict(tv_weight=2.5)
    for kw in (dict(tv_weight=-1e-9), dict(tv_weight=float('nan')), dict(tv_weight=float('inf')), dict(tv_weight='x'), dict(tv_weight=None)):
        with pytest.raises(ValueError, match='Mumford-Shah'):
            check_ms_params(**kw)
    for kw in (dict(K=33), dict(K=0), dict(C=5), dict(C=0)):
        with pytest.raises(NotImplementedError, match='Mumford-Shah'):
            check_ms_params(**kw)
    import pacingpseudo_amd.losses as L
    from pacingpseudo_amd.losses.losses import mumford_shah_loss
    assert L.mumford_shah_loss is mumford_shah_loss
    with pytest.raises(TypeError):                                  # host tensors: refused before the library is touched
        mumford_shah_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))


def test_expected_keys_with_and_without_the_flags():
    from pacingpseudo_amd.data import full_flags
    from pacingpseudo_amd.models.consistency_reglur_memory import _LOSS_KEYS, ConsistencyRegulr
    assert _LOSS_KEYS.index('loss_ms') == _LOSS_KEYS.index('loss_nc') + 1 == _LOSS_KEYS.index('loss_crf') + 2

    class M:
        _expected_keys = ConsistencyRegulr._expected_keys
    m = M()
    m.args = full_flags()                                          # a namespace without the attributes: every flag off
    off = m._expected_keys('train')
    cut = off.index('segmentation/logits_strong') + 1
    assert not {'loss_ms', 'loss_nc', 'loss_crf'} & set(off)
    m.args = full_flags(do_loss_ms=True)
    assert m._expected_keys('train') == off[:cut] + ['loss_ms'] + off[cut:]
    assert 'loss_ms' not in m._expected_keys('val')
    m.args = full_flags(do_loss_nc=True)                           # NC alone: what it was
    assert m._expected_keys('train') == off[:cut] + ['loss_nc'] + off[cut:]
    m.args = full_flags(do_loss_crf=True, do_loss_ms=True)
    assert m._expected_keys('train') == off[:cut] + ['loss_crf', 'loss_ms'] + off[cut:]
    m.args = full_flags(do_loss_crf=True, do_loss_nc=True, do_loss_ms=True)
    assert m._expected_keys('train') == off[:cut] + ['loss_crf', 'loss_nc', 'loss_ms'] + off[cut:]
    assert 'loss_ms' not in m._expected_keys('val')
    m.args = full_flags(do_loss_ms=True, do_decoder_consistency=False, do_loss_ent=False, do_aux_path=False, do_memory=False)
    assert m._expected_keys('train') == ['segmentation/logits', 'loss_pce', 'loss_ms']


def test_resume_accepts_state_files_older_than_the_flags():
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.train import apply_dataset_preset, parse_args
    new = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x'])))
    for n in NAMES:
        assert n not in resume.MAY_DIFFER and resume.ABSENT_DEFAULTS[n] == new[n], n
    saved = {k: v for k, v in new.items() if k not in NAMES}
    resume.check_compatible(saved, new, 1, 1)                       # absent from the file = the parser defaults
    on = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_ms'])))
    with pytest.raises(resume.ResumeError, match='--do_loss_ms'):
        resume.check_compatible(saved, on, 1, 1)
    other = resume.flag_dict(apply_dataset_preset(parse_args(['--tag', 'x', '--do_loss_ms', '--ms_tv_weight', '0.5'])))
    with pytest.raises(resume.ResumeError, match='--ms_tv_weight'):
        resume.check_compatible(on, other, 1, 1)
    resume.check_compatible(on, dict(on), 1, 1)


def test_abi_has_the_ms_entry_points():
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
    assert _lib._PROTOS['pp_ms_loss_workspace'][0] is _lib.sz and len(_lib._PROTOS['pp_ms_loss_workspace'][1]) == 5
    assert len(_lib._PROTOS['pp_ms_loss_fwd'][1]) == 15 and len(_lib._PROTOS['pp_ms_loss_bwd'][1]) == 8
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert 'pp_ms_loss' not in open(os.path.join(ROOT, 'include', h)).read()


def _inputs(N, K, C, H, W, masked, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    x = R.offset_image(N, C, H, W, seed=seed)
    m = (torch.rand(N, 1, H, W, generator=g) < 0.7).float() if masked else None
    return z, x, m


SHAPES = [(2, 1, 1, 6, 7), (2, 2, 1, 7, 9), (1, 5, 3, 9, 8), (2, 17, 2, 5, 6), (1, 32, 4, 4, 5), (2, 4, 1, 1, 13), (2, 9, 2, 11, 1)]


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', SHAPES, ids=['-'.join(map(str, s)) for s in SHAPES])
def test_analytic_form_agrees_with_autograd_of_the_definition(shape, masked):
    """The derivative through mu vanishes: the analytic gradient equals float64 autograd of the direct definition (mu not detached)
    to 1e-12, K = 1 .. 32, with and without a mask, single rows and single columns included."""
    N, K, C, H, W = shape
    z, x, m = _inputs(N, K, C, H, W, masked, seed=K + H)
    for lam in (0.0, 1.0, 0.3):
        _accepted(lam, K=K, C=C)
        loss, grad = R.ms_loss_and_grad(z, x, m, tv_weight=lam)
        loss_a, grad_a, u, D = R.ms_analytic_form(z, x, m, tv_weight=lam)
        assert torch.isfinite(loss) and torch.isfinite(grad).all()
        assert abs(float(loss - loss_a)) <= 1e-12 * max(1.0, abs(float(loss)))
        assert float((grad - grad_a).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))
        assert float((u / D - grad_a).abs().max()) == 0.0
        assert float(grad.sum(1).abs().max()) <= 1e-12                      # a soft-max gradient: zero sum over the classes
        if K == 1:
            assert float(grad.abs().max()) <= 1e-15                         # one class: p = 1, nothing to move
        else:
            assert float(loss) > 0 and float(grad.abs().max()) > 0          # not a vacuous case
        if masked:
            assert float(grad[(m == 0).expand_as(grad)].abs().max()) == 0.0  # no gradient at a masked pixel
    assert int(R.ambiguous_pixels(z, m).sum()) == 0


def test_means_are_per_image():
    """Images with different intensity offsets: every image's mu carries its own offset, and mixing the images is another loss."""
    _accepted(K=4, C=1)
    z, x, m = _inputs(3, 4, 1, 8, 9, False, seed=5)
    S, mu, active = R.ms_stats(z, x, m)
    assert bool(active.all()) and float((mu[1] - mu[0]).min()) > 0.4 and float((mu[2] - mu[1]).min()) > 0.4
    each = sum(float(R.ms_energy_direct(z[i:i + 1], x[i:i + 1], None, 0.0)[0]) for i in range(3))
    assert abs(each - float(R.ms_energy_direct(z, x, None, 0.0)[0])) <= 1e-12 * each


def test_half_batches_add_up_with_the_global_denominator():
    """What a data-parallel rank contributes: its energy over the GLOBAL D; the shares add up to the whole batch's loss."""
    _accepted(K=5, C=1)
    z, x, m = _inputs(4, 5, 1, 10, 12, True, seed=7)
    whole = float(R.ms_loss_direct(z, x, m))
    D = float(m.sum())
    shares = [float(R.ms_loss_direct(z[i:i + 2], x[i:i + 2], m[i:i + 2], denominator=D)) for i in (0, 2)]
    assert whole > 0 and abs(sum(shares) - whole) <= 1e-12 * whole


def test_piecewise_constant_image_with_matching_regions_costs_only_the_boundary():
    """The property the loss is there for: a confident partition along the image's edge has next to no level-set energy, the same
    partition moved into a homogeneous region a large one; the TV term counts the boundary length either way."""
    def two_regions(col):
        z = torch.zeros(1, 2, 16, 16, dtype=torch.float64)
        z[:, 0, :, :col] = 40.0
        z[:, 1, :, col:] = 40.0
        x = torch.zeros(1, 1, 16, 16)
        x[..., 8:] = 1.0
        return z, x
    _accepted(0.0, K=2, C=1)
    on_edge = float(R.ms_energy_direct(*two_regions(8), None, 0.0)[0])
    off_edge = float(R.ms_energy_direct(*two_regions(4), None, 0.0)[0])
    assert on_edge < 1e-12 and off_edge > 10.0
    for col in (8, 4):
        z, x = two_regions(col)
        tv = float(R.ms_energy_direct(z, x, None, 1.0)[0] - R.ms_energy_direct(z, x, None, 0.0)[0])
        assert abs(tv - 2 * 16) <= 1e-9                             # 16 horizontal pairs across the boundary, two classes


def test_inactive_class_and_empty_mask():
    """A class of no mass in an image: no level-set term and no level-set gradient from it; an all-zero mask: loss 0, gradient 0."""
    _accepted(K=5, C=1)
    z, x, _ = _inputs(2, 5, 1, 8, 9, False, seed=3)
    z[0, 3] = -1e4
    S, mu, active = R.ms_stats(z, x, None)
    assert not bool(active[0, 3]) and bool(active[1].all()) and float(mu[0, 3].abs().max()) == 0.0
    loss, grad = R.ms_loss_and_grad(z, x, None)
    loss_a, grad_a, _, _ = R.ms_analytic_form(z, x, None)
    assert abs(float(loss - loss_a)) <= 1e-12 and float((grad - grad_a).abs().max()) <= 1e-12
    assert float(grad[0, 3].abs().max()) == 0.0
    zero = R.ms_loss_and_grad(z, x, torch.zeros(2, 1, 8, 9))
    assert float(zero[0]) == 0.0 and float(zero[1].abs().max()) == 0.0


def test_ambiguous_pixels_lists_both_ends_of_a_close_pair():
    _accepted(K=2, C=1)
    z = torch.zeros(1, 2, 3, 4, dtype=torch.float64)
    assert int(R.ambiguous_pixels(z).sum()) == 0                    # exactly equal: sign is 0 on both sides, not ambiguous
    z[0, 0, 1, 2] = 1e-7
    amb = R.ambiguous_pixels(z)
    want = torch.zeros(3, 4, dtype=torch.bool)
    want[1, 1:4] = True
    want[0, 2] = want[2, 2] = True
    assert bool((amb[0] == want).all())
    m = torch.ones(1, 1, 3, 4)
    m[0, 0, 1, 2] = 0
    assert int(R.ambiguous_pixels(z, m).sum()) == 0                 # pairs the mask removes do not count
