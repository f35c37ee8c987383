"""The consistency variants bikl_loss, js_loss and hard_ce_loss (cr_variant 5 - 7 of pp_seg_losses_fwd / _bwd) without a GPU: the
command line, the two variant tables, the exports, the header comment, the library version, and the float64 reference of
tests/_cr_reference.py -- pinned to the reference's own bidirectional_kl_loss by tests/golden/cr_bikl.npz, and checked against
finite differences (js_loss and hard_ce_loss have no counterpart in the reference: unpinned)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _cr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'bikl_loss': 5, 'js_loss': 6, 'hard_ce_loss': 7}


def test_parser_accepts_the_new_names_and_rejects_an_unknown_one(capsys):
    from pacingpseudo_amd.train import parse_args, parser
    assert parser.get_default('loss_cr_variants') == 'ce_loss'
    for name in ('ce_loss', 'l1_loss', 'l2_loss', 'kl_loss') + tuple(NEW):
        assert parse_args(['--tag', 't', '--loss_cr_variants', name]).loss_cr_variants == name
    with pytest.raises(SystemExit) as e:
        parse_args(['--tag', 't', '--loss_cr_variants', 'tv_loss'])
    assert e.value.code == 2
    assert 'invalid choice' in capsys.readouterr().err


def test_variant_tables_agree():
    from pacingpseudo_amd import engine
    from pacingpseudo_amd.losses import losses
    assert engine.CR_VARIANTS == losses._VARIANT
    assert engine.CR_VARIANTS == {'ce_loss': 1, 'l1_loss': 2, 'l2_loss': 3, 'kl_loss': 4, **NEW}
    assert R.CODE == NEW and set(R.BY_NAME) == set(NEW)
    from pacingpseudo_amd.train import parser
    choices = next(a.choices for a in parser._actions if a.dest == 'loss_cr_variants')
    assert sorted(choices) == sorted(engine.CR_VARIANTS)


def test_functions_are_exported():
    import inspect
    import pacingpseudo_amd.losses as L
    for name in ('bidirectional_kl_loss', 'js_loss', 'hard_label_cross_entropy_loss'):
        f = getattr(L, name)
        assert list(inspect.signature(f).parameters) == ['input', 'target', 'valid_mask']
        assert inspect.signature(f).parameters['valid_mask'].default is None
        with pytest.raises(TypeError, match='4-D float32 CUDA tensor'):
            f(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 2))          # _check: CPU tensors are refused before any launch


def test_header_and_kernel_name_the_three_codes():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    comment = re.search(r'/\*((?:(?!\*/).)*cr_variant:(?:(?!\*/).)*)\*/\s*size_t pp_seg_losses_workspace', header, flags=re.S).group(1)
    for name, code in NEW.items():
        assert re.search(r'\b%d %s\b' % (code, name), comment), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_loss.hip')).read()
    assert src.count('cr_variant >= 0 && cr_variant <= 7') == 2
    # no new launch entry point: the two entries keep their 14 and 19 parameters
    from pacingpseudo_amd import _lib
    assert len(_lib._PROTOS['pp_seg_losses_fwd'][1]) == 14 and len(_lib._PROTOS['pp_seg_losses_bwd'][1]) == 19
    assert len(_lib._PROTOS['pp_seg_losses_workspace'][1]) == 2


def test_library_version_is_unchanged():
    from pacingpseudo_amd import _lib
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION == 606


# ---------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize('spread', [1, 60])
@pytest.mark.parametrize('masked', [False, True])
def test_reference_reproduces_the_captured_bidirectional_kl(spread, masked):
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'cr_bikl.npz'))
    assert d['input'].shape == (2, 5, 6, 7) and d['input'].dtype == np.float64 and list(d['spreads']) == [1, 60]
    zs = (torch.from_numpy(d['input']) * spread).requires_grad_(True)
    zw = (torch.from_numpy(d['target']) * spread).requires_grad_(True)
    m = torch.from_numpy(d['valid_mask']) if masked else None
    loss = R.bidirectional_kl_loss(zs, zw, m)
    loss.backward()
    loss = loss.detach()
    tag = f's{spread}_{"masked" if masked else "unmasked"}'
    assert abs(float(loss) - float(d[f'{tag}/loss'])) <= 1e-12 * abs(float(d[f'{tag}/loss']))
    for got, key in ((zs.grad, 'grad_input'), (zw.grad, 'grad_target')):
        ref = torch.from_numpy(d[f'{tag}/{key}'])
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), key


def _fd_inputs(K, spread, seed):
    g = torch.Generator().manual_seed(seed)
    zs = (torch.randn(2, K, 3, 2, generator=g, dtype=torch.float64) * spread).requires_grad_(True)
    zw = (torch.randn(2, K, 3, 2, generator=g, dtype=torch.float64) * spread).requires_grad_(True)
    mask = (torch.rand(2, 1, 3, 2, generator=g) > 0.3).double()
    return zs, zw, mask


@pytest.mark.parametrize('name', ['bikl_loss', 'js_loss'])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('K', [2, 5])
def test_reference_gradients_match_finite_differences(name, masked, K):
    zs, zw, mask = _fd_inputs(K, 2.0, 7 + K)
    m = mask if masked else None
    assert torch.autograd.gradcheck(lambda a, b: R.BY_NAME[name](a, b, m), (zs, zw), eps=1e-6, atol=1e-8, rtol=1e-6)
    # symmetric in its two arguments, zero (value and gradients) where they agree
    with torch.no_grad():
        assert float(R.BY_NAME[name](zs, zw, m)) == pytest.approx(float(R.BY_NAME[name](zw, zs, m)), rel=1e-13)
        assert abs(float(R.BY_NAME[name](zs, zs.clone(), m))) < 1e-15


@pytest.mark.parametrize('masked', [False, True])
def test_hard_label_reference(masked):
    zs, zw, mask = _fd_inputs(5, 2.0, 3)
    m = mask if masked else None
    assert torch.autograd.gradcheck(lambda a: R.hard_label_cross_entropy_loss(a, zw, m), (zs,), eps=1e-6, atol=1e-8, rtol=1e-6)
    loss = R.hard_label_cross_entropy_loss(zs, zw, m)
    loss.backward()
    assert zw.grad is None                                          # the target is a constant
    loss, zs = loss.detach(), zs.detach()
    # it is F.cross_entropy against the arg-max, and the first of equal maxima wins
    per = torch.nn.functional.cross_entropy(zs, zw.argmax(1), reduction='none')[:, None]
    want = (per * mask).sum() / mask.sum() if masked else per.mean()
    assert float(loss) == pytest.approx(float(want), rel=1e-13)
    tie = zw.detach().clone()
    tie[:, 1] = tie[:, 3] = tie.max() + 1.0
    assert float(R.hard_label_cross_entropy_loss(zs, tie, None)) == pytest.approx(float(-torch.log_softmax(zs, 1)[:, 1].mean()), rel=1e-13)


def test_js_is_bounded_by_ln2_where_the_views_disagree_completely():
    zs = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    zw = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    zs[:, 0], zw[:, 2] = 500.0, 500.0                              # gaps far beyond the underflow of exp()
    v = float(R.js_loss(zs, zw))
    assert np.isfinite(v) and abs(v - np.log(2.0)) < 1e-12
    zs.requires_grad_(True)
    R.js_loss(zs, zw).backward()
    assert torch.isfinite(zs.grad).all()
