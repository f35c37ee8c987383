"""The regularisers on the weak logits as regop.py binds them: one table decides the order of their launches, their pairs in the plan's
sums block and their output keys, whatever subset is on; and the stand-alone loss functions make the engine's calls.

The smallest whole step the other step tests use: the narrow network, batch 2 at 64x64, a valid_mask with a zeroed rectangle.
"""
import itertools
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _ms_reference as R  # noqa: E402
from tests import _stream_hazards as H  # noqa: E402
from tests.test_gpu_step import build_model  # noqa: E402

SMALL = dict(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
NAMES = ('crf', 'nc', 'ms')
PARAMS = {'crf': dict(radius=3, dilation=2, sigma_xy=4.0, sigma_rgb=0.2), 'nc': dict(radius=4, dilation=1, sigma_xy=5.0, sigma_rgb=0.15),
          'ms': dict(tv_weight=0.7)}
WEIGHTS = {'loss_crf': 0.3, 'loss_nc': 0.2, 'loss_ms': 0.4}
EPOCH = 37
B, K, SIZE = 2, 5, 64


def _flags(subset, **over):
    on = {f'do_loss_{n}': True for n in subset}
    prm = {f'{n}_{k}': v for n in subset for k, v in PARAMS[n].items()}
    return O.full_flags(**SMALL, **on, **prm, **over)


def _batch():
    b = O.synthetic_batch(B, SIZE, SIZE, seed=3, keep=0.05)
    b['image'] = R.offset_image(B, 1, SIZE, SIZE, seed=3)
    b['image_strong'] = b['image'] * 1.3 - 0.2
    b['valid_mask'][:, :, 20:50, 10:40] = 0
    return {k: v.cuda() for k, v in b.items() if k != 'label'}


def _step(args):
    """One train step, forward and backward: (model, batch, outputs, plan)."""
    torch.manual_seed(1)
    model = build_model(args)
    model.train()
    batch = _batch()
    out = model(batch, mode='train', step=EPOCH)
    w = dict(O.loss_weights(args, EPOCH), **WEIGHTS)
    sum(out[k] * w[k] for k in out if k.startswith('loss_')).backward()
    torch.cuda.synchronize()
    return model, batch, out, model.engine.last_plan


def test_the_table_is_the_order():
    from pacingpseudo_amd.regop import REGULARISERS
    assert tuple(REGULARISERS) == NAMES and [r.key for r in REGULARISERS.values()] == ['loss_crf', 'loss_nc', 'loss_ms']


def test_launch_order_and_arguments_of_a_step_with_all_three_and_aux():
    with pytest.MonkeyPatch.context() as mp, H.Recording(mp) as rec:
        model, batch, out, plan = _step(_flags(NAMES))
    log = [(it[1], it[2]) for it in rec.log if it[0] == 'L' and re.match(r'pp_(seg_losses|crf_loss|nc_loss|ms_loss|aux_pce|losses_finalize)', it[1])]
    assert [n for n, _ in log].count('pp_aux_pce_fwd') == 1                 # on either stream: its place in the log is not fixed
    log = [(n, a) for n, a in log if not n.startswith('pp_aux_pce')]
    fwd, bwd = [(n, a) for n, a in log if not n.endswith('_bwd')], [(n, a) for n, a in log if n.endswith('_bwd')]
    assert [n for n, _ in fwd] == ['pp_seg_losses_fwd', 'pp_crf_loss_fwd', 'pp_nc_loss_fwd', 'pp_ms_loss_fwd'] + ['pp_losses_finalize'] * 5
    assert [n for n, _ in bwd] == ['pp_seg_losses_bwd', 'pp_crf_loss_bwd', 'pp_nc_loss_bwd', 'pp_ms_loss_bwd']
    sums = plan.all_sums
    assert sums.numel() == 14 and plan.aux['sums'].data_ptr() == sums[12:].data_ptr()
    # finalizes: the main one, one per regulariser reading its pair through the ratio slot ([2] / [3] of its first argument), the aux one
    fin = [a for n, a in fwd if n == 'pp_losses_finalize']
    assert [a[0] for a in fin] == [sums[i:].data_ptr() for i in (0, 4, 6, 8, 12)]
    assert [a[1] for a in fin] == [1, 1, 0, 1, 0]                           # has_mask: crf and ms 1, nc 0
    assert [a[3] for a in fin[1:4]] == [out[f'loss_{n}'].data_ptr() for n in NAMES] and all(a[2] is None and a[4] is None for a in fin[1:4])
    # forward launches: unit, (state,) sums, workspace, bytes are the RegOp's fields
    ops = plan.regs
    assert list(ops) == list(NAMES)
    image, mask, logits = batch['image'].data_ptr(), batch['valid_mask'].data_ptr(), out['segmentation/logits'].data_ptr()
    for (n, a), name, state in zip(fwd[1:4], NAMES, (False, True, True)):
        op = ops[name]
        assert op.sums.data_ptr() == sums[6 + 2 * NAMES.index(name):].data_ptr() and op.sums.numel() == 2
        assert a[:8] == [logits, image, mask, B, K, 1, SIZE, SIZE]
        assert a[8:8 + len(PARAMS[name])] == [pytest.approx(v) for v in PARAMS[name].values()]
        tail = [op.unit.data_ptr()] + ([op.state.data_ptr()] if state else []) + [op.sums.data_ptr(), op.ws.data_ptr(), op.ws_bytes]
        assert a[8 + len(PARAMS[name]):] == tail and (op.state is not None) == state
        assert op.ws.numel() == op.ws_bytes and tuple(op.unit.shape) == (B, K, SIZE, SIZE)
    # backward launches: behind the kernel that writes dlogits, each adds onto the same B*K*H*W floats of it
    dl, n_el = plan.dlogits.data_ptr(), B * K * SIZE * SIZE
    assert bwd[0][1][-2] == dl
    for (n, a), name in zip(bwd[1:], NAMES):
        op = ops[name]
        assert a[:2] == [op.unit.data_ptr(), op.sums.data_ptr()] and a[-2:] == [dl, n_el] and a[-3] == plan.loss_scale
        assert (a[2] == 1 and len(a) == 7) if name != 'nc' else len(a) == 6      # has_mask: crf and ms take it (1), nc has no such argument


SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(NAMES, r)]


@pytest.mark.parametrize('subset,aux', [(s, False) for s in SUBSETS] + [(('crf', 'ms'), True)], ids=lambda v: '+'.join(v) if isinstance(v, tuple) else f'aux={v}')
def test_any_subset_keeps_the_table_order(subset, aux):
    model, batch, out, plan = _step(_flags(subset, do_aux_path=aux, do_memory=aux))
    assert [k for k in out if k in WEIGHTS] == [f'loss_{n}' for n in subset]
    assert list(out) == model._expected_keys('train')
    assert list(plan.regs) == list(subset) == list(model.engine.regs)
    assert plan.all_sums.numel() == 8 + 2 * len(subset)
    for i, n in enumerate(subset):
        op = plan.regs[n]
        assert op.sums.data_ptr() == plan.all_sums[6 + 2 * i:].data_ptr() and op.sums.numel() == 2
        assert op.fin.data_ptr() == plan.all_sums[4 + 2 * i:].data_ptr()
        assert float(out[f'loss_{n}'].detach()) > 0
    # the auxiliary pair is the last one; a model with an auxiliary module keeps that slot with the path switched off, and nothing uses it
    assert ('loss_aux_cls' in out) == aux and plan.aux is not None
    assert plan.aux['sums'].data_ptr() == plan.all_sums[6 + 2 * len(subset):].data_ptr() and plan.aux['sums'].numel() == 2
    assert aux or (plan.aux['sums'] == 0).all()
    assert torch.isfinite(plan.dlogits).all()


@pytest.mark.parametrize('name', NAMES)
def test_the_stand_alone_function_is_the_engine_loss_bit_for_bit(name):
    """Both run the same RegOp calls on the same inputs through the same kernels (the parent of regop.py agreed bit for bit too)."""
    import pacingpseudo_amd.losses.losses as L
    fn = {'crf': L.gated_crf_loss, 'nc': L.normalized_cut_loss, 'ms': L.mumford_shah_loss}[name]
    model, batch, out, plan = _step(_flags((name,)))
    alone = fn(out['segmentation/logits'].detach(), batch['image'], batch['valid_mask'], **PARAMS[name])
    torch.cuda.synchronize()
    step = out[f'loss_{name}'].detach()
    print(f'{name}: engine {float(step)!r} function {float(alone)!r}')
    assert float(alone) > 0 and torch.equal(alone, step)
