"""``freeze_encoder(n)`` on the device: a frozen encoder prefix changes nothing it should not change, and launches nothing for it.

The small model of tests/test_gpu_step.py (its helpers and tolerances, imported), B = 2, 32 x 32, K = 5, output stride 8, full flags:
at this size all six stages, the three pooled boundaries and the two dilated stages exist.  (The two 16-bit storage cases run the
full widths on the same batch: that storage has kernels from 32 output channels up only.)

  * eval-mode BatchNorm: the frozen model IS the unfrozen one with some launches left out -- logits, losses and every trainable
    gradient bit-identical, frozen parameters without a gradient;
  * train-mode BatchNorm: frozen stages normalise with their running statistics and leave them alone, the rest runs in train mode
    -- against the float64 reference of tests/_freeze_reference.py, branch choices aligned as tests/test_gpu_step.py aligns them;
  * three Adam steps with the recipe's weight decay leave the frozen prefix bit-unchanged;
  * the launch log holds exactly the backward launches of the trainable layers, and no unordered cross-stream pair;
  * hipGraph replays equal eager steps; both drivers, --init_from and inference.py end to end.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pacing_oracle as O  # noqa: E402
from tests import _freeze_reference as R  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests import _stream_hazards as H  # noqa: E402
from tests.test_gpu_step import (TOL_OUT, build_model, check_grads, device_masks, device_pool_winners,  # noqa: E402
                                 iteration)

EPOCH = 37              # (ramp-up weights well above zero: every loss contributes)
B, SIZE, K = 2, 32, 5
LOSSES = ('loss_pce', 'loss_ent', 'loss_cr', 'loss_aux_cls', 'loss_memory')


def _small_args(**over):
    return O.full_flags(num_classes=K, ignored_index=K, init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], **over)


@functools.lru_cache(maxsize=None)
def _batch_cpu():
    return O.synthetic_batch(B, SIZE, SIZE, num_classes=K, seed=3, keep=0.08)


def _batch():
    return {k: v.cuda() for k, v in _batch_cpu().items() if k != 'label'}


def _build(variant='bn', storage='fp32'):
    """A fresh small model of one variant with non-trivial BatchNorm statistics and a non-empty bank (the same for every call)."""
    # (16-bit storage has split-fp16 kernels only, from 32 output channels up: those two cases run the full widths, 32 .. 512)
    args = _small_args() if storage == 'fp32' else O.full_flags(num_classes=K, ignored_index=K)
    args.storage = storage
    if variant == 'strided':
        args.is_stride_conv = args.is_trans_conv = True
    torch.manual_seed(1)
    if variant == 'gn':
        from tests.test_gpu_groupnorm import build_gn_model
        model = build_gn_model(args, groups=4)
    else:
        model = build_model(args)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith('running_mean'):
                v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
            elif k.endswith('running_var'):
                v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(v.device))
            elif k.endswith('memory_bank'):
                v.copy_((torch.randn(v.shape, generator=g) * 0.2).to(v.device))
    return model, args


def _total(out, args):
    w = O.loss_weights(args, EPOCH)
    return sum(out[k] * wt for k, wt in w.items())


def _step_once(variant, storage, n, train):
    """One forward + backward of a fresh model frozen at n: (outputs, {name: gradient or None}, the model)."""
    model, args = _build(variant, storage)
    if n:
        model.freeze_encoder(n)
    model.train(train)
    out = model(_batch(), mode='train', step=EPOCH)
    rec = {k: v.detach().clone() for k, v in out.items()}
    _total(out, args).backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return rec, grads, model


@functools.lru_cache(maxsize=None)
def _unfrozen(variant, storage, train):
    """The N = 0 run of one configuration, computed once and shared by its frozen cases."""
    rec, grads, model = _step_once(variant, storage, 0, train)
    del model
    return rec, grads


@pytest.fixture(scope='module', autouse=True)
def _drop_the_shared_runs():
    yield
    _unfrozen.cache_clear()
    torch.cuda.empty_cache()


def _frozen_keys(n):
    return R.frozen_prefixes(n)


# pooled boundary (1), unpooled boundary with `enc_rest` empty (4), auxiliary features partly frozen (5), whole encoder (6); then one
# case each of GroupNorm blocks (also in train(): they have no mode), the strided / transposed variant and the two 16-bit storages
IDENTITY = [('bn', 'fp32', 1, False), ('bn', 'fp32', 4, False), ('bn', 'fp32', 5, False), ('bn', 'fp32', 6, False),
            ('gn', 'fp32', 3, False), ('gn', 'fp32', 3, True), ('strided', 'fp32', 2, False),
            ('bn', 'fp16', 3, False), ('bn', 'bf16', 3, False)]


@pytest.mark.parametrize('variant,storage,n,train', IDENTITY)
def test_eval_mode_freezing_is_bit_identical(variant, storage, n, train):
    ref_out, ref_grads = _unfrozen(variant, storage, train)
    out, grads, model = _step_once(variant, storage, n, train)
    assert set(out) == set(ref_out)
    for k in ref_out:
        assert torch.equal(out[k], ref_out[k]), k
    for k in LOSSES:
        assert torch.isfinite(out[k]).all(), k
    pre = _frozen_keys(n)
    n_frozen = 0
    for k, p in model.named_parameters():
        if k.startswith(pre):
            assert grads[k] is None and p.grad is None and not p.requires_grad, k
            n_frozen += 1
        elif k == 'aux_path.memory_bank':
            assert grads[k] is None
        else:
            assert grads[k] is not None and torch.equal(grads[k], ref_grads[k]), k
    assert n_frozen == 8 * n
    assert float(ref_grads['backbone.dec_block1.conv_block.conv_layer2.conv.weight'].abs().max()) > 0
    # the slab holds the trainable parameters only
    assert all(not model.flat.owns(p) for k, p in model.named_parameters() if k.startswith(pre))
    assert sum(p.numel() for p in model.flat.offsets) == sum(p.numel() for p in model.parameters() if p.requires_grad)


def _reference_with_device_branches(model, start_state, args, n):
    """tests/_freeze_reference.train_step with the LeakyReLU branches and pool winners the device took (O.MASKS / O.POOLS, as
    tests/test_gpu_step.oracle_with_device_branches sets them), and its bounds on how much that alignment may have changed."""
    O.MASKS = device_masks(model)
    O.POOLS = pools = device_pool_winners(model)
    try:
        out, grads, total, post = R.train_step(start_state, _batch_cpu(), EPOCH, args, True, n)
        stats, pstats = list(O.MASK_STATS), list(O.POOL_STATS)
        total_act = sum(int(m.numel()) for ms in O.MASKS.values() for m in ms)
    finally:
        O.MASKS = None
        O.POOLS = None
    total_win = sum(int(i.numel()) for idx in pools.values() for i in idx)
    moved, gap = sum(c for _, c, _ in pstats), max([m for _, c, m in pstats if c] or [0.0])
    flipped, closest = sum(c for _, c, _ in stats), max([m for _, c, m in stats if c] or [0.0])
    assert moved <= max(16, 2e-5 * total_win) and gap < 1e-4, (moved, gap)
    assert flipped <= max(8, 2e-5 * total_act) and closest < 1e-4, (flipped, closest)
    return out, grads, total, post


@pytest.mark.parametrize('n', [1, 4])
def test_train_mode_mixed_batchnorm_against_float64(n):
    from pacingpseudo_amd.optim import FusedAdam
    model, args = _build()
    model.freeze_encoder(n)
    model.train()
    opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
    start = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    rec, grads = iteration(model, opt, _batch_cpu(), args, EPOCH)
    ref_out, ref_grads, ref_total, post = _reference_with_device_branches(model, start, args, n)
    for k, v in ref_out.items():
        e = G.rel_err(rec[k].double().cpu().numpy(), v.numpy())
        assert e < TOL_OUT, f'{k}: rel err {e:.3e}'
    assert abs(float(rec['total_loss']) - ref_total) < TOL_OUT * max(1.0, abs(ref_total))
    pre = _frozen_keys(n)
    assert all(not k.startswith(pre) for k in ref_grads) and len(ref_grads) == len(O.trainable_keys(start)) - 8 * n
    check_grads(grads, {k: v.numpy() for k, v in ref_grads.items() if v is not None}, True)
    for k, g in grads.items():
        if k.startswith(pre):
            assert g is None, k
    sd = model.state_dict()
    seen = 0
    for k, v in sd.items():
        if k in grads and k != 'aux_path.memory_bank':
            continue
        if k.startswith(pre):                                # running_mean / running_var / num_batches_tracked of a frozen stage
            assert torch.equal(v.cpu(), start[k]), k
            seen += 1
        elif v.dtype == torch.int64:                         # backbone: the weak and the strong pass; the auxiliary bottleneck: one call
            assert int(v) == int(post[k]) == int(start[k]) + (2 if k.startswith('backbone.') else 1), k
        else:
            assert G.rel_err(v.double().cpu().numpy(), post[k].numpy()) < TOL_OUT, k
            assert k.endswith('memory_bank') or not torch.equal(v.cpu(), start[k]), k
    assert seen == 6 * n


def test_three_adam_steps_leave_the_frozen_prefix_alone():
    from pacingpseudo_amd.optim import FusedAdam
    n = 3
    model, args = _build()
    model.freeze_encoder(n)
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for _ in range(3):
        iteration(model, opt, _batch_cpu(), args, EPOCH)
    torch.cuda.synchronize()
    pre = _frozen_keys(n)
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert len(trainable) == len(O.trainable_keys(start)) - 8 * n
    n_frozen = 0
    for k, v in model.state_dict().items():
        if k.startswith(pre):
            assert torch.equal(v, start[k]), k
            n_frozen += 1
        elif k in trainable:
            assert not torch.equal(v, start[k]), k
    assert n_frozen == 14 * n
    assert opt.state_dict()['slabs'][0]['steps'] == {'backbone': 3, 'aux_path': 3}


def _count(log, pattern):
    import re
    return sum(1 for it in log if it[0] == 'L' and re.match(pattern, it[1]))


@pytest.mark.parametrize('n', [1, 4, 6])
def test_launch_log_holds_the_trainable_layers_only(n):
    from pacingpseudo_amd.optim import FusedAdam
    steps = 2                                                # buffers and events are reused from the first step to the second
    with pytest.MonkeyPatch.context() as mp, H.Recording(mp) as rec:
        model, args = _build()
        model.freeze_encoder(n)
        model.train()
        opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
        torch.cuda.synchronize()
        for _ in range(steps):
            iteration(model, opt, _batch_cpu(), args, EPOCH)
        torch.cuda.synchronize()
        rec.name_events(model.engine.last_plan)
    log = rec.log
    layers = 2 * (6 - n) + 10 + 1                            # trainable 3x3 layers: encoder, decoder, the auxiliary bottleneck
    bwd = sorted({it[1] for it in log if it[0] == 'L' and 'bwd' in it[1]})
    assert _count(log, r'pp_conv3x3_(wino_)?bwd_weight') == steps * layers, bwd
    assert _count(log, r'pp_(bn|gn)_lrelu_bwd') == steps * layers, bwd
    assert _count(log, r'pp_conv3x3_(wino_)?bwd_data') == steps * (layers - 1), bwd
    # nothing flows into the frozen stages: the pooling in front of stage k is differentiated only when stage k - 1 trains
    pools_live = sum(1 for k, e in enumerate(model.backbone.enc_blocks(), start=1) if e.pooling is not None and k - 1 > n)
    assert _count(log, r'pp_maxpool2_bwd') + _count(log, r'pp_(bn|gn)_lrelu_bwd(_eval)?_pool') == steps * pools_live, bwd
    # the forward of the frozen stages: eval-mode coefficients per layer, no statistics update
    assert _count(log, r'pp_bn_eval_coeffs$') == steps * 2 * n
    assert _count(log, r'pp_bn_train_finalize') == steps * layers
    found, total = H.check(log)
    assert total == 0, H.report(found, total)


def test_graph_replays_equal_eager_steps():
    from pacingpseudo_amd.graph import GraphedStep
    from pacingpseudo_amd.optim import FusedAdam
    runs = {}
    for tag in ('eager', 'graph'):
        model, args = _build()
        model.freeze_encoder(3)
        model.train()
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)
        f = lambda out, epoch: _total(out, args)             # noqa: E731
        gs = GraphedStep(model, opt, f, warmup=1) if tag == 'graph' else None
        b = _batch()
        losses = []
        for _ in range(4):                                   # graph: one eager warm-up call, a capture, three replays in all
            if gs is None:
                out = model(b, mode='train', step=EPOCH)
                loss = f(out, EPOCH)
                opt.zero_grad()
                loss.backward()
                opt.step()
            else:
                loss, _ = gs(b, EPOCH)
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        if gs is not None:
            assert (gs.captures, gs.replays) == (1, 3)
        runs[tag] = (torch.stack(losses).cpu(), {k: v.detach().clone() for k, v in model.state_dict().items()})
    assert torch.isfinite(runs['eager'][0]).all() and torch.equal(runs['eager'][0], runs['graph'][0])
    for k, v in runs['eager'][1].items():
        assert torch.equal(v, runs['graph'][1][k]), k


def test_bare_unet_trains_with_a_frozen_prefix():
    """UNet.freeze_encoder on the stand-alone backbone (upper_bound.py): eval-mode identity with its own N = 0 run."""
    from pacingpseudo_amd.losses.losses import dice_loss_fn, partial_cross_entropy_loss
    from pacingpseudo_amd.models import UNet
    b = _batch_cpu()
    runs = {}
    for n in (0, 2, 6):
        torch.manual_seed(1)
        net = UNet(input_ch=1, init_ch=8, max_ch=64, num_classes=K, output_stride=8, elab_end_points=True).cuda()
        if n:
            net.freeze_encoder(n)
        net.eval()
        logits = net(b['image'].cuda())['segmentation/logits']
        label = b['label'].cuda()
        loss = partial_cross_entropy_loss(logits, label.argmax(1).long(), K) + dice_loss_fn(logits, label)
        loss.backward()
        torch.cuda.synchronize()
        runs[n] = (logits.detach().clone(), {k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()})
    for n in (2, 6):
        assert torch.equal(runs[n][0], runs[0][0])
        for k, g in runs[n][1].items():
            if k.startswith(tuple(f'enc_block{s}.' for s in range(1, n + 1))):
                assert g is None, k
            else:
                assert torch.equal(g, runs[0][1][k]), k


# ---------------------------------------------------------------------------------------------------------------- drivers
_COMMON = ['--synthetic', '8', '--epoch', '1', '--batch_size', '4', '--image_size', '32', '--num_workers', '0', '--cpu_input']
_FULL = ['--session', 'Experiment', '--do_loss_ent', '--do_decoder_consistency', '--do_aux_path', '--do_memory']


@pytest.fixture(scope='module')
def upper_bound_checkpoints(tmp_path_factory):
    """ckp_0.pth of two one-epoch upper_bound_chaos.py runs: 5 classes and 3 classes."""
    from pacingpseudo_amd.upper_bound import train_main as ub_main
    root = str(tmp_path_factory.mktemp('ub'))
    out = {}
    for k in (5, 3):
        ub_main(['--tag', f'ub{k}', '--root', root, '--num_classes', str(k), '--ignored_index', str(k)] + _COMMON)
        ck = glob.glob(os.path.join(root, 't1', 'Upperbound', f'Upperbound-*-fold1-ub{k}', 'ckps', 'ckp_0.pth'))
        assert len(ck) == 1
        out[k] = ck[0]
    return out


def test_drivers_fine_tune_from_a_checkpoint(tmp_path, upper_bound_checkpoints):
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.train import train_main
    init = torch.load(upper_bound_checkpoints[5], map_location='cpu')
    assert 'enc_block1.conv_block.conv_layer1.conv.weight' in init            # the bare U-Net layout
    root = str(tmp_path / 'out')
    vd = train_main(['--tag', 'ft', '--root', root, '--init_from', upper_bound_checkpoints[5], '--freeze_encoder', '6'] + _FULL + _COMMON)
    assert np.isfinite(vd).all()
    run = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-ft'))
    assert len(run) == 1
    log = open(os.path.join(run[0], 'log.txt')).read()
    assert 'initialised from' in log and '--freeze_encoder 6' in log
    sd = torch.load(os.path.join(run[0], 'ckps', 'ckp_0.pth'), map_location='cpu')
    enc = dec = 0
    for k, v in init.items():
        if k.startswith('enc_block'):
            assert torch.equal(sd['backbone.' + k], v), k
            enc += 1
        elif k.endswith(('conv.weight', 'norm_op.weight', 'running_mean', 'final_conv.weight')):
            assert not torch.equal(sd['backbone.' + k], v), k
            dec += 1
    assert enc == 6 * 14 and dec >= 5 * 2 * 3 + 1
    dicearr, _ = I.main(['--fold', '1', '--checkpoint_file', os.path.join(run[0], 'ckps', 'ckp_0.pth'), '--dataset', 'chaost1',
                         '--root', str(tmp_path / 'inf'), '--synthetic', '4', '--image_size', '32', '--batch_size', '2', '--num_workers', '0'])
    assert dicearr.shape == (4, 5)


def test_drivers_checkpoint_of_another_class_count(tmp_path, upper_bound_checkpoints, capsys):
    from pacingpseudo_amd.train import train_main
    root = str(tmp_path / 'out')
    argv = ['--root', root, '--init_from', upper_bound_checkpoints[3], '--freeze_encoder', '6'] + _FULL + _COMMON
    with pytest.raises(SystemExit) as e:
        train_main(['--tag', 'refused'] + argv)
    assert e.value.code == 2 and '--init_reset_head' in capsys.readouterr().err
    vd = train_main(['--tag', 'reset', '--init_reset_head'] + argv)
    assert np.isfinite(vd).all()
    run = glob.glob(os.path.join(root, 't1', 'Experiment', 'Experiment-*-fold1-reset'))
    sd = torch.load(os.path.join(run[0], 'ckps', 'ckp_0.pth'), map_location='cpu')
    init = torch.load(upper_bound_checkpoints[3], map_location='cpu')
    assert sd['backbone.final_conv.weight'].shape[0] == 5 and init['final_conv.weight'].shape[0] == 3
    assert torch.equal(sd['backbone.enc_block6.conv_block.conv_layer2.conv.weight'], init['enc_block6.conv_block.conv_layer2.conv.weight'])
