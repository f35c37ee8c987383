#!/usr/bin/env python
"""Step time of the block normalisers at the benchmark shape, in one process: the eager full-flags PacingPseudo step (batch 32,
256x256, 5 classes, fused Adam) with train-mode BatchNorm (epoch 0 of the reference), eval-mode BatchNorm (the reference from
epoch 1 on, train_chaos.py:370) and GroupNorm blocks (--norm_op group).  Prints one JSON line.

usage: python scripts/bench_norm.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--groups 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(a, norm, groups, device):
    import torch
    from pacingpseudo_amd.models import ConsistencyRegulr
    torch.manual_seed(1)
    extra = dict(norm_op='group', norm_groups=groups) if norm == 'group' else {}
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=a.input_ch, init_ch=a.init_ch, max_ch=a.max_ch, num_classes=a.num_classes,
                         output_stride=a.output_stride, is_stride_conv=False, is_trans_conv=False, elab_end_points=True, **extra),
        kwargs_aux_path=dict(num_classes=a.num_classes, feat_stage=a.feat_stage, feat_ch=a.feat_ch, hid_ch=a.hid_ch,
                             aux_drop_prob=a.aux_drop_prob, do_memory=a.do_memory, max_step=a.epoch,
                             update_momentum=a.update_momentum, ensemble_mode=a.ensemble_mode),
        args_parser=a)
    return model.to(device)


def step(model, opt, batch, a, epoch):
    """The iteration body of train_chaos.py:272-315 (losses weighted as train.py assembles them)."""
    from pacingpseudo_amd.losses.losses import weighted_loss_sum
    from pacingpseudo_amd.utils import gaussian_ramp_up
    out = model(batch, mode='train', step=epoch)
    terms = [out['loss_pce'], out['loss_ent'], out['loss_cr'], out['loss_aux_cls'], out['loss_memory']]
    weights = [1.0, gaussian_ramp_up(epoch, a.loss_ent_weight, scale=a.ramp_up_scale),
               gaussian_ramp_up(epoch, a.loss_cr_weight, scale=a.ramp_up_scale), a.loss_aux_weight, a.loss_memory_weight]
    loss = weighted_loss_sum(terms, weights)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def time_leg(name, a, batch, cli, device):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    norm = 'group' if name == 'group_norm' else 'batch'
    model = build(a, norm, cli.groups, device)
    opt = FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd)
    epoch = 1 if name == 'bn_eval' else 0
    model.eval() if name == 'bn_eval' else model.train()
    for _ in range(cli.warmup):
        step(model, opt, batch, a, epoch)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(cli.steps + 1)]
    ev[0].record()
    for i in range(cli.steps):
        loss = step(model, opt, batch, a, epoch)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(cli.steps)]
    finite = bool(torch.isfinite(loss).item())
    del model, opt
    torch.cuda.empty_cache()
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                images_per_s=round(cli.batch / (statistics.median(ms) / 1e3), 1), loss_finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--groups', type=int, default=8)
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    a = full_flags()
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    legs = {name: time_leg(name, a, batch, cli, device) for name in ('bn_train', 'bn_eval', 'group_norm')}
    ratio = legs['group_norm']['median_ms'] / legs['bn_train']['median_ms']
    print(json.dumps(dict(metric='eager full-flags step time by block normaliser', batch=cli.batch, size=cli.size,
                          num_classes=a.num_classes, norm_groups=cli.groups, steps=cli.steps, warmup=cli.warmup, legs=legs,
                          group_over_bn_train=round(ratio, 3), device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
