#!/usr/bin/env python
"""Step time by class count, in one process: the eager full-flags PacingPseudo step (batch 32, 256x256, fused Adam, train-mode
BatchNorm) at K = 5 (the benchmark's CHAOS head: MK = 8 kernels, four-pixel loss forms), 9 (MK = 16), 17 and 32 (MK = 32).  After
the timed steps, a few untimed steps under the library's event profiler give the 'loss' and 'spatial' family times per step (the
families whose traffic grows with K).  Prints one JSON line.

usage: python scripts/bench_classes.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--classes 5 9 17 32]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def step(model, opt, batch, a, epoch):
    """The iteration body of train_chaos.py:272-315 (losses weighted as train.py assembles them), as in bench_norm.py."""
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


def build(a, device):
    import torch
    from pacingpseudo_amd.models import ConsistencyRegulr
    torch.manual_seed(1)
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=a.input_ch, init_ch=a.init_ch, max_ch=a.max_ch, num_classes=a.num_classes,
                         output_stride=a.output_stride, is_stride_conv=False, is_trans_conv=False, elab_end_points=True),
        kwargs_aux_path=dict(num_classes=a.num_classes, feat_stage=a.feat_stage, feat_ch=a.feat_ch, hid_ch=a.hid_ch,
                             aux_drop_prob=a.aux_drop_prob, do_memory=a.do_memory, max_step=a.epoch,
                             update_momentum=a.update_momentum, ensemble_mode=a.ensemble_mode),
        args_parser=a)
    return model.to(device)


def time_leg(K, cli, device):
    import torch
    from pacingpseudo_amd._lib import PROF_KINDS, lib, prof_collect
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    from pacingpseudo_amd.optim import FusedAdam
    a = full_flags(num_classes=K, ignored_index=K)
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, K, seed=0).items() if k != 'label'}
    model = build(a, device)
    opt = FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd)
    model.train()
    for _ in range(cli.warmup):
        step(model, opt, batch, a, 0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(cli.steps + 1)]
    ev[0].record()
    for i in range(cli.steps):
        loss = step(model, opt, batch, a, 0)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(cli.steps)]
    finite = bool(torch.isfinite(loss).item())
    # untimed: loss and spatial family times per step from the event profiler
    kinds = ('loss', 'spatial')
    lib.pp_prof_select(sum(1 << PROF_KINDS.index(k) for k in kinds))
    lib.pp_prof_enable(1)
    prof_collect()
    for _ in range(cli.prof_steps):
        step(model, opt, batch, a, 0)
    torch.cuda.synchronize()
    lib.pp_prof_enable(0)
    prof = prof_collect()
    lib.pp_prof_select((1 << len(PROF_KINDS)) - 1)
    fam = {k: dict(ms_per_step=round(prof[k]['ms'] / cli.prof_steps, 4), launches_per_step=prof[k]['launches'] // cli.prof_steps,
                   alg_tb_per_s=round(prof[k]['bytes'] / (prof[k]['ms'] * 1e9), 3) if prof[k]['ms'] > 0 else None) for k in kinds}
    del model, opt, batch
    torch.cuda.empty_cache()
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                images_per_s=round(cli.batch / (statistics.median(ms) / 1e3), 1), loss_finite=finite, families=fam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--prof-steps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, nargs='+', default=[5, 9, 17, 32])
    cli = ap.parse_args()
    import torch
    device = torch.device('cuda', 0)
    legs = {f'K{K}': time_leg(K, cli, device) for K in cli.classes}
    base = legs.get('K5')
    ratios = {k: round(v['median_ms'] / base['median_ms'], 3) for k, v in legs.items()} if base else None
    print(json.dumps(dict(metric='eager full-flags step time by class count', batch=cli.batch, size=cli.size, steps=cli.steps,
                          warmup=cli.warmup, legs=legs, over_K5=ratios, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
