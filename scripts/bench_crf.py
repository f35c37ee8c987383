#!/usr/bin/env python
"""Step time of the gated-CRF loss (--do_loss_crf) at the benchmark shape, in one process: the eager full-flags PacingPseudo step
(batch 32, 256x256, 5 classes, fused Adam) without and with the loss at its defaults (radius 5, dilation 1: 120 neighbours).  The
loss is a constant of an engine, so the two settings are two models built from one seed; their steps ALTERNATE (off, on, off, on,
...), so clock and thermal drift hit both alike, and each step is timed with its own pair of events.  fp32 and bf16 activation
storage.  Prints one JSON line.

`off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one setting against itself; a difference
between the settings inside it is not resolved.

usage: python scripts/bench_crf.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--storages fp32,bf16]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.bench_norm import build  # noqa: E402

SETTINGS = ('off', 'on')


def step(model, opt, batch, a, epoch):
    """The iteration body of train.py: the parent's five terms, plus loss_crf at --loss_crf_weight when the model has it."""
    from pacingpseudo_amd.losses.losses import weighted_loss_sum
    from pacingpseudo_amd.utils import gaussian_ramp_up
    out = model(batch, mode='train', step=epoch)
    terms = [out['loss_pce'], out['loss_ent'], out['loss_cr'], out['loss_aux_cls'], out['loss_memory']]
    weights = [1.0, gaussian_ramp_up(epoch, a.loss_ent_weight, scale=a.ramp_up_scale),
               gaussian_ramp_up(epoch, a.loss_cr_weight, scale=a.ramp_up_scale), a.loss_aux_weight, a.loss_memory_weight]
    if 'loss_crf' in out:
        terms.append(out['loss_crf'])
        weights.append(a.loss_crf_weight)
    loss = weighted_loss_sum(terms, weights)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss, out


def time_storage(storage, a, batch, cli, device):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    run = {}
    for s in SETTINGS:
        b = copy.copy(a)
        b.storage = storage
        b.do_loss_crf = s == 'on'
        model = build(b, 'batch', 0, device)
        model.train()
        run[s] = (model, FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd), b)
    for _ in range(cli.warmup):
        for s in SETTINGS:
            step(*run[s][:2], batch, run[s][2], 0)
    ms = {s: [] for s in SETTINGS}
    last = {}
    for i in range(cli.steps):
        for s in SETTINGS:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            last[s] = step(*run[s][:2], batch, run[s][2], 0)
            ev[1].record()
            ms[s].append(ev)
    torch.cuda.synchronize()
    ms = {s: [e0.elapsed_time(e1) for e0, e1 in v] for s, v in ms.items()}
    finite = all(bool(torch.isfinite(last[s][0]).item()) for s in SETTINGS)
    loss_crf = float(last['on'][1]['loss_crf'])
    assert 'loss_crf' not in last['off'][1]
    del run, last
    torch.cuda.empty_cache()
    legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
    off = ms['off']
    return dict(legs=legs, off_halves_ms=[round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)],
                on_minus_off_ms=round(legs['on']['median_ms'] - legs['off']['median_ms'], 3), loss_crf=loss_crf, loss_finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--storages', type=str, default='fp32,bf16')
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    a = full_flags(loss_crf_weight=0.1, crf_radius=5, crf_dilation=1, crf_sigma_xy=6.0, crf_sigma_rgb=0.1)
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    res = {s: time_storage(s, a, batch, cli, device) for s in cli.storages.split(',')}
    print(json.dumps(dict(metric='eager full-flags step time without / with the gated-CRF loss (alternating steps)', batch=cli.batch,
                          size=cli.size, steps_per_setting=cli.steps, warmup=cli.warmup, crf=dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1),
                          storage=res, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
