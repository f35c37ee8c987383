#!/usr/bin/env python
"""Step time of the uncertainty mask (--cr_uncertainty) at the benchmark shape, in one process: the eager full-flags PacingPseudo
step (batch 32, 256x256, 5 classes, fused Adam with ``ema_decay``, the EMA teacher attached) with the mask off / on, for
T = 1 with sigma = 0 (the plain entropy of the clean teacher pass: one streaming launch), T = 4 and T = 8 (sigma 0.1).  Per
setting the two legs ALTERNATE step by step on one model (the engine's settings are switched; the state buffer and the teacher
plan's buffers stay allocated), so clock and thermal drift hit both alike; each step is timed with its own pair of events.
Prints one JSON line.

`off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one leg against itself; a difference inside it
is not resolved.  The expectation for `on_minus_off_ms` is T eval-mode forwards of `batch` images (scripts/bench_teacher.py:
`teacher_pass_ms`, which includes the weight packs the noisy passes do not repeat) plus 2 T + 1 streaming launches.

usage: python scripts/bench_uncertainty.py [--steps 12] [--warmup 2] [--batch 32] [--size 256] [--decay 0.999] [--storage fp32] [--bn_eval]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.bench_norm import build, step  # noqa: E402

SETTINGS = ((1, 0.0), (4, 0.1), (8, 0.1))      # (T, sigma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=12, help='timed steps PER LEG and setting')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--storage', type=str, default='fp32')
    ap.add_argument('--bn_eval', action='store_true', help="eval-mode BatchNorm in the student (the reference's state from epoch 1 on)")
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    from pacingpseudo_amd.optim import FusedAdam
    device = torch.device('cuda', 0)
    a = full_flags()
    a.storage = cli.storage
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    model = build(a, 'batch', 0, device)
    opt = FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd, ema_decay=cli.decay)
    model.attach_teacher(opt)
    eng = model.engine
    model.train(not cli.bn_eval)
    results = []
    for T, sigma in SETTINGS:
        eng.set_uncertainty(T, sigma=sigma, clip=0.2, start=0.75, seed=1)
        table = dict(off=None, on=eng.unc)
        for s in ('off', 'on') * cli.warmup:
            eng.unc = table[s]
            step(model, opt, batch, a, 0)
        ms = dict(off=[], on=[])
        for _ in range(cli.steps):
            for s in ('off', 'on'):
                eng.unc = table[s]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                loss = step(model, opt, batch, a, 0)
                ev[1].record()
                ms[s].append(ev)
        torch.cuda.synchronize()
        ms = {s: [e0.elapsed_time(e1) for e0, e1 in v] for s, v in ms.items()}
        st = eng.uncertainty_stats().cpu().tolist()
        legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
        off = ms['off']
        results.append(dict(passes=T, sigma=sigma, legs=legs,
                            off_halves_ms=[round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)],
                            on_minus_off_ms=round(legs['on']['median_ms'] - legs['off']['median_ms'], 3),
                            kept=round(st[0] / max(st[2], 1.0), 4), mean_entropy=round(st[1] / max(st[2], 1.0), 4),
                            loss_finite=bool(torch.isfinite(loss).item())))
    eng.set_uncertainty(None)
    print(json.dumps(dict(metric='eager full-flags step time with the EMA teacher, --cr_uncertainty off / on (alternating steps)',
                          batch=cli.batch, size=cli.size, ema_decay=cli.decay, storage=cli.storage,
                          student_bn='eval' if cli.bn_eval else 'train', steps_per_leg=cli.steps, warmup=cli.warmup, settings=results,
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
