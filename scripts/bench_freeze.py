#!/usr/bin/env python
"""Step time of fine-tuning with a frozen encoder prefix at the benchmark shape, in one process: the eager full-flags PacingPseudo
step (batch 32, 256x256, 5 classes, fused Adam) after ``freeze_encoder(N)`` for N = 0 .. 6, with the backbone's BatchNorm in train
mode (epoch 0 of a run) and in eval mode (every later epoch).  Each row is a fresh model -- freezing rebuilds the slab, and the
optimizer belongs to a slab -- with its own warm-up; every step is timed with its own pair of events.  An N = 0 row stands at the
start AND at the end of each mode: the difference between the two is the noise a row is to be read against.  Prints one JSON line.

usage: python scripts/bench_freeze.py [--steps 15] [--warmup 3] [--batch 32] [--size 256] [--storage fp32] [--modes train,eval]
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

ROWS = (0, 1, 2, 3, 4, 5, 6, 0)


def time_row(n, mode, a, batch, cli, device):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    model = build(a, 'batch', 0, device)
    if n:
        model.freeze_encoder(n)
    opt = FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd)
    epoch = 0 if mode == 'train' else 1
    model.train(mode == 'train')
    for _ in range(cli.warmup):
        step(model, opt, batch, a, epoch)
    evs = []
    for _ in range(cli.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        loss = step(model, opt, batch, a, epoch)
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    row = dict(n=n, median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
               slab_numel=model.flat.numel, loss_finite=bool(torch.isfinite(loss).item()))
    del model, opt
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=15, help='timed steps per row')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--storage', type=str, default='fp32')
    ap.add_argument('--modes', type=str, default='train,eval')
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    a = full_flags()
    a.storage = cli.storage
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    res = {}
    for mode in cli.modes.split(','):
        rows = [time_row(n, mode, a, batch, cli, device) for n in ROWS]
        first, last = rows[0]['median_ms'], rows[-1]['median_ms']
        base = 0.5 * (first + last)
        for r in rows:
            r['minus_n0_ms'] = round(r['median_ms'] - base, 3)
        res[mode] = dict(rows=rows, n0_first_ms=first, n0_last_ms=last, n0_spread_ms=round(abs(first - last), 3))
    print(json.dumps(dict(metric='eager full-flags step time by freeze_encoder(N), BatchNorm in train / eval mode', batch=cli.batch,
                          size=cli.size, steps_per_row=cli.steps, warmup=cli.warmup, storage=cli.storage, modes=res,
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
