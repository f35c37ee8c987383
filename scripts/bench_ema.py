#!/usr/bin/env python
"""Step time of EMA weight averaging at the benchmark shape, in one process: the eager full-flags PacingPseudo step (batch 32,
256x256, 5 classes, fused Adam) with ``ema_decay`` off / on.  The two settings ALTERNATE step by step on one model (the setting
is a key of the optimizer's param group; the shadow slab stays allocated), so clock and thermal drift hit both alike; each step
is timed with its own pair of events.  fp32 and bf16 activation storage.  Prints one JSON line.

`off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one setting against itself; a difference
between settings inside it is not resolved.

usage: python scripts/bench_ema.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--decay 0.999] [--storages fp32,bf16]
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

SETTINGS = ('off', 'on')


def time_storage(storage, a, batch, cli, device):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    a.storage = storage
    model = build(a, 'batch', 0, device)
    opt = FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd, ema_decay=cli.decay)
    group = opt.param_groups[0]
    model.train()
    for _ in range(cli.warmup):
        step(model, opt, batch, a, 0)
    value = dict(off=None, on=cli.decay)
    ms = {s: [] for s in SETTINGS}
    for i in range(cli.steps):
        for s in SETTINGS:
            group['ema_decay'] = value[s]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            loss = step(model, opt, batch, a, 0)
            ev[1].record()
            ms[s].append(ev)
    torch.cuda.synchronize()
    group['ema_decay'] = cli.decay
    ms = {s: [e0.elapsed_time(e1) for e0, e1 in v] for s, v in ms.items()}
    finite = bool(torch.isfinite(loss).item())
    shadow = next(iter(opt._slabs.values()))['ema']
    lag = float((shadow - model.flat.params).abs().max())             # (a host read, outside the timed steps)
    numel = model.flat.numel
    del model, opt
    torch.cuda.empty_cache()
    legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
    off = ms['off']
    return dict(legs=legs, off_halves_ms=[round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)],
                on_minus_off_ms=round(legs['on']['median_ms'] - legs['off']['median_ms'], 3),
                max_abs_shadow_minus_params=lag, slab_numel=numel, loss_finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--storages', type=str, default='fp32,bf16')
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    a = full_flags()
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    res = {s: time_storage(s, a, batch, cli, device) for s in cli.storages.split(',')}
    print(json.dumps(dict(metric='eager full-flags step time by ema_decay setting (alternating steps)', batch=cli.batch,
                          size=cli.size, ema_decay=cli.decay, steps_per_setting=cli.steps, warmup=cli.warmup, storage=res,
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
