#!/usr/bin/env python
"""Time the fused optimizers against each other on the benchmark's model: FusedAdam (the yardstick: its kernel is untouched),
FusedAdamW and FusedAdamW(exempt_1d=True), alternating in ONE process on ONE model.

Two figures per variant and repeat, both on the MI355X only (no GPU: the script fails, it does not fall back):
  * ``optimizer.step()`` alone: --inner calls between two device events on the gradients of one backward, time per call;
  * the whole eager step of bench.py (both passes, losses, backward, optimizer): --steps iterations under a host clock that ends
    in a device synchronise.
The three optimizers hold their own moments over the same parameter slab, so every variant streams the same addresses for p and g.
Bytes per parameter are what the update kernel must move (p, g, m, v read, p, m, v written: 28; the byte mask: 1 more), computed
here from the slab's size, not measured; GB/s = those bytes over the measured time of step() alone, launches and the norm-free host
side included -- a rate of the call, not of the kernel.  The spread is min .. max over the repeats.

    python scripts/bench_adamw.py [--batch 32 --size 256 --repeats 7 --inner 50 --steps 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=7, help='rounds over the three variants; the spread is taken over these')
    ap.add_argument('--inner', type=int, default=50, help='optimizer.step() calls per timed window')
    ap.add_argument('--steps', type=int, default=5, help='whole iterations per timed window')
    ap.add_argument('--warmup', type=int, default=3, help='untimed iterations per variant before the first round')
    ap.add_argument('--out', type=str, default=None, help='also write the JSON result here')
    return ap


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), spread_pct=100.0 * (max(xs) - min(xs)) / statistics.median(xs))


def main(argv=None):
    cli = build_parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_adamw.py measures on the GPU and found none')
    import bench
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    from pacingpseudo_amd.optim import FusedAdam, FusedAdamW

    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    a = full_flags()
    model = bench.build(a, device)
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    variants = {
        'FusedAdam': (FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd), 28.0),
        'FusedAdamW': (FusedAdamW(model.parameters(), lr=a.lr, weight_decay=a.wd), 28.0),
        'FusedAdamW(exempt_1d=True)': (FusedAdamW(model.parameters(), lr=a.lr, weight_decay=a.wd, exempt_1d=True), 29.0),
    }
    for opt, _ in variants.values():          # every shape and every code object of the timed windows, before the first of them
        for _ in range(cli.warmup):
            bench.train_iteration(model, opt, batch, a, 0)
    torch.cuda.synchronize()
    n = sum(b - s for s, b in model.flat.segments.values())
    exempt = int(next(iter(variants['FusedAdamW(exempt_1d=True)'][0]._slabs.values()))['exempt'].sum())
    step_us = {k: [] for k in variants}
    iter_ms = {k: [] for k in variants}
    order = list(variants)
    for r in range(cli.repeats):
        for name in order[r % 3:] + order[:r % 3]:          # alternate, and rotate who goes first
            opt, _ = variants[name]
            bench.train_iteration(model, opt, batch, a, 0)          # fresh gradients; also re-warms this variant's kernels
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(cli.inner):
                opt.step()
            t1.record()
            torch.cuda.synchronize()
            step_us[name].append(1e3 * t0.elapsed_time(t1) / cli.inner)
            tic = time.perf_counter()
            for _ in range(cli.steps):
                bench.train_iteration(model, opt, batch, a, 0)
            torch.cuda.synchronize()
            iter_ms[name].append(1e3 * (time.perf_counter() - tic) / cli.steps)
    assert bool(torch.isfinite(model.flat.params).all()), 'the parameters are not finite after the timed windows'
    result = dict(tool='bench_adamw', device=torch.cuda.get_device_name(0), batch=cli.batch, size=cli.size, parameters=n,
                  exempt_elements=exempt, repeats=cli.repeats, inner=cli.inner, steps=cli.steps, variants={})
    base = statistics.median(step_us['FusedAdam'])
    print(f'{n} slab elements ({exempt} exempt), batch {cli.batch} at {cli.size}x{cli.size}, {cli.repeats} repeats')
    print(f'{"variant":28s} {"step() us (min .. max)":>30s} {"spread":>8s} {"vs Adam":>8s} {"B/param":>8s} {"GB/s":>8s} {"iteration ms (min .. max)":>32s}')
    for name, (_, bpp) in variants.items():
        s, it = summary(step_us[name]), summary(iter_ms[name])
        gbs = bpp * n / (s['median'] * 1e-6) / 1e9
        result['variants'][name] = dict(step_us=s, iteration_ms=it, bytes_per_parameter=bpp, gb_per_s=gbs, step_vs_adam=s['median'] / base)
        print(f'{name:28s} {s["median"]:10.1f} ({s["min"]:7.1f} .. {s["max"]:7.1f}) {s["spread_pct"]:7.1f}% {s["median"] / base:8.3f} {bpp:8.0f} {gbs:8.0f} '
              f'{it["median"]:12.2f} ({it["min"]:7.2f} .. {it["max"]:7.2f})')
    line = json.dumps(result)
    print(line)
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, 'w') as f:
            f.write(line + '\n')
    return result


if __name__ == '__main__':
    main()
