#!/usr/bin/env python
"""Cost of the surface metrics (inference.py --surface_metrics) against the HD95 path they replace, in one process.  Prints one
JSON line.

Two batches of hard class maps (batch 32, 256x256, 5 classes): `phantom` -- the labels of --synthetic phantoms against the same
labels with 3 % of the pixels re-drawn, the sizes a trained model leaves (1 - 3 k distances per item) -- and `noise`, uniform
noise against uniform noise (~10^5 distances per item, an early-training prediction).  Per batch:

  batch_hd95_ms             median wall clock of utils.metrics.batch_hd95: two launches, the copy of `dist` and `counts` to the
                            host, one numpy.percentile per (slice, class)
  batch_surface_metrics_ms  median wall clock of utils.metrics.batch_surface_metrics on the same inputs: the same two launches,
                            pp_surface_reduce, the copy of `counts` and `out`, the host finish
  distance_kernels_ms       pp_hd95_surface_distances alone, between two events (both paths pay it)
  reduce_kernel_ms          pp_surface_reduce alone, between two events
  *_bytes_to_host           what each path copies back
  largest_item / items      distances of the largest (slice, class) item and the number of items: one block per item, so the
                            reduce kernel cannot end before its largest item has

The calls ALTERNATE (hd95, surface, hd95, ...), so clock drift hits both alike; `hd95_halves_ms` is the median of the even and of
the odd batch_hd95 samples -- the spread of one setting against itself.

usage: python scripts/bench_surface.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--classes 5]
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


def make_batches(cli, device):
    import numpy as np
    import torch
    from pacingpseudo_amd.data import SyntheticPhantoms
    K = cli.classes
    ds = SyntheticPhantoms(cli.batch, K, size=cli.size, train=False, seed=1)
    label = torch.stack([ds[i]['label'].argmax(0) for i in range(cli.batch)]).to(torch.int64)
    rng = np.random.default_rng(0)
    pred = label.numpy().copy()
    hit = rng.random(pred.shape) < 0.03
    pred[hit] = rng.integers(0, K, int(hit.sum()))
    noise = [torch.as_tensor(rng.integers(0, K, pred.shape)) for _ in range(2)]
    return {'phantom': (torch.as_tensor(pred).to(device), label.to(device)), 'noise': (noise[0].to(device), noise[1].to(device))}


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def bench_batch(cli, pred, label):
    import torch
    from pacingpseudo_amd._lib import lib, stream_ptr
    from pacingpseudo_amd.utils.metrics import batch_hd95, batch_surface_metrics
    N, H, W = pred.shape
    K = cli.classes
    spacing = (1.62, 1.62)
    for _ in range(cli.warmup):
        batch_hd95(pred, label, K, spacing)
        batch_surface_metrics(pred, label, K, spacing)
    old, new = [], []
    for _ in range(cli.steps):
        old.append(wall(lambda: batch_hd95(pred, label, K, spacing)))
        new.append(wall(lambda: batch_surface_metrics(pred, label, K, spacing)))
    # the kernels alone, on buffers of their own
    dist = torch.empty((N * K, 2, H * W), device=pred.device, dtype=torch.float32)
    counts = torch.empty((N * K, 4), device=pred.device, dtype=torch.int32)
    out = torch.empty((N * K, 8), device=pred.device, dtype=torch.float64)
    nws = lib.pp_hd95_workspace(N, K, H, W)
    ws = torch.empty(nws, device=pred.device, dtype=torch.uint8)

    def distances():
        lib.pp_hd95_surface_distances(pred.data_ptr(), label.data_ptr(), N, K, H, W, spacing[0], spacing[1], dist.data_ptr(), counts.data_ptr(),
                                      ws.data_ptr(), nws, stream_ptr())

    def reduce():
        lib.pp_surface_reduce(dist.data_ptr(), counts.data_ptr(), N * K, H * W, 95.0, 2.0, out.data_ptr(), stream_ptr())

    def events(fn):
        samples = []
        for _ in range(cli.warmup + cli.steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            samples.append(ev)
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in samples[cli.warmup:])
    dist_ms = events(distances)
    red_ms = events(reduce)
    n = out.cpu().numpy()[:, 7]
    return dict(batch_hd95_ms=round(statistics.median(old), 3), batch_surface_metrics_ms=round(statistics.median(new), 3),
                hd95_halves_ms=[round(statistics.median(old[0::2]), 3), round(statistics.median(old[1::2]), 3)],
                distance_kernels_ms=round(dist_ms, 4), reduce_kernel_ms=round(red_ms, 4),
                hd95_bytes_to_host=dist.numel() * 4 + counts.numel() * 4, surface_bytes_to_host=out.numel() * 8 + counts.numel() * 4,
                items=N * K, largest_item=int(n.max()), median_item=int(statistics.median(n.tolist())), distances=int(n.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed calls per setting')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    cli = ap.parse_args()
    import torch
    device = torch.device('cuda', 0)
    res = dict(metric='surface metrics: batch_hd95 against batch_surface_metrics on the same class maps (alternating calls, median)',
               batch=cli.batch, size=cli.size, classes=cli.classes, steps=cli.steps, warmup=cli.warmup)
    for name, (pred, label) in make_batches(cli, device).items():
        res[name] = bench_batch(cli, pred, label)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
