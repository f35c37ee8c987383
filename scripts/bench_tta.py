#!/usr/bin/env python
"""Cost of test-time augmentation (inference.py --tta) at the benchmark shape, in one process.  Prints one JSON line.

(a) Evaluation of one batch of --synthetic phantoms (batch 32, 256x256, 5 classes, the default U-Net widths, random weights) with
`--tta none`, `flips` and `d4`, ALTERNATING batch by batch (none, flips, d4, none, ...), so clock and thermal drift hit the modes
alike: the median of `predict_ms` (events around the forward passes and the TTA kernels; for `none` the forward pass alone) and of
`evaluate_ms` (wall clock of inference.evaluate on that batch: prediction, Dice counts, HD95 with its host part).
`none_halves_ms`: the medians of the even and the odd `none` samples -- the spread of one setting against itself.  The yardstick
for a mode with V views is V times the `none` figure.

(b) The three kernels against the torch composition they replace, on the same buffers: per op, pp_tta_accumulate (adding) against
`acc.add_(inverse(softmax(z, 1)))` with flip / transpose(...).contiguous(), pp_tta_view against the flip / transpose of the input,
and pp_tta_finalize against `acc.mul_(1 / V)` + `argmax(1)`.  Each figure is the median over --steps samples of --reps launches
between two events; `gbps` is the traffic model (accumulate: 3 K 4 B per pixel, view: 8 B per element, finalize: 8 K + 8 B per pixel)
over that time.

usage: python scripts/bench_tta.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--classes 5] [--reps 10]
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

MODES = ('none', 'flips', 'd4')


def timed(fn, reps, steps, warmup):
    """Median milliseconds of one call of fn: `steps` samples of `reps` calls between two events."""
    import torch
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) / reps


def torch_inverse(p, op):
    if op & 1:
        p = p.flip(-1)
    if op & 2:
        p = p.flip(-2)
    if op & 4:
        p = p.transpose(-1, -2)
    return p


def torch_view(x, op):
    if op & 4:
        x = x.transpose(-1, -2)
    if op & 2:
        x = x.flip(-2)
    if op & 1:
        x = x.flip(-1)
    return x.contiguous()


def bench_kernels(cli, device):
    import torch
    from pacingpseudo_amd._lib import lib, stream_ptr
    from pacingpseudo_amd.utils import tta_view
    N, K, H, W = cli.batch, cli.classes, cli.size, cli.size
    torch.manual_seed(0)
    z = torch.randn(N, K, H, W, device=device) * 3
    x = torch.randn(N, 1, H, W, device=device)
    acc = torch.zeros(N, K, H, W, device=device)
    cls = torch.empty(N, H, W, device=device, dtype=torch.int64)
    px = N * H * W
    out = {}
    for op in range(8):
        hip = timed(lambda: lib.pp_tta_accumulate(z.data_ptr(), N, K, H, W, op, 0, acc.data_ptr(), stream_ptr()), cli.reps, cli.steps, cli.warmup)
        ref = timed(lambda: acc.add_(torch_inverse(torch.softmax(z, 1), op).contiguous() if op & 4 else torch_inverse(torch.softmax(z, 1), op)),
                    cli.reps, cli.steps, cli.warmup)
        vh = timed(lambda: tta_view(x, op), cli.reps, cli.steps, cli.warmup)
        vt = timed(lambda: torch_view(x, op), cli.reps, cli.steps, cli.warmup)
        out[f'op{op}'] = dict(accumulate_ms=round(hip, 4), accumulate_torch_ms=round(ref, 4), accumulate_gbps=round(12.0 * K * px / hip / 1e6, 1),
                              view_ms=round(vh, 4), view_torch_ms=round(vt, 4), view_gbps=round(8.0 * px / vh / 1e6, 1))
        acc.zero_()
    acc.copy_(torch.softmax(z, 1))
    fin = timed(lambda: lib.pp_tta_finalize(acc.data_ptr(), N, K, H, W, 1, cls.data_ptr(), stream_ptr()), cli.reps, cli.steps, cli.warmup)
    ref = timed(lambda: acc.mul_(1.0).argmax(1), cli.reps, cli.steps, cli.warmup)
    out['finalize'] = dict(ms=round(fin, 4), torch_ms=round(ref, 4), gbps=round((8.0 * K + 8.0) * px / fin / 1e6, 1))
    return out


def bench_evaluate(cli, device):
    import torch
    from pacingpseudo_amd import inference as I
    from pacingpseudo_amd.data import SyntheticPhantoms, collate_by_shape, expand_compact
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.utils import tta_predict
    K = cli.classes
    torch.manual_seed(1)
    net = UNet(input_ch=1, init_ch=32, max_ch=512, num_classes=K, output_stride=8).to(device)
    net.eval()
    ds = SyntheticPhantoms(cli.batch, K, size=cli.size, train=False, seed=1, native=True, compact=True)
    batches = list(torch.utils.data.DataLoader(ds, batch_size=cli.batch, shuffle=False, num_workers=0, collate_fn=collate_by_shape))
    groups = batches[0] if isinstance(batches[0], list) else [batches[0]]
    image = expand_compact(groups[0], K, device)['image']

    def predict(mode):
        with torch.no_grad():
            if mode == 'none':
                return net(image)['segmentation/logits']
            return tta_predict(lambda t: net(t)['segmentation/logits'], image, mode)

    def evaluate(mode):
        return I.evaluate(net, batches, K, (1.62, 1.62), device, tta=mode, extra={})
    for _ in range(cli.warmup):
        for m in MODES:
            predict(m)
            evaluate(m)
    pred = {m: [] for m in MODES}
    wall = {m: [] for m in MODES}
    for _ in range(cli.steps):
        for m in MODES:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            predict(m)
            ev[1].record()
            pred[m].append(ev)
        for m in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate(m)
            torch.cuda.synchronize()
            wall[m].append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    pred = {m: [e0.elapsed_time(e1) for e0, e1 in v] for m, v in pred.items()}
    views = {'none': 1, 'flips': 4, 'd4': 8}
    res = {m: dict(views=views[m], predict_ms=round(statistics.median(pred[m]), 3), evaluate_ms=round(statistics.median(wall[m]), 3),
                   predict_over_views_x_none=round(statistics.median(pred[m]) / (views[m] * statistics.median(pred['none'])), 3)) for m in MODES}
    res['none_halves_ms'] = [round(statistics.median(pred['none'][0::2]), 3), round(statistics.median(pred['none'][1::2]), 3)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed samples per setting')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help='launches per sample in the kernel comparison')
    ap.add_argument('--skip_evaluate', action='store_true', help='only the kernel comparison (b)')
    cli = ap.parse_args()
    import torch
    device = torch.device('cuda', 0)
    res = dict(metric='test-time augmentation: evaluation per batch (alternating modes) and kernels against the torch composition',
               batch=cli.batch, size=cli.size, classes=cli.classes, steps=cli.steps, warmup=cli.warmup, reps=cli.reps)
    if not cli.skip_evaluate:
        res['evaluate'] = bench_evaluate(cli, device)
    res['kernels'] = bench_kernels(cli, device)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
