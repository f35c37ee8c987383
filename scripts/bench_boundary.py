#!/usr/bin/env python
"""Cost of the boundary loss (upper_bound_chaos.py --do_loss_boundary) in one process: the fully supervised step (bare U-Net, partial
cross entropy + soft Dice, fused Adam) at batch 12 and batch 32, 256x256, 5 classes, with the term off and on.  The two settings
ALTERNATE step by step on one model, so clock and thermal drift hit both alike; each step is timed with its own pair of events.
`off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one setting against itself; a difference
between settings inside it is not resolved.

Then ``signed_distance_maps`` and the loss forward and backward alone, with device events, on the synthetic phantom labels of the
step and on one adversarial label (a single foreground pixel in a corner: the longest scans of the row pass), beside the HBM floor of
the map kernels -- 8 N H W bytes read + 4 N K H W bytes written at the streaming rate DESIGN.md section 7 records for
grad_sumsq_kernel / adam_kernel (--stream_tbps).  Prints one JSON line.

usage: python scripts/bench_boundary.py [--steps 20] [--warmup 3] [--batches 12,32] [--size 256] [--stream_tbps 6.5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 5


def phantom_batch(n, size, device):
    """(image (n, 1, S, S), one-hot label (n, K, S, S), class map (n, S, S)) of data.SyntheticPhantoms, on the device."""
    import numpy as np
    import torch
    from pacingpseudo_amd.data import SyntheticPhantoms
    ds = SyntheticPhantoms(n, K, size=size, seed=1)
    arrays = [ds.raw_arrays(i) for i in range(n)]
    image = torch.from_numpy(np.stack([a[0] for a in arrays]))[:, None].to(device)
    cls = torch.from_numpy(np.stack([a[1] for a in arrays])).to(device)
    label = torch.nn.functional.one_hot(cls, K).permute(0, 3, 1, 2).float().contiguous()
    return image, label, cls


def _median_ms(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        evs.append(e)
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in evs), 4)


def time_batch(n, cli, device):
    import torch
    from pacingpseudo_amd.losses.losses import boundary_loss, dice_loss_fn, partial_cross_entropy_loss
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.optim import FusedAdam
    from pacingpseudo_amd.utils import signed_distance_maps
    torch.manual_seed(1)
    model = UNet(input_ch=1, init_ch=32, max_ch=512, num_classes=K, output_stride=8, is_stride_conv=False, is_trans_conv=False,
                 elab_end_points=True).to(device)
    opt = FusedAdam(model.parameters(), lr=1e-4, weight_decay=3e-4)
    image, label, cls = phantom_batch(n, cli.size, device)
    model.train()

    def step(on):
        logits = model(image)['segmentation/logits']
        target = torch.argmax(label, dim=1).long()
        loss = partial_cross_entropy_loss(logits, target, K) + dice_loss_fn(logits, label)
        if on:
            loss = loss + 0.01 * boundary_loss(logits, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for _ in range(cli.warmup):
        step(False)
        step(True)
    ms = dict(off=[], on=[])
    for _ in range(cli.steps):
        for s in ('off', 'on'):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            loss = step(s == 'on')
            ev[1].record()
            ms[s].append(ev)
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(loss).item())
    ms = {s: [a.elapsed_time(b) for a, b in v] for s, v in ms.items()}
    legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
    off = ms['off']
    # the pieces alone
    with torch.no_grad():
        logits = model(image)['segmentation/logits'].detach()
    corner = torch.zeros_like(cls)
    corner[:, 0, 0] = 1                                        # adversarial: one foreground pixel in a corner
    floor_bytes = 8 * n * cli.size * cli.size + 4 * n * K * cli.size * cli.size
    floor_ms = round(floor_bytes / (cli.stream_tbps * 1e12) * 1e3, 4)
    parts = {}
    for name, c in (('phantom', cls), ('corner', corner)):
        phi = signed_distance_maps(c, K)
        z = logits.clone().requires_grad_(True)
        g = torch.ones((), device=device)

        def fwd_bwd():
            z.grad = None
            boundary_loss(z, None, dist_maps=phi).backward(g)
        fwd_ms = _median_ms(lambda: boundary_loss(logits, None, dist_maps=phi), cli.steps)
        parts[name] = dict(signed_maps_ms=_median_ms(lambda: signed_distance_maps(c, K), cli.steps), loss_fwd_ms=fwd_ms,
                           loss_fwd_bwd_ms=_median_ms(fwd_bwd, cli.steps))
    del model, opt
    torch.cuda.empty_cache()
    return dict(legs=legs, off_halves_ms=[round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)],
                on_minus_off_ms=round(legs['on']['median_ms'] - legs['off']['median_ms'], 3), parts=parts,
                maps_hbm_floor_bytes=floor_bytes, maps_hbm_floor_ms=floor_ms, loss_finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', type=str, default='12,32')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--stream_tbps', type=float, default=6.5, help="streaming rate of the HBM floor, TB/s (DESIGN.md section 7: adam_kernel 6.5 - 6.7, grad_sumsq_kernel 4.6)")
    cli = ap.parse_args()
    import torch
    device = torch.device('cuda', 0)
    res = {b: time_batch(int(b), cli, device) for b in cli.batches.split(',')}
    print(json.dumps(dict(metric='fully supervised step time with the boundary loss off / on (alternating steps), and its parts alone',
                          size=cli.size, classes=K, steps_per_setting=cli.steps, warmup=cli.warmup, stream_tbps=cli.stream_tbps,
                          batch=res, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
