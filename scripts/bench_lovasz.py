#!/usr/bin/env python
"""Cost of the Lovasz-softmax loss (upper_bound_chaos.py --do_loss_lovasz) in one process.

1. The loss alone, forward plus backward, at (32, 5, 256, 256) on the logits of the step's model and the synthetic phantom labels, in
   both modes (whole batch / per image), timed in WINDOWS of --reps calls between two device events; median (min .. max) over the
   windows.  Beside it, timed the same way on the same device: a torch composite of the same loss (soft-max, torch.sort, gather,
   cumsum, autograd backward), ``dice_loss_fn`` forward plus backward, and ``utils.sort_descending`` of (5, 32*256*256) alone.
2. The fully supervised step (bare U-Net, partial cross entropy + soft Dice, fused Adam) with the term off and on: the two settings
   ALTERNATE step by step on one model, so clock and thermal drift hit both alike; each step has its own pair of events.
   `off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one setting against itself; a difference
   between the settings inside it is not resolved.
Prints one JSON line.  There is no pass/fail threshold on time.

usage: python scripts/bench_lovasz.py [--windows 7] [--reps 5] [--steps 20] [--warmup 3] [--batch 32] [--size 256]
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


def torch_lovasz(z, cls, per_image):
    """The same loss as a composite of torch operators on the device (classes='present', no ignored pixel)."""
    import torch
    N = z.shape[0]
    p = torch.softmax(z, dim=1)
    p = p.flatten(2) if per_image else p.permute(1, 0, 2, 3).reshape(1, K, -1)          # (images, K, n)
    t = cls.reshape(N, -1) if per_image else cls.reshape(1, -1)
    fg = (t[:, None, :] == torch.arange(K, device=z.device)[None, :, None]).float()
    e = (fg - p).abs()
    es, perm = torch.sort(e, dim=2, descending=True, stable=True)
    fs = torch.gather(fg, 2, perm)
    G = fs.sum(2, keepdim=True)
    inter = G - fs.cumsum(2)
    union = G + (1.0 - fs).cumsum(2)
    J = 1.0 - inter / union
    g = torch.cat([J[..., :1], J[..., 1:] - J[..., :-1]], dim=2)
    present = (G[..., 0] > 0).float()
    per = ((es * g).sum(2) * present).sum(1) / present.sum(1).clamp(min=1)
    return per.mean()


def windows_ms(fn, windows, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(windows):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(reps):
            fn()
        e[1].record()
        evs.append(e)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) / reps for a, b in evs]
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7, help='timed windows per figure (at least 7)')
    ap.add_argument('--reps', type=int, default=5, help='calls per window')
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING of the whole step')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    cli = ap.parse_args()
    if cli.windows < 7:
        ap.error('--windows must be at least 7')
    import torch
    from pacingpseudo_amd.losses.losses import dice_loss_fn, lovasz_softmax_loss, partial_cross_entropy_loss
    from pacingpseudo_amd.models import UNet
    from pacingpseudo_amd.optim import FusedAdam
    from pacingpseudo_amd.utils import sort_descending
    device = torch.device('cuda', 0)
    torch.manual_seed(1)
    n = cli.batch
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
            loss = loss + 1.0 * lovasz_softmax_loss(logits, target, ignore_index=K)
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
    with torch.no_grad():
        logits = model(image)['segmentation/logits'].detach()
    del model, opt
    torch.cuda.empty_cache()
    z = logits.clone().requires_grad_(True)
    g = torch.ones((), device=device)

    def fwd_bwd(loss_fn):
        def run():
            z.grad = None
            loss_fn().backward(g)
        return run
    parts, agree = {}, {}
    for per_image in (False, True):
        mode = 'per_image' if per_image else 'batch'
        parts[mode] = dict(
            hip_fwd_bwd=windows_ms(fwd_bwd(lambda: lovasz_softmax_loss(z, cls, per_image=per_image)), cli.windows, cli.reps),
            hip_fwd=windows_ms(lambda: lovasz_softmax_loss(logits, cls, per_image=per_image), cli.windows, cli.reps),
            torch_composite_fwd_bwd=windows_ms(fwd_bwd(lambda: torch_lovasz(z, cls, per_image)), cli.windows, cli.reps))
        agree[mode] = abs(float(lovasz_softmax_loss(logits, cls, per_image=per_image)) - float(torch_lovasz(logits, cls, per_image)))
    parts['dice_loss_fn_fwd_bwd'] = windows_ms(fwd_bwd(lambda: dice_loss_fn(z, label)), cli.windows, cli.reps)
    keys = torch.rand(K, n * cli.size * cli.size, device=device)
    parts['sort_descending_alone'] = windows_ms(lambda: sort_descending(keys), cli.windows, cli.reps)
    parts['torch_sort_alone'] = windows_ms(lambda: torch.sort(keys, dim=1, descending=True, stable=True), cli.windows, cli.reps)
    print(json.dumps(dict(metric='Lovasz-softmax loss forward + backward alone (windows of device events: median, min, max) beside a torch '
                                 'composite, dice_loss_fn and the sort alone; the fully supervised step with the term off / on (alternating steps)',
                          shape=[n, K, cli.size, cli.size], windows=cli.windows, reps_per_window=cli.reps, steps_per_setting=cli.steps,
                          warmup=cli.warmup, parts=parts, hip_minus_torch_loss_abs=agree, step=dict(
                              legs=legs, off_halves_ms=[round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)],
                              on_minus_off_ms=round(legs['on']['median_ms'] - legs['off']['median_ms'], 3), loss_finite=finite),
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
