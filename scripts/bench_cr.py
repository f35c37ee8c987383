#!/usr/bin/env python
"""Step time of the seven --loss_cr_variants (ce_loss, l1_loss, l2_loss, kl_loss, bikl_loss, js_loss, hard_ce_loss) at the benchmark
shape, in one process: the eager full-flags PacingPseudo step (batch 32, 256x256, 5 classes, fused Adam), one model per variant built
from one seed, the variants one after the other (one engine's buffers on the device at a time), each step timed with its own pair of
events.  The default, ce_loss, runs first AND last (`ce_loss_again`): the difference of its two medians is the spread of one setting
against itself in this process; a difference between variants inside it is not resolved.

`kernels_ms`: the fused loss launches alone -- pp_seg_losses_fwd + pp_seg_losses_bwd on random logits of the same shape -- per variant.

Prints one JSON line.

usage: python scripts/bench_cr.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--variants ce_loss,js_loss]
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

from scripts.bench_norm import build, step  # noqa: E402


def time_variant(name, a, batch, cli, device):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    b = copy.copy(a)
    b.loss_cr_variants = name
    model = build(b, 'batch', 0, device)
    model.train()
    opt = FusedAdam(model.parameters(), lr=b.lr, weight_decay=b.wd)
    for _ in range(cli.warmup):
        step(model, opt, batch, b, cli.epoch)
    evs = []
    for _ in range(cli.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        loss = step(model, opt, batch, b, cli.epoch)
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    res = dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
               loss_finite=bool(torch.isfinite(loss).item()))
    del model, opt, loss
    torch.cuda.empty_cache()
    return res


def time_kernels(code, cli, device, K=5, reps=20):
    """pp_seg_losses_fwd + pp_seg_losses_bwd alone, full flags (entropy on, mask), median of `reps` pairs."""
    import torch
    from pacingpseudo_amd._lib import lib, stream_ptr
    N, HW = cli.batch, cli.size * cli.size
    g = torch.Generator(device='cpu').manual_seed(0)
    zw = (torch.randn(N, K, HW, generator=g) * 2).to(device)
    zs = (torch.randn(N, K, HW, generator=g) * 2).to(device)
    t = torch.randint(0, K + 1, (N, HW), generator=g).to(device)
    mask = torch.ones(N, 1, HW, device=device)
    sums = torch.zeros(6, dtype=torch.float64, device=device)
    nws = lib.pp_seg_losses_workspace(N, HW)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    one = torch.ones((), device=device)
    dzw, dzs = torch.empty_like(zw), torch.empty_like(zs)
    st = stream_ptr()

    def pair():
        lib.pp_seg_losses_fwd(zw.data_ptr(), zs.data_ptr(), t.data_ptr(), mask.data_ptr(), N, K, HW, K, 1, code, sums.data_ptr(),
                              ws.data_ptr(), nws, st)
        lib.pp_seg_losses_bwd(zw.data_ptr(), zs.data_ptr(), t.data_ptr(), mask.data_ptr(), N, K, HW, K, 1, code, 0, sums.data_ptr(),
                              one.data_ptr(), one.data_ptr(), one.data_ptr(), 1.0, dzw.data_ptr(), dzs.data_ptr(), st)
    for _ in range(3):
        pair()
    evs = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        pair()
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    return round(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs), 4)


def main():
    from pacingpseudo_amd.engine import CR_VARIANTS
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER VARIANT')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--epoch', type=int, default=100, help='epoch of the timed steps (100: past the ramp-up, the consistency loss at full weight)')
    ap.add_argument('--variants', type=str, default=','.join(CR_VARIANTS))
    cli = ap.parse_args()
    variants = cli.variants.split(',')
    if not variants or any(v not in CR_VARIANTS for v in variants):
        ap.error(f'--variants: a comma-separated subset of {",".join(CR_VARIANTS)}')
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    a = full_flags()
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    legs = {v: time_variant(v, a, batch, cli, device) for v in variants}
    if 'ce_loss' in legs:
        legs['ce_loss_again'] = time_variant('ce_loss', a, batch, cli, device)
    kernels = {v: time_kernels(CR_VARIANTS[v], cli, device) for v in variants}
    print(json.dumps(dict(metric='eager full-flags step time per --loss_cr_variants (one model per variant, one after the other)',
                          batch=cli.batch, size=cli.size, steps_per_variant=cli.steps, warmup=cli.warmup, epoch=cli.epoch, legs=legs,
                          kernels_ms=kernels, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
