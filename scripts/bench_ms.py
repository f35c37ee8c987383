#!/usr/bin/env python
"""Step time of the Mumford-Shah level-set loss (--do_loss_ms) at the benchmark shape, in one process: the eager full-flags
PacingPseudo step (batch 32, 256x256, 5 classes, fused Adam) with the loss off and on (--ms_tv_weight 1), and optionally beside the
gated-CRF and normalised-cut losses (`all`: the three regularisers, the run a kernel trace is taken from).  The loss is a constant
of an engine, so the settings are models built from one seed; their steps ALTERNATE (off, on, then on, off, ...: the round's first
setting rotates), so clock and thermal drift hit all alike, and each step is timed with its own pair of events.  fp32 and bf16
activation storage.  Prints one JSON line.

`off_halves_ms`: the medians of the even and the odd `off` samples -- the spread of one setting against itself; a difference
between the settings inside it is not resolved.

usage: python scripts/bench_ms.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--storages fp32,bf16] [--settings off,on]
       python scripts/bench_ms.py --settings all --steps 8 --warmup 0 --storages fp32      # eight eager steps for a kernel trace
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

SETTINGS = {'off': (False, False, False), 'on': (False, False, True), 'all': (True, True, True)}      # (do_loss_crf, do_loss_nc, do_loss_ms)
KEYS = ('loss_crf', 'loss_nc', 'loss_ms')


def step(model, opt, batch, a, epoch):
    """The iteration body of train.py: the parent's five terms, plus the regularisers at their weights when the model has them."""
    from pacingpseudo_amd.losses.losses import weighted_loss_sum
    from pacingpseudo_amd.utils import gaussian_ramp_up
    out = model(batch, mode='train', step=epoch)
    terms = [out['loss_pce'], out['loss_ent'], out['loss_cr'], out['loss_aux_cls'], out['loss_memory']]
    weights = [1.0, gaussian_ramp_up(epoch, a.loss_ent_weight, scale=a.ramp_up_scale),
               gaussian_ramp_up(epoch, a.loss_cr_weight, scale=a.ramp_up_scale), a.loss_aux_weight, a.loss_memory_weight]
    for name, w in zip(KEYS, (a.loss_crf_weight, a.loss_nc_weight, a.loss_ms_weight)):
        if name in out:
            terms.append(out[name])
            weights.append(w)
    loss = weighted_loss_sum(terms, weights)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss, out


def time_storage(storage, a, batch, cli, device, settings):
    import torch
    from pacingpseudo_amd.optim import FusedAdam
    run = {}
    for s in settings:
        b = copy.copy(a)
        b.storage = storage
        b.do_loss_crf, b.do_loss_nc, b.do_loss_ms = SETTINGS[s]
        model = build(b, 'batch', 0, device)
        model.train()
        run[s] = (model, FusedAdam(model.parameters(), lr=a.lr, weight_decay=a.wd), b)
    for _ in range(cli.warmup):
        for s in settings:
            step(*run[s][:2], batch, run[s][2], 0)
    ms = {s: [] for s in settings}
    last = {}
    for i in range(cli.steps):
        for s in settings[i % len(settings):] + settings[:i % len(settings)]:      # every setting follows every other equally often
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            last[s] = step(*run[s][:2], batch, run[s][2], 0)
            ev[1].record()
            ms[s].append(ev)
    torch.cuda.synchronize()
    ms = {s: [e0.elapsed_time(e1) for e0, e1 in v] for s, v in ms.items()}
    finite = all(bool(torch.isfinite(last[s][0]).item()) for s in settings)
    for s in settings:
        assert tuple(k in last[s][1] for k in KEYS) == SETTINGS[s], s
    losses = {s: {k: float(last[s][1][k].detach()) for k in KEYS if k in last[s][1]} for s in settings}
    del run, last
    torch.cuda.empty_cache()
    legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
    res = dict(legs=legs, losses=losses, loss_finite=finite)
    if 'off' in ms:
        off = ms['off']
        res['off_halves_ms'] = [round(statistics.median(off[0::2]), 3), round(statistics.median(off[1::2]), 3)]
        res['minus_off_ms'] = {s: round(legs[s]['median_ms'] - legs['off']['median_ms'], 3) for s in settings if s != 'off'}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--storages', type=str, default='fp32,bf16')
    ap.add_argument('--settings', type=str, default='off,on')
    cli = ap.parse_args()
    settings = tuple(cli.settings.split(','))
    if not settings or any(s not in SETTINGS for s in settings):
        ap.error(f'--settings: a comma-separated subset of {",".join(SETTINGS)}')
    import torch
    from pacingpseudo_amd.data import full_flags, synthetic_batch
    device = torch.device('cuda', 0)
    prm = dict(radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1)
    a = full_flags(loss_crf_weight=0.1, loss_nc_weight=0.1, loss_ms_weight=0.1, ms_tv_weight=1.0, **{f'crf_{k}': v for k, v in prm.items()},
                   **{f'nc_{k}': v for k, v in prm.items()})
    batch = {k: v.to(device) for k, v in synthetic_batch(cli.batch, cli.size, cli.size, a.num_classes, seed=0).items() if k != 'label'}
    res = {s: time_storage(s, a, batch, cli, device, settings) for s in cli.storages.split(',')}
    print(json.dumps(dict(metric='eager full-flags step time: Mumford-Shah loss off / on / beside the gated-CRF and normalised-cut losses '
                                 '(alternating steps)', batch=cli.batch, size=cli.size, steps_per_setting=cli.steps, warmup=cli.warmup,
                          tv_weight=1.0, storage=res, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
