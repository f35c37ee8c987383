#!/usr/bin/env python
"""Step time of the EMA teacher (--cr_teacher ema) at the benchmark shape, in one process: the eager full-flags PacingPseudo step
(batch 32, 256x256, 5 classes, fused Adam with ``ema_decay``) with the teacher off ('none') / on ('ema').  The two settings
ALTERNATE step by step on one model (the engine's teacher table is switched; the shadow slab and the teacher plan stay allocated),
so clock and thermal drift hit both alike; each step is timed with its own pair of events.  Prints one JSON line.

`none_halves_ms`: the medians of the even and the odd `none` samples -- the spread of one setting against itself; a difference
between settings inside it is not resolved.
`teacher_pass_ms`: the teacher's pass by itself (weight packs from the shadow slab, image pack, eval-mode forward of `batch`
images through its forward-only plan), timed in the same process -- what `ema_minus_none_ms` is to be compared with (the two loss
calls and one finalize launch come on top).  `val_forward_ms`: an ordinary no-grad forward of the model on the same images
(mode 'val', eval-mode BatchNorm, its partial CE included), for scale.

usage: python scripts/bench_teacher.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--decay 0.999] [--storage fp32] [--bn_eval]
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

SETTINGS = ('none', 'ema')


def _timed(fn, n):
    import torch
    evs = []
    for _ in range(n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed steps PER SETTING')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--storage', type=str, default='fp32')
    ap.add_argument('--bn_eval', action='store_true', help="eval-mode BatchNorm in the student (the reference's state from epoch 1 on)")
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd._lib import stream_ptr
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
    table = dict(none=None, ema=eng.teacher)
    model.train(not cli.bn_eval)
    for s in SETTINGS * cli.warmup:
        eng.teacher = table[s]
        step(model, opt, batch, a, 0)
    ms = {s: [] for s in SETTINGS}
    for i in range(cli.steps):
        for s in SETTINGS:
            eng.teacher = table[s]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            loss = step(model, opt, batch, a, 0)
            ev[1].record()
            ms[s].append(ev)
    torch.cuda.synchronize()
    eng.teacher = table['ema']
    ms = {s: [e0.elapsed_time(e1) for e0, e1 in v] for s, v in ms.items()}
    finite = bool(torch.isfinite(loss).item())
    plan = eng.last_plan
    eng._frozen = eng._frozen_stages()
    alone = _timed(lambda: eng._teacher_forward(plan, batch['image'], stream_ptr()), cli.steps)
    mode = model.training
    model.eval()
    with torch.no_grad():
        for _ in range(cli.warmup):
            model(batch, mode='val')
        val = _timed(lambda: model(batch, mode='val'), cli.steps)
    model.train(mode)
    legs = {s: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for s, v in ms.items()}
    none = ms['none']
    print(json.dumps(dict(metric='eager full-flags step time by --cr_teacher setting (alternating steps)', batch=cli.batch, size=cli.size,
                          ema_decay=cli.decay, storage=cli.storage, student_bn='eval' if cli.bn_eval else 'train',
                          steps_per_setting=cli.steps, warmup=cli.warmup, legs=legs,
                          none_halves_ms=[round(statistics.median(none[0::2]), 3), round(statistics.median(none[1::2]), 3)],
                          ema_minus_none_ms=round(legs['ema']['median_ms'] - legs['none']['median_ms'], 3),
                          teacher_pass_ms=round(statistics.median(alone), 3), val_forward_ms=round(statistics.median(val), 3),
                          loss_finite=finite, device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
