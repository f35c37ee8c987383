#!/usr/bin/env python
"""Time of one random-walker expansion call (--rw_scribbles) at the driver's batch: 32 synthetic phantoms of
256 x 256 with 5 classes at the default parameters -- pprep_rw_solve + pprep_rw_labels between one pair of events per call (the
workspace and output allocations are outside), the solver's iteration counts and worst true residual, and for context the time
scipy's float64 sparse direct solve (splu, all classes of a slice from one factorisation) takes per slice on this host's CPU.
The cost is paid once per run, not per step.  Prints one JSON line.

usage: python scripts/bench_rw.py [--steps 5] [--warmup 1] [--batch 32] [--size 256] [--classes 5] [--cpu_slices 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--cpu_slices', type=int, default=2, help='slices timed with scipy splu (0 = skip)')
    cli = ap.parse_args()
    import numpy as np
    import torch
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._prep import prep
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import check_rw_params
    device = torch.device('cuda', 0)
    N, K, S = cli.batch, cli.classes, cli.size
    prm = check_rw_params(K=K)
    ds = SyntheticPhantoms(N, K, size=S, raw=True)
    raw = [ds.raw_arrays(i) for i in range(N)]
    img = torch.from_numpy(np.stack([r[0] for r in raw]).astype(np.float32)).to(device)
    scb = torch.from_numpy(np.stack([r[2] for r in raw]).astype(np.int32)).to(device)
    prob = torch.empty((N, K, S, S), device=device)
    stats = torch.empty((N, K, 3), device=device)
    out = torch.empty((N, S, S), device=device, dtype=torch.int32)
    ws = torch.empty(prep.pprep_rw_workspace_bytes(N, K, S, S), device=device, dtype=torch.uint8)

    def call():
        prep.pprep_rw_solve(img.data_ptr(), scb.data_ptr(), None, N, K, S, S, prm['beta'], prm['eps'], prm['tol'], prm['max_iters'],
                            prob.data_ptr(), stats.data_ptr(), ws.data_ptr(), stream_ptr())
        prep.pprep_rw_labels(prob.data_ptr(), scb.data_ptr(), None, N, K, S, S, prm['threshold'], out.data_ptr(), stream_ptr())

    for _ in range(cli.warmup):
        call()
    evs = []
    for _ in range(cli.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call()
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    st = stats.cpu().numpy()
    its = st[:, :, 0][st[:, :, 0] > 0]
    res = dict(metric='random-walker expansion, one call (solve + labels)', batch=N, size=S, classes=K, steps=cli.steps, warmup=cli.warmup,
               params=prm, median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
               systems=int(N * K), systems_solved=int(its.size),
               iterations=dict(min=int(its.min()), median=float(np.median(its)), max=int(its.max())) if its.size else None,
               worst_relres=float(st[:, :, 1].max()), unconverged=int((st[:, :, 2] < 0.5).sum()),
               coverage_before=float((scb != K).float().mean()), coverage_after=float((out != K).float().mean()),
               workspace_mib=round(ws.numel() / 2 ** 20, 1), device=torch.cuda.get_device_name(0))
    if cli.cpu_slices:
        from tests import _rw_reference as R
        cpu = []
        for i in range(min(cli.cpu_slices, N)):
            t0 = time.perf_counter()
            R.rw_prob(raw[i][0], raw[i][2], K, prm['beta'], prm['eps'])
            cpu.append(1e3 * (time.perf_counter() - t0))
        res['scipy_splu_f64_ms_per_slice'] = round(statistics.median(cpu), 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
