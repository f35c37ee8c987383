#!/usr/bin/env python
"""Cost of the volume-wise evaluation of one patient volume (inference.py --volumes) on the device, beside the same work done with
scipy on the host.  Prints one JSON line.

The volume: --depth x --size x --size cross-sections of K-1 ellipsoids (data.SyntheticVolumes) as the label; the prediction is the
label with 1 % of the voxels re-drawn and --islands planted blobs of 3 x 3 x 3 voxels, the kind of error the 3-D filter removes.

  label_ms / keep_largest_ms / surface_ms / dice_ms   median wall clock of utils.label_components_3d, keep_largest_components_3d,
                                                      volume_surface_metrics (on the filtered map; includes pp_surface_reduce and the
                                                      copy of K x 12 numbers to the host) and volume_dice, each synchronised
  device_total_ms                                     median of the three steps the driver runs per volume in one go
                                                      (filter + Dice + surface metrics)
  scipy_*_ms                                          median of the restatement on the host: ndimage.label per class + bincount,
                                                      binary_erosion + distance_transform_edt per class and direction, numpy.percentile
  *_halves_ms                                         the medians of the even and of the odd samples of device_total_ms: the spread of
                                                      one setting against itself

usage: python scripts/bench_volume.py [--steps 30] [--warmup 5] [--depth 32] [--size 256] [--classes 5] [--host_steps 3]
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


def make_volume(cli):
    import numpy as np
    from pacingpseudo_amd.data import SyntheticVolumes
    K, D, S = cli.classes, cli.depth, cli.size
    ds = SyntheticVolumes(D, K, depth=D, size=S, seed=1)
    label = np.stack([ds.raw_arrays(i)[1] for i in range(D)]).astype(np.int64)
    rng = np.random.default_rng(0)
    pred = label.copy()
    hit = rng.random(pred.shape) < 0.01
    pred[hit] = rng.integers(0, K, int(hit.sum()))
    for i in range(cli.islands):
        z, y, x = rng.integers(0, D - 3), rng.integers(0, S - 3), rng.integers(0, S - 3)
        pred[z:z + 3, y:y + 3, x:x + 3] = 1 + i % (K - 1)
    return pred, label


def wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return 1e3 * (time.perf_counter() - t0)


def host_path(pred, label, K, spacing, connectivity=1):
    """The same numbers with scipy: -> (seconds for labels of all values, keep-largest, surface metrics)."""
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, connectivity)
    cross = ndimage.generate_binary_structure(3, 1)
    t0 = time.perf_counter()
    for v in range(K):
        ndimage.label(pred == v, structure=st)
    t1 = time.perf_counter()
    out = pred.copy()
    for k in range(1, K):
        lab, n = ndimage.label(pred == k, structure=st)
        if n:
            sizes = np.bincount(lab.ravel())[1:]
            out[(lab > 0) & (lab != int(np.argmax(sizes)) + 1)] = 0
    t2 = time.perf_counter()
    res = []
    for k in range(K):
        a, b = out == k, label == k
        if not (a.any() and b.any()) or a.all() or b.all():
            continue
        sa, sb = a ^ ndimage.binary_erosion(a, cross), b ^ ndimage.binary_erosion(b, cross)
        d1 = ndimage.distance_transform_edt(~sb, sampling=spacing)[sa]
        d2 = ndimage.distance_transform_edt(~sa, sampling=spacing)[sb]
        s = np.hstack((d1, d2))
        res.append((s.max(), np.percentile(s, 95), (d1.mean() + d2.mean()) / 2, ((d1 <= 2.0).sum() + (d2 <= 2.0).sum()) / s.size))
    t3 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host_steps', type=int, default=3)
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--islands', type=int, default=12)
    ap.add_argument('--slice_spacing', type=float, default=5.0)
    cli = ap.parse_args()
    import numpy as np
    import torch
    from pacingpseudo_amd.utils import keep_largest_components_3d, label_components_3d, volume_dice, volume_surface_metrics
    assert torch.cuda.is_available(), 'bench_volume.py needs the GPU'
    dev = torch.device('cuda', 0)
    K = cli.classes
    spacing = (cli.slice_spacing, 1.62, 1.62)
    pred_h, label_h = make_volume(cli)
    pred, label = torch.from_numpy(pred_h).to(dev), torch.from_numpy(label_h).to(dev)
    sync = torch.cuda.synchronize
    filtered = keep_largest_components_3d(pred, K)

    def total():
        f = keep_largest_components_3d(pred, K)
        return volume_dice(f, label, K), volume_surface_metrics(f, label, K, spacing)

    steps = {'label_ms': lambda: label_components_3d(pred), 'keep_largest_ms': lambda: keep_largest_components_3d(pred, K),
             'surface_ms': lambda: volume_surface_metrics(filtered, label, K, spacing), 'dice_ms': lambda: volume_dice(filtered, label, K),
             'device_total_ms': total}
    samples = {k: [] for k in steps}
    for _ in range(cli.warmup):
        for fn in steps.values():
            fn()
    for _ in range(cli.steps):                       # the settings alternate, so clock drift hits all alike
        for k, fn in steps.items():
            samples[k].append(wall(fn, sync))
    out = {'volume': [cli.depth, cli.size, cli.size], 'classes': K, 'spacing_mm': list(spacing), 'steps': cli.steps, 'warmup': cli.warmup,
           'voxels_removed_by_the_filter': int((filtered != pred).sum())}
    for k, v in samples.items():
        out[k] = round(statistics.median(v), 4)
    tot = samples['device_total_ms']
    out['device_total_halves_ms'] = [round(statistics.median(tot[0::2]), 4), round(statistics.median(tot[1::2]), 4)]
    host = [host_path(pred_h, label_h, K, spacing) for _ in range(cli.host_steps)]
    for i, k in enumerate(('scipy_label_ms', 'scipy_keep_largest_ms', 'scipy_surface_ms')):
        out[k] = round(statistics.median(h[i] for h in host), 2)
    out['scipy_total_ms'] = round(out['scipy_keep_largest_ms'] + out['scipy_surface_ms'], 2)
    # the two paths computed the same thing
    got = volume_surface_metrics(filtered, label, K, spacing)
    ref = host[0][3]
    scored = [k for k in range(K) if not np.isnan(got['hd'][k])]
    assert len(scored) == len(ref)
    for k, r in zip(scored, ref):
        assert np.allclose([got['hd'][k], got['hdp'][k], got['assd'][k], got['nsd'][k]], r, rtol=1e-5), (k, r)
    out['hd95_mm'] = [round(float(got['hdp'][k]), 3) for k in scored]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
