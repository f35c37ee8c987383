#!/usr/bin/env python
"""Cost of the size threshold and the hole filling (inference.py --min_component_size / --fill_holes) on the device, as --depth
slices and as one volume, beside the labelling each consumes, beside keep_largest_components at the same shape from the same run,
and beside the same work done with scipy on the host.  Prints one JSON line.

The maps: --depth x --size x --size cross-sections of K-1 ellipsoids (data.SyntheticVolumes) with 1 % of the voxels re-drawn (specks
of other classes inside the organs), 1 % set to 0 (pin-holes) and --islands planted blobs of 3 x 3 x 3 voxels.

  2d_* / 3d_*            the maps as --depth slices (one call for all) / as one volume
  *_label_ms             utils.label_components / label_components_3d alone: what every function below starts with
  *_remove_small_ms      utils.remove_small_components[_3d] (labelling + pmor_remove_small), *_fill_holes_ms likewise
  *_small_kernels_ms     pmor_remove_small alone on labels made beforehand (a clear, two launches), *_fill_kernels_ms likewise
  *_keep_largest_ms      utils.keep_largest_components[_3d], the yardstick
  *_chain_ms             threshold -> keep-largest -> fill in one go, as the driver runs them
  scipy_*_ms             the restatement on the host: ndimage.label per class + bincount; ndimage.label of the background, one
                         binary_dilation per class for the contacts; the chain with ndimage.label + argmax for keep-largest
All device figures are medians of synchronised wall-clock samples; the settings alternate, so clock drift hits all alike.

usage: python scripts/bench_morph.py [--steps 30] [--warmup 5] [--depth 32] [--size 256] [--classes 5] [--host_steps 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_maps(cli):
    import numpy as np
    from pacingpseudo_amd.data import SyntheticVolumes
    K, D, S = cli.classes, cli.depth, cli.size
    ds = SyntheticVolumes(D, K, depth=D, size=S, seed=1)
    label = np.stack([ds.raw_arrays(i)[1] for i in range(D)]).astype(np.int64)
    rng = np.random.default_rng(0)
    pred = label.copy()
    hit = rng.random(pred.shape) < 0.01
    pred[hit] = rng.integers(1, K, int(hit.sum()))
    pred[rng.random(pred.shape) < 0.01] = 0
    for i in range(cli.islands):
        z, y, x = rng.integers(0, D - 3), rng.integers(0, S - 3), rng.integers(0, S - 3)
        pred[z:z + 3, y:y + 3, x:x + 3] = 1 + i % (K - 1)
    return pred


def wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return 1e3 * (time.perf_counter() - t0)


def host_remove_small(cm, K, min_size, connectivity):
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(cm.ndim, connectivity)
    out = cm.copy()
    for k in range(1, K):
        lab, n = ndimage.label(cm == k, structure=st)
        if n:
            small = np.bincount(lab.ravel(), minlength=n + 1) < min_size
            small[0] = False
            out[small[lab]] = 0
    return out


def host_keep_largest(cm, K, connectivity):
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(cm.ndim, connectivity)
    out = cm.copy()
    for k in range(1, K):
        lab, n = ndimage.label(cm == k, structure=st)
        if n:
            out[(lab > 0) & (lab != int(np.argmax(np.bincount(lab.ravel())[1:])) + 1)] = 0
    return out


def host_fill_holes(cm, K, connectivity):
    """The definition with whole-array scipy calls: per background component one bit per contact class, bit 0 for the border."""
    import numpy as np
    from scipy import ndimage
    st = ndimage.generate_binary_structure(cm.ndim, connectivity)
    zero = cm == 0
    lab, n = ndimage.label(zero, structure=st)
    bits = np.zeros(n + 1, np.int64)
    border = np.zeros(cm.shape, bool)
    for ax in range(cm.ndim):
        idx = [slice(None)] * cm.ndim
        for edge in (0, cm.shape[ax] - 1):
            idx[ax] = edge
            border[tuple(idx)] = True
    bits[np.unique(lab[border])] |= 1
    for k in range(1, K):
        bits[np.unique(lab[ndimage.binary_dilation(cm == k, structure=st) & zero])] |= 1 << k
    bits[np.unique(lab[ndimage.binary_dilation((cm < 0) | (cm >= K), structure=st) & zero])] |= 1
    bits[0] = 1
    single = (bits > 1) & ((bits & (bits - 1)) == 0)
    fill = np.where(single, np.log2(np.maximum(bits, 1)).astype(np.int64), 0)
    return np.where(zero, fill[lab], cm)


def host_path(pred, K, min_size, per_slice):
    """-> (ms threshold, ms fill, ms chain, the three results)."""
    import numpy as np
    items = list(pred) if per_slice else [pred]
    join = np.stack if per_slice else (lambda r: r[0])
    t0 = time.perf_counter()
    small = join([host_remove_small(a, K, min_size, 1) for a in items])
    t1 = time.perf_counter()
    filled = join([host_fill_holes(a, K, 1) for a in items])
    t2 = time.perf_counter()
    chain = join([host_fill_holes(host_keep_largest(host_remove_small(a, K, min_size, 1), K, 1), K, 1) for a in items])
    t3 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), (small, filled, chain)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host_steps', type=int, default=2)
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--islands', type=int, default=12)
    ap.add_argument('--min_size_2d', type=int, default=20)
    ap.add_argument('--min_size_3d', type=int, default=50)
    cli = ap.parse_args()
    import numpy as np
    import torch
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._morph import morph
    from pacingpseudo_amd.utils import (fill_holes, fill_holes_3d, keep_largest_components, keep_largest_components_3d, label_components,
                                        label_components_3d, remove_small_components, remove_small_components_3d)
    assert torch.cuda.is_available(), 'bench_morph.py needs the GPU'
    dev = torch.device('cuda', 0)
    K, D, S = cli.classes, cli.depth, cli.size
    pred_h = make_maps(cli)
    pred = torch.from_numpy(pred_h).to(dev)
    sync = torch.cuda.synchronize
    m2, m3 = cli.min_size_2d, cli.min_size_3d

    # the two library calls alone, on labels and buffers made beforehand
    lab2, lab3 = label_components(pred, 1), label_components_3d(pred, 1)
    out = torch.empty_like(pred)
    stats = torch.empty((D, K, 2), device=dev, dtype=torch.int32)
    nws = morph.pmor_workspace(D, K, 1, S, S, 2)
    assert nws == morph.pmor_workspace(1, K, D, S, S, 3)
    ws = torch.empty(nws // 8, device=dev, dtype=torch.float64)
    thr2, thr3 = (ctypes.c_int32 * K)(*[m2] * K), (ctypes.c_int32 * K)(*[m3] * K)

    def raw(kind, dims):
        N, Dz, lab = (D, 1, lab2) if dims == 2 else (1, D, lab3)
        if kind == 'small':
            morph.pmor_remove_small(pred.data_ptr(), lab.data_ptr(), N, K, Dz, S, S, dims, thr2 if dims == 2 else thr3, out.data_ptr(),
                                    stats.data_ptr(), ws.data_ptr(), nws, stream_ptr())
        else:
            morph.pmor_fill_holes(pred.data_ptr(), lab.data_ptr(), N, K, Dz, S, S, dims, 1, out.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                  nws, stream_ptr())

    steps = {
        '2d_label_ms': lambda: label_components(pred, 1),
        '2d_remove_small_ms': lambda: remove_small_components(pred, K, m2),
        '2d_fill_holes_ms': lambda: fill_holes(pred, K),
        '2d_small_kernels_ms': lambda: raw('small', 2),
        '2d_fill_kernels_ms': lambda: raw('fill', 2),
        '2d_keep_largest_ms': lambda: keep_largest_components(pred, K),
        '2d_chain_ms': lambda: fill_holes(keep_largest_components(remove_small_components(pred, K, m2), K), K),
        '3d_label_ms': lambda: label_components_3d(pred, 1),
        '3d_remove_small_ms': lambda: remove_small_components_3d(pred, K, m3),
        '3d_fill_holes_ms': lambda: fill_holes_3d(pred, K),
        '3d_small_kernels_ms': lambda: raw('small', 3),
        '3d_fill_kernels_ms': lambda: raw('fill', 3),
        '3d_keep_largest_ms': lambda: keep_largest_components_3d(pred, K),
        '3d_chain_ms': lambda: fill_holes_3d(keep_largest_components_3d(remove_small_components_3d(pred, K, m3), K), K),
    }
    samples = {k: [] for k in steps}
    for _ in range(cli.warmup):
        for fn in steps.values():
            fn()
    for _ in range(cli.steps):
        for k, fn in steps.items():
            samples[k].append(wall(fn, sync))
    res = {'maps': [D, S, S], 'classes': K, 'min_size': [m2, m3], 'steps': cli.steps, 'warmup': cli.warmup}
    for k, v in samples.items():
        res[k] = round(statistics.median(v), 4)
    for dims in ('2d', '3d'):
        tot = samples[dims + '_chain_ms']
        res[dims + '_chain_halves_ms'] = [round(statistics.median(tot[0::2]), 4), round(statistics.median(tot[1::2]), 4)]

    # the host, and that both paths computed the same thing
    for dims, per_slice, small_fn, fill_fn, chain_fn in (
            ('2d', True, lambda: remove_small_components(pred, K, m2, return_stats=True), lambda: fill_holes(pred, K, return_stats=True),
             steps['2d_chain_ms']),
            ('3d', False, lambda: remove_small_components_3d(pred, K, m3, return_stats=True), lambda: fill_holes_3d(pred, K, return_stats=True),
             steps['3d_chain_ms'])):
        host = [host_path(pred_h, K, m2 if per_slice else m3, per_slice) for _ in range(cli.host_steps)]
        for i, name in enumerate(('remove_small', 'fill_holes', 'chain')):
            res[f'scipy_{dims}_{name}_ms'] = round(statistics.median(h[i] for h in host), 2)
        small_h, filled_h, chain_h = host[0][3]
        small_d, small_stats = small_fn()
        filled_d, fill_stats = fill_fn()
        assert np.array_equal(small_d.cpu().numpy(), small_h) and np.array_equal(filled_d.cpu().numpy(), filled_h)
        assert np.array_equal(chain_fn().cpu().numpy(), chain_h)
        res[f'{dims}_voxels_removed'] = int(small_stats[..., 1].sum())
        res[f'{dims}_voxels_filled'] = int(fill_stats[..., 1:, 1].sum())
        res[f'{dims}_cavities_mixed'] = int(fill_stats[..., 0, 0].sum())
        assert res[f'{dims}_voxels_removed'] == int((small_h != pred_h).sum()) and res[f'{dims}_voxels_filled'] == int((filled_h != pred_h).sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
