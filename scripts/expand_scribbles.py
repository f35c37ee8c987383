#!/usr/bin/env python
"""Offline random-walker expansion of scribbles (pacingpseudo_amd/utils/random_walker.py): the same call the
training driver makes with --rw_scribbles, written to disk -- to train from later without the flag, or to look at the pseudo-labels.
With --method geo it is the geodesic expansion of --geo_scribbles instead (pacingpseudo_amd/utils/geodesic.py).

    python scripts/expand_scribbles.py --file_list train_fold1.txt --data_root ./data/chaos --out ./data/chaos_rw
    python scripts/expand_scribbles.py --synthetic 4 --image_size 32 --out /tmp/rw

Every slice becomes one .npz in --out with the keys of its source (uid / img / lab / scb): `scb` is the expanded map (the ignore
index where the walker is not confident), the original is kept as `scb_orig`, and `rw_maxprob` (float16) is the walker's largest
class probability per pixel (--method geo: `geo_mindist`, the smallest geodesic distance over the classes, in its place).  The
summary line is the driver's.  Needs the MI355X: there is no CPU path."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    from pacingpseudo_amd.utils.geodesic import add_geo_flags
    from pacingpseudo_amd.utils.random_walker import add_rw_flags
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--file_list', type=str, help='text file with one .npz path per line (relative to --data_root)')
    src.add_argument('--synthetic', type=int, default=0, help='N synthetic phantom slices instead of files')
    ap.add_argument('--data_root', type=str, default='', help='prefix of the paths in --file_list')
    ap.add_argument('--image_size', type=int, default=256, help='size of the synthetic phantoms')
    ap.add_argument('--seed', type=int, default=1, help='seed of the synthetic phantoms')
    ap.add_argument('--num_classes', type=int, default=5, help='classes incl. background; the ignore index is this number')
    ap.add_argument('--out', type=str, required=True, help='output directory')
    ap.add_argument('--method', choices=('rw', 'geo'), default='rw', help='random walker (--rw_* flags) or geodesic distance (--geo_* flags)')
    add_rw_flags(ap)                               # --rw_beta ... (--rw_scribbles is implied here)
    add_geo_flags(ap)                              # --geo_lambda ... (--geo_scribbles is implied by --method geo)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    import torch
    from pacingpseudo_amd.data import NpzSlices, SyntheticPhantoms
    from pacingpseudo_amd.utils.random_walker import check_rw_params, expand_dataset, summarize, summary_line
    from pacingpseudo_amd.utils.geodesic import check_geo_params, expand_dataset_geo, summarize_geo, summary_line_geo
    geo = args.method == 'geo'
    try:
        if geo:
            prm = check_geo_params(args.geo_lambda, args.geo_ratio, args.geo_max_dist, args.geo_max_sweeps, K=args.num_classes)
        else:
            prm = check_rw_params(args.rw_beta, args.rw_eps, args.rw_tol, args.rw_max_iters, args.rw_threshold, K=args.num_classes)
    except (ValueError, NotImplementedError) as e:
        ap.error(str(e))
    if args.synthetic:
        ds = SyntheticPhantoms(args.synthetic, args.num_classes, size=args.image_size, seed=args.seed, raw=True)
        names = [f'phantom_{i:04d}.npz' for i in range(args.synthetic)]
    else:
        files = [os.path.join(args.data_root, line.strip()) for line in open(args.file_list) if line.strip()]
        ds = NpzSlices(files, args.num_classes, raw=True)
        names = [os.path.basename(f) for f in files]
        if len(set(names)) != len(names):
            ap.error('--file_list: two slices share a file name; the output directory is flat')
    os.makedirs(args.out, exist_ok=True)
    if geo:
        maps, rep = expand_dataset_geo(ds, args.num_classes, torch.device('cuda'), prm, keep_mindist=True)
    else:
        maps, rep = expand_dataset(ds, args.num_classes, torch.device('cuda'), prm, keep_maxprob=True)
    for i, name in enumerate(names):
        if args.synthetic:
            img, lab, scb = ds.raw_arrays(i)
            keys = dict(uid=name[:-4], img=img, lab=lab)
        else:
            z = np.load(ds.files[i])
            keys, scb = {k: z[k] for k in z.files if k != 'scb'}, z['scb']
        extra = dict(geo_mindist=rep['mindist'][i]) if geo else dict(rw_maxprob=rep['maxprob'][i])
        np.savez(os.path.join(args.out, name), **keys, scb=maps[i].astype(np.asarray(scb).dtype), scb_orig=scb, **extra)
    if geo:
        s = summarize_geo(rep)
        print(summary_line_geo(s))
        if s['unconverged']:
            print(f'warning: {s["unconverged"]} planes stopped at --geo_max_sweeps, first slices: {s["unconverged_slices"][:8]}')
        return s
    s = summarize(rep)
    print(summary_line(s))
    if s['unconverged']:
        print(f'warning: {s["unconverged"]} systems stopped at --rw_max_iters before --rw_tol, first slices: {s["unconverged_slices"][:8]}')
    return s


if __name__ == '__main__':
    main()
