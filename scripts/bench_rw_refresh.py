#!/usr/bin/env python
"""What one pseudo-label refresh costs beside the epoch it precedes (train_chaos.py --rw_refresh): one
``refresh_dataset`` over ``--synthetic 256`` phantoms of 256 x 256 with the default model and parameters -- the eval-mode forward of
every slice, the random walker with priors, the labels, the copies back -- and one training epoch (plain flags, GPU augmentation,
batch 12) over the same slices, in the same process, each between host clocks with a device synchronisation on both sides.
No threshold is attached to either number.  Prints one JSON line.

usage: python scripts/bench_rw_refresh.py [--synthetic 256] [--size 256] [--batch_size 12] [--gamma 0.1] [--init_ch 32] [--max_ch 512]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--synthetic', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batch_size', type=int, default=12)
    ap.add_argument('--gamma', type=float, default=0.1)
    ap.add_argument('--init_ch', type=int, default=32)
    ap.add_argument('--max_ch', type=int, default=512)
    cli = ap.parse_args()
    import numpy as np
    import torch
    from pacingpseudo_amd.augment import AugConfig, DeviceAugmenter, collate_raw
    from pacingpseudo_amd.data import SyntheticPhantoms, default_args
    from pacingpseudo_amd.models import ConsistencyRegulr
    from pacingpseudo_amd.optim import FusedAdam
    from pacingpseudo_amd.utils import SharedMaps, check_rw_params, refresh_dataset
    from pacingpseudo_amd.utils.random_walker import refresh_forward, summarize
    device = torch.device('cuda', 0)
    K, S, n = 5, cli.size, cli.synthetic
    args = default_args(init_ch=cli.init_ch, max_ch=cli.max_ch, feat_ch=[cli.max_ch, cli.max_ch])
    torch.manual_seed(1)
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=K, output_stride=args.output_stride,
                         is_stride_conv=False, is_trans_conv=False, elab_end_points=True),
        kwargs_aux_path=dict(num_classes=K, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=args.hid_ch, aux_drop_prob=0.0,
                             do_memory=False, max_step=args.epoch, update_momentum=0.9, ensemble_mode='cosine_similarity'),
        args_parser=args).cuda()
    opt = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd)
    ds = SyntheticPhantoms(n, K, size=S, raw=True, seed=1)
    ds.scribble_override = SharedMaps([np.asarray(ds.raw_arrays(i)[2]).astype(np.uint8) for i in range(n)])
    aug = DeviceAugmenter(AugConfig(num_classes=K, crop_size=(S, S)), device=device, seed=1)
    loader = torch.utils.data.DataLoader(ds, batch_size=cli.batch_size, shuffle=True, num_workers=0, drop_last=True, collate_fn=collate_raw)

    def epoch():
        for batch in loader:
            b = aug(batch['img'], batch['lab'], batch['scb'], batch['sizes'])
            b.pop('label', None)
            out = model(b, mode='train', step=0)
            opt.zero_grad()
            out['loss_pce'].backward()
            opt.step()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    prm = dict(check_rw_params(K=K), gamma=cli.gamma)
    refresh = lambda: refresh_dataset(ds, refresh_forward(model, K), K, device, prm, args.output_stride)
    timed(epoch)                                                             # warm-up: plans, kernels, the loader
    timed(refresh)
    _, t_epoch = timed(epoch)
    (maps, rep), t_refresh = timed(refresh)
    s = summarize(rep)
    print(json.dumps(dict(metric='one pseudo-label refresh beside one training epoch over the same slices', slices=n, size=S, classes=K,
                          batch_size=cli.batch_size, gamma=cli.gamma, params={k: v for k, v in prm.items()},
                          refresh_s=round(t_refresh, 3), epoch_s=round(t_epoch, 3), refresh_over_epoch=round(t_refresh / t_epoch, 3),
                          max_iterations=s['max_iterations'], worst_relres=s['worst_relres'], unconverged=s['unconverged'],
                          coverage_after=s['coverage_after'], changed=float(rep['changed'].mean()),
                          device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
