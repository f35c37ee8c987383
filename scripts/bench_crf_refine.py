#!/usr/bin/env python
"""Cost of the mean-field CRF refinement (inference.py --crf_refine) at the benchmark shape, in one process.  Prints one JSON line.

Batch 32, 256x256, K = 5 classes, C = 1 image channel, radius 5, dilation 1, T = 5 iterations (all settable).  Reported, each the
median over --steps samples of --reps calls between two events:
  refine_ms            one pp_crf_refine call with T iterations (T launches), and refine_1_ms with one iteration (the launch that
                       forms the soft-max while staging); per_iteration_ms = refine_ms / T
  loss_fwd_ms          pp_crf_loss_fwd at the same shape, window and sigmas without the gradient pass (crf_fwd_kernel + its
                       reduction launch): the kernel that walks the same window over the same tile -- the yardstick of one iteration;
                       loss_fwd_unit_ms with the `unit` output the training step asks for
  iteration_over_loss  per_iteration_ms / loss_fwd_ms
  unet_forward_ms      one forward pass of the default U-Net on the same batch (eval mode, random weights)
  wrapper_ms           utils.crf_refine (allocations and enqueue included)
The inputs are low-resolution noise up-sampled (regions with ragged borders) and a piecewise-smooth image, as in the tests.

usage: python scripts/bench_crf_refine.py [--steps 20] [--warmup 3] [--batch 32] [--size 256] [--classes 5] [--channels 1]
                                          [--radius 5] [--dilation 1] [--iterations 5] [--reps 5] [--skip_unet]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, steps, warmup):
    """Median milliseconds of one call of fn: `steps` samples of `reps` calls between two events."""
    import torch
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        evs.append(ev)
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) / reps


def smooth(shape, seed, scale, noise, device):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    coarse = torch.randn(N, C, max(H // 8, 2), max(W // 8, 2), generator=g)
    out = F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True) * scale + noise * torch.randn(shape, generator=g)
    return out.contiguous().to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed samples per setting')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--channels', type=int, default=1)
    ap.add_argument('--radius', type=int, default=5)
    ap.add_argument('--dilation', type=int, default=1)
    ap.add_argument('--iterations', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5, help='calls per sample')
    ap.add_argument('--skip_unet', action='store_true', help='leave the U-Net forward pass out')
    cli = ap.parse_args()
    import torch
    from pacingpseudo_amd._lib import lib, stream_ptr
    from pacingpseudo_amd.utils import crf_refine
    from pacingpseudo_amd.utils.crf_refine import check_crf_refine_params
    device = torch.device('cuda', 0)
    N, K, C, H, W, T, r, d = cli.batch, cli.classes, cli.channels, cli.size, cli.size, cli.iterations, cli.radius, cli.dilation
    prm = check_crf_refine_params(T, r, d, K=K, C=C)
    z = smooth((N, K, H, W), 0, 3.0, 0.5, device)
    x = smooth((N, C, H, W), 1, 0.15, 0.0, device)
    prob = torch.empty_like(z)
    cls = torch.empty((N, H, W), device=device, dtype=torch.int64)
    nws = lib.pp_crf_refine_workspace(N, K, H, W)
    ws = torch.empty(nws, device=device, dtype=torch.uint8)

    def refine(iters):
        lib.pp_crf_refine(z.data_ptr(), x.data_ptr(), N, K, C, H, W, iters, r, d, prm['sigma_xy'], prm['sigma_rgb'], prm['sigma_smooth'],
                          prm['w_bilateral'], prm['w_smooth'], prob.data_ptr(), cls.data_ptr(), ws.data_ptr(), nws, stream_ptr())
    sums = torch.zeros(2, device=device, dtype=torch.float64)
    unit = torch.empty_like(z)
    nlw = lib.pp_crf_loss_workspace(N, H, W)
    lws = torch.empty(nlw, device=device, dtype=torch.uint8)

    def loss(with_unit):
        lib.pp_crf_loss_fwd(z.data_ptr(), x.data_ptr(), None, N, K, C, H, W, r, d, prm['sigma_xy'], prm['sigma_rgb'],
                            unit.data_ptr() if with_unit else None, sums.data_ptr(), lws.data_ptr(), nlw, stream_ptr())
    res = dict(metric='mean-field CRF refinement: ms per batch, one iteration against pp_crf_loss_fwd and a U-Net forward pass',
               batch=N, size=H, classes=K, channels=C, radius=r, dilation=d, iterations=T, steps=cli.steps, warmup=cli.warmup, reps=cli.reps)
    t_all = timed(lambda: refine(T), cli.reps, cli.steps, cli.warmup)
    t_one = timed(lambda: refine(1), cli.reps, cli.steps, cli.warmup)
    t_loss = timed(lambda: loss(False), cli.reps, cli.steps, cli.warmup)
    t_unit = timed(lambda: loss(True), cli.reps, cli.steps, cli.warmup)
    t_wrap = timed(lambda: crf_refine(z, x, **prm), cli.reps, cli.steps, cli.warmup)
    torch.cuda.synchronize()
    before = z.argmax(1)
    refine(T)
    res.update(refine_ms=round(t_all, 4), refine_1_ms=round(t_one, 4), per_iteration_ms=round(t_all / T, 4), loss_fwd_ms=round(t_loss, 4),
               loss_fwd_unit_ms=round(t_unit, 4), iteration_over_loss=round(t_all / T / t_loss, 3), first_iteration_over_loss=round(t_one / t_loss, 3),
               wrapper_ms=round(t_wrap, 4), classes_changed=round(float((cls != before).float().mean()), 4))
    if not cli.skip_unet:
        from pacingpseudo_amd.models import UNet
        torch.manual_seed(1)
        net = UNet(input_ch=C, init_ch=32, max_ch=512, num_classes=K, output_stride=8).to(device)
        net.eval()

        def forward():
            with torch.no_grad():
                net(x)['segmentation/logits']
        t_net = timed(forward, cli.reps, cli.steps, cli.warmup)
        res.update(unet_forward_ms=round(t_net, 4), refine_over_unet_forward=round(t_all / t_net, 3))
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
