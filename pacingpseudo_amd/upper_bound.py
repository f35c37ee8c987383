"""Fully-supervised upper bound: the reference's ``upper_bound_chaos.py`` (bare UNet trained with cross entropy on the
FULL label + soft Dice loss, upper_bound_chaos.py:110-244) on the MI355X path.

Kept from the reference: flag names / types / defaults (upper_bound_chaos.py:23-108), the run-directory layout
``{root}/{modality}/{session}/{session}-{time}-fold{k}-{tag}/`` with ``ckps/``, ``log.txt``, ``valdice.npz``, the log
lines (:173-174, :213-218, :241-243), per-epoch poly LR, ``model.eval()`` after the first epoch and never back (:180),
``ckp_{epoch}.pth`` / ``best_ckp.pth`` holding the bare UNet's ``state_dict()``.
The step runs through ``UNet.forward`` (one autograd node over the engine's static plan) and the HIP loss kernels
``partial_cross_entropy_loss`` / ``dice_loss_fn``; the training set goes through the reference's WEAK augmentation list
(upper_bound_chaos.py:132-137) on the GPU (``augment.DeviceAugmenter(do_strong=False)``; ``--cpu_input`` selects the minimal CPU
path); validation at the native slice size with device-side meters; widened ``choices`` and the --synthetic / --image_size /
--max_iters additions are those of ``pacingpseudo_amd.train``.  ``--do_loss_boundary`` (not in the reference) adds the boundary loss
of Kervadec et al. on signed distance maps recomputed per step from the augmented label (``losses.boundary_loss``);
``--do_loss_lovasz`` (not in the reference either) adds the Lovasz-softmax loss of Berman et al. (``losses.lovasz_softmax_loss``).
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import shutil
import sys
import time

import numpy as np
import torch

from . import finetune, resume
from .optim import WD_HELP, add_clip_flag, add_ema_flags, add_wd_exempt_flag, check_optimizer_flags, log_clip_stats

parser = argparse.ArgumentParser()
parser.add_argument('--gpu', type=str, default='1')
parser.add_argument('--seed', type=int, default=1)
parser.add_argument('--dataset', type=str, default='chaos')
parser.add_argument('--root', type=str, default='./outputs/chaos')
parser.add_argument('--session', type=str, default='Upperbound')
parser.add_argument('--tag', type=str, required=True)
parser.add_argument('--fold', type=int, default=1, choices=[0, 1, 2, 3, 4])
parser.add_argument('--modality', type=str, default='t1', choices=['t1', 't2'])
parser.add_argument('--num_classes', type=int, default=None, help='default: the --dataset preset (5 for chaos)')
parser.add_argument('--num_workers', type=int, default=4)
parser.add_argument('--augmentation_configs', type=str, default='datasets.chaos.chaos_aug_configs')
parser.add_argument('--augmentations', type=str, default='TransformsColor', choices=['TransformsColor'])
parser.add_argument('--input_ch', type=int, default=1)
parser.add_argument('--init_ch', type=int, default=32)
parser.add_argument('--max_ch', type=int, default=512)
parser.add_argument('--output_stride', type=int, default=8, choices=[32, 16, 8])
parser.add_argument('--is_stride_conv', type=bool, default=False)
parser.add_argument('--is_trans_conv', type=bool, default=False)
parser.add_argument('--elab_end_points', type=bool, default=True)
parser.add_argument('--loss_dice', action='store_true', default=True)
parser.add_argument('--ignored_index', type=int, default=None, help='default: the --dataset preset (5 for chaos)')
parser.add_argument('--epoch', type=int, default=400)
parser.add_argument('--batch_size', type=int, default=12)
parser.add_argument('--optimizer', type=str, default='adam', choices=['adam', 'adamw'],
                    help='FusedAdam or FusedAdamW (one kernel over the flat parameter slab); adamw decouples --wd from the gradient')
parser.add_argument('--momentum', type=float, default=0.9)
parser.add_argument('--lr', type=float, default=0.0001)
parser.add_argument('--lr_decay', type=str, default='poly', choices=['linear', 'poly', 'cosine'])
parser.add_argument('--wd', type=float, default=0.0003, help=WD_HELP)
parser.add_argument('--ckp_interval', type=int, default=10000)
# ---- additions of this implementation (same meaning as in pacingpseudo_amd.train)
parser.add_argument('--synthetic', type=int, default=0)
parser.add_argument('--image_size', type=int, default=None, help='training crop size (default: the --dataset preset); validation runs at the native size')
parser.add_argument('--max_iters', type=int, default=0)
parser.add_argument('--cpu_input', action='store_true',
                    help='minimal CPU input path of data.py (MeanStdNorm + centre crop only) instead of the weak augmentation '
                         'pipeline on the GPU')
parser.add_argument('--norm_op', type=str, default='batch', choices=['batch', 'group'],
                    help='block normaliser of the U-Net: batch = nn.BatchNorm2d (the reference); group = nn.GroupNorm(--norm_groups, C): '
                         'per-image statistics, no running state, the same function in train and eval mode (fp32 storage only)')
parser.add_argument('--norm_groups', type=int, default=8, help='channel groups of --norm_op group; must divide every block width')
parser.add_argument('--gpu_augment', action='store_true', help='accepted for compatibility: the GPU pipeline is the default')
add_clip_flag(parser)                         # --clip_grad_norm X (pacingpseudo_amd/optim.py)
add_ema_flags(parser)                         # --ema_decay D / --ema_val_interval N (pacingpseudo_amd/optim.py)
add_wd_exempt_flag(parser)                    # --wd_exempt_1d, with --optimizer adamw (pacingpseudo_amd/optim.py)
resume.add_flags(parser)                      # --state_interval N / --resume PATH (pacingpseudo_amd/resume.py)
finetune.add_flags(parser)                    # --freeze_encoder N / --init_from PATH / --init_reset_head (pacingpseudo_amd/finetune.py)
# ---- boundary loss (Kervadec et al., MIDL 2019): mean of soft-max x the signed distance map of the label, recomputed per step on the
# device from the augmented label (libpacingpseudo_dist.so); the reference has no such term.  Off: the step is the reference's.
parser.add_argument('--do_loss_boundary', action='store_true', default=False,
                    help='add loss_boundary_weight * boundary_loss(logits, label) (pixel units) to cross entropy + Dice')
parser.add_argument('--loss_boundary_weight', type=float, default=0.01,
                    help="weight of the boundary loss; 0.01 is Kervadec's initial alpha, here an untuned first value")
parser.add_argument('--ramp_up_loss_boundary', type=int, default=0,
                    help='0: constant weight; E > 0: the weight of epoch e is gaussian_ramp_up(e, loss_boundary_weight, max_t=E)')
# ---- Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018): the convex extension of the per-class Jaccard loss on the sorted pixel
# errors, sorted and scanned on the device (libpacingpseudo_lov.so); the reference has no such term.  Off: the step is the reference's.
parser.add_argument('--do_loss_lovasz', action='store_true', default=False,
                    help='add loss_lovasz_weight * lovasz_softmax_loss(logits, label, ignore_index=ignored_index) to cross entropy + Dice')
parser.add_argument('--loss_lovasz_weight', type=float, default=1.0,
                    help='weight of the Lovasz-softmax loss; 1.0 is an untuned first value')
parser.add_argument('--ramp_up_loss_lovasz', type=int, default=0,
                    help='0: constant weight; E > 0: the weight of epoch e is gaussian_ramp_up(e, loss_lovasz_weight, max_t=E)')
parser.add_argument('--lovasz_per_image', action='store_true', default=False,
                    help='the Lovasz-softmax loss per image, averaged over the batch, instead of over the whole batch at once')


def train_interface(args, resume_state=None):
    from .augment import AugConfig, DeviceAugmenter, collate_raw
    from .data import SyntheticPhantoms, collate_by_shape, dataset_class, expand_compact, loader_context
    from .losses.losses import boundary_loss, dice_loss_fn, lovasz_softmax_loss, partial_cross_entropy_loss
    from .models import UNet
    from .models.unet import norm_kwargs
    from .optim import FusedAdam, FusedAdamW
    from .train import _class_names
    from .utils import cosine_lr_decay, gaussian_ramp_up, linear_lr_decay, poly_lr_decay
    from .utils.metrics import ValAccumulator
    from .utils.scalars import ScalarLog

    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    best_avg, best_epoch, best_avg_class = 0, 0, []
    model = UNet(input_ch=args.input_ch, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=args.num_classes,
                 output_stride=args.output_stride, is_stride_conv=args.is_stride_conv, is_trans_conv=args.is_trans_conv,
                 elab_end_points=args.elab_end_points, **norm_kwargs(args)).cuda()
    finetune.init_model(args, model, parser, logging.info)      # --init_from / --freeze_encoder: before the optimizer exists
    logging.info(model)
    if args.optimizer == 'adamw':
        optimizer = FusedAdamW(model.parameters(), lr=args.lr, weight_decay=args.wd, exempt_1d=args.wd_exempt_1d,
                               max_grad_norm=args.clip_grad_norm or None, ema_decay=args.ema_decay or None)
    else:
        optimizer = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd, max_grad_norm=args.clip_grad_norm or None,
                              ema_decay=args.ema_decay or None)
    ds_kw = dict(num_classes=args.num_classes, size=args.image_size, seed=args.seed)
    # the reference trains the upper bound with the whole WEAK pipeline (upper_bound_chaos.py:132-137: base_transforms =
    # Scaling, Elastic, Rotation, Mirroring, GaussianNoise, RandomCrop; no strong view): the same device pipeline as
    # train_chaos.py with do_strong=False, fed by raw slices
    gpu_aug = not args.cpu_input
    augmenter = DeviceAugmenter(AugConfig(num_classes=args.num_classes, crop_size=(args.image_size, args.image_size),
                                          do_strong=False), device=device, seed=args.seed) if gpu_aug else None
    if args.synthetic:
        train_dataset = SyntheticPhantoms(args.synthetic, do_strong=False, train=True, raw=gpu_aug, **ds_kw)
        val_dataset = SyntheticPhantoms(max(args.synthetic // 4, 1), train=False, native=True, compact=True, **ds_kw)
    else:
        train_dataset = dataset_class(args.dataset)(args.train_ls, do_strong=False, train=True, raw=gpu_aug, **ds_kw)
        val_dataset = dataset_class(args.dataset)(args.val_ls, train=False, native=True, compact=True, **ds_kw)
    train_loader = torch.utils.data.DataLoader(train_dataset, batch_size=args.batch_size, shuffle=True,
                                               num_workers=args.num_workers, drop_last=True,
                                               collate_fn=collate_raw if gpu_aug else None,
                                               persistent_workers=bool(gpu_aug and args.num_workers > 0), pin_memory=gpu_aug,
                                               multiprocessing_context=loader_context(args.num_workers))
    val_loader = torch.utils.data.DataLoader(val_dataset, batch_size=args.batch_size, shuffle=False,
                                             num_workers=args.num_workers, drop_last=False, collate_fn=collate_by_shape,
                                             persistent_workers=args.num_workers > 0, pin_memory=True,
                                             multiprocessing_context=loader_context(args.num_workers))
    names = _class_names(args.num_classes, args.dataset)
    scalars = ScalarLog(os.path.join(args.child, 'tb_summary', 'scalars.jsonl'))
    decay = {'poly': poly_lr_decay, 'cosine': cosine_lr_decay, 'linear': linear_lr_decay}
    if args.lr_decay not in decay:
        raise ValueError('Unimplemented learning rate decay policy.')
    valdice = np.zeros(args.epoch)
    ema_on = bool(args.ema_decay)                  # --ema_decay: see pacingpseudo_amd/train.py
    bl_on = bool(args.do_loss_boundary)            # --do_loss_boundary: off = the parent's step, log lines and scalar tags
    lv_on = bool(args.do_loss_lovasz)              # --do_loss_lovasz: likewise; its fields and tags come after the boundary ones
    valdice_ema = np.zeros(args.epoch) if ema_on else None
    best_ema = dict(avg=0, epoch=0, avg_class=[])
    aug_stream = torch.cuda.Stream() if (augmenter is not None and os.environ.get('PP_AUG_STREAM', '1') != '0') else None
    start_epoch = 0
    if resume_state is not None:
        best_avg, best_epoch, best_avg_class = resume.restore(resume_state, model, optimizer, valdice)
        if ema_on:
            best_ema = resume.restore_ema(resume_state, valdice_ema)
        resume.prime_persistent_loaders([train_loader, val_loader])      # see pacingpseudo_amd/train.py
        resume.set_rng_states(resume_state['rng'][0], device, augmenter)
        start_epoch = resume_state['epoch'] + 1

    def validate():
        """One pass over the validation slices with the weights the model holds: (per-class Dice, loss_ce, loss_dice,
        loss_boundary -- None without --do_loss_boundary, loss_lovasz -- None without --do_loss_lovasz)."""
        meters = ValAccumulator(args.num_classes, device)              # Dice meters + n-weighted loss_ce, on the device
        dsum = torch.zeros(1, device=device, dtype=torch.float64)       # n-weighted loss_dice
        bsum = torch.zeros(1, device=device, dtype=torch.float64)       # n-weighted loss_boundary
        lsum = torch.zeros(1, device=device, dtype=torch.float64)       # n-weighted loss_lovasz
        for groups in val_loader:
            for batch in groups:
                batch = expand_compact(batch, args.num_classes, device)      # uint8 class maps -> one-hot planes, on the device
                image, label = batch['image'], batch['label']
                with torch.no_grad():
                    logits = model(image)['segmentation/logits']
                    target = torch.argmax(label, dim=1).long()
                    meters.update(logits, label, partial_cross_entropy_loss(logits, target, args.ignored_index))
                    dsum += dice_loss_fn(logits, label).double() * image.shape[0]
                    if bl_on:
                        bsum += boundary_loss(logits, target).double() * image.shape[0]
                    if lv_on:
                        lsum += lovasz_softmax_loss(logits, target, ignore_index=args.ignored_index,
                                                    per_image=args.lovasz_per_image).double() * image.shape[0]
        dsc, val_ce, n_val = meters.result()                            # the host sync of the validation epoch
        return (dsc, val_ce, float(dsum) / max(n_val, 1), (float(bsum) / max(n_val, 1) if bl_on else None),
                (float(lsum) / max(n_val, 1) if lv_on else None))

    for curr_epoch in range(start_epoch, args.epoch):
        epoch_tic = time.time()
        optimizer, new_lr = decay[args.lr_decay](optimizer, curr_epoch, args.epoch, args.lr)
        # sum ce*n, sum dice*n, n (read once per epoch); with --do_loss_boundary also sum boundary*n, with --do_loss_lovasz sum lovasz*n
        acc = torch.zeros(5 if lv_on else (4 if bl_on else 3), device=device, dtype=torch.float64)
        bl_weight = lv_weight = 0.0
        if lv_on:
            lv_weight = (gaussian_ramp_up(curr_epoch, args.loss_lovasz_weight, max_t=args.ramp_up_loss_lovasz)
                         if args.ramp_up_loss_lovasz > 0 else args.loss_lovasz_weight)
        if bl_on:
            bl_weight = (gaussian_ramp_up(curr_epoch, args.loss_boundary_weight, max_t=args.ramp_up_loss_boundary)
                         if args.ramp_up_loss_boundary > 0 else args.loss_boundary_weight)
        for idx, batch in enumerate(train_loader):
            if args.max_iters and idx >= args.max_iters:
                break
            if augmenter is not None:
                batch = augmenter.ahead(aug_stream, batch['img'], batch['lab'], batch['scb'], batch['sizes'])   # beside the previous step (train.py)
            image, label = batch['image'].to(device, non_blocking=True), batch['label'].to(device, non_blocking=True)
            n = image.shape[0]
            logits = model(image)['segmentation/logits']
            target = torch.argmax(label, dim=1).long()
            loss_ce = partial_cross_entropy_loss(logits, target, args.ignored_index)
            loss = loss_ce
            acc[0] += loss_ce.detach() * n
            if args.loss_dice:
                loss_dice = dice_loss_fn(logits, label)
                loss = loss + loss_dice
                acc[1] += loss_dice.detach() * n
            if bl_on:
                loss_bl = boundary_loss(logits, target)
                loss = loss + bl_weight * loss_bl
                acc[3] += loss_bl.detach() * n
            if lv_on:
                loss_lv = lovasz_softmax_loss(logits, target, ignore_index=args.ignored_index, per_image=args.lovasz_per_image)
                loss = loss + lv_weight * loss_lv
                acc[4] += loss_lv.detach() * n
            acc[2] += n
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        a = acc.cpu().numpy()
        cnt = max(a[2], 1)
        logging.info("epoch: {:03d}, lr: {:.6f}, loss_ce: {:.6f}, loss_dice: {:.6f}, {}{}{:.2f} s/epoch".format(
            curr_epoch, new_lr, a[0] / cnt, a[1] / cnt, "loss_boundary: {:.6f}, ".format(a[3] / cnt) if bl_on else "",
            "loss_lovasz: {:.6f}, ".format(a[4] / cnt) if lv_on else "", time.time() - epoch_tic))
        log_clip_stats(optimizer, curr_epoch, scalars, logging.info)      # --clip_grad_norm: behind the sync above

        model.eval()                                   # upper_bound_chaos.py:180, never undone
        tic = time.time()
        dsc, val_ce, val_dice, val_bl, val_lv = validate()
        avg_all = np.mean([dsc[_] for _ in range(1, args.num_classes)])
        logging.info("val: {:03d}, loss_ce: {:.6f}, loss_dice: {:.6f}, {}{}{:.2f} s/epoch".format(
            curr_epoch, val_ce, val_dice, "loss_boundary: {:.6f}, ".format(val_bl) if bl_on else "",
            "loss_lovasz: {:.6f}, ".format(val_lv) if lv_on else "", time.time() - tic))
        logging.info("[" + ", ".join("{}: {:.4f}".format(nm, dsc[i]) for i, nm in enumerate(names))
                     + ", All: {:.4f}]".format(avg_all))
        # scalar tags of upper_bound_chaos.py:176-178, :216-224
        scalars.add('losses/loss_ce_train', a[0] / cnt, curr_epoch)
        scalars.add('losses/loss_dice_train', a[1] / cnt, curr_epoch)
        scalars.add('lr/current_lr', new_lr, curr_epoch)
        scalars.add('losses/loss_ce_val', val_ce, curr_epoch)
        scalars.add('losses/loss_dice_val', val_dice, curr_epoch)
        if bl_on:
            scalars.add('losses/loss_boundary_train', a[3] / cnt, curr_epoch)
            scalars.add('losses/loss_boundary_val', val_bl, curr_epoch)
            scalars.add('losses/boundary_weight', bl_weight, curr_epoch)
        if lv_on:
            scalars.add('losses/loss_lovasz_train', a[4] / cnt, curr_epoch)
            scalars.add('losses/loss_lovasz_val', val_lv, curr_epoch)
            scalars.add('losses/lovasz_weight', lv_weight, curr_epoch)
        for i, nm in enumerate(names):
            scalars.add(f'DSC/{nm}', dsc[i], curr_epoch)
        scalars.add('DSC/All', avg_all, curr_epoch)
        scalars.add('DSC/Best', max(best_avg, avg_all), curr_epoch)
        valdice[curr_epoch] = avg_all
        if curr_epoch + 1 == args.epoch or (curr_epoch + 1) % args.ckp_interval == 0:
            torch.save(model.state_dict(), os.path.join(args.child, 'ckps', 'ckp_{:d}.pth'.format(curr_epoch)))
        if avg_all > best_avg:
            best_epoch, best_avg = curr_epoch, avg_all
            best_avg_class = [dsc[_] for _ in range(1, args.num_classes)]
            torch.save(model.state_dict(), args.child + '/best_ckp.pth')
        # --ema_decay: the validation again on the averaged weights, and the EMA checkpoints (pacingpseudo_amd/train.py)
        last = curr_epoch + 1 == args.epoch
        ema_val = ema_on and (last or (curr_epoch + 1) % args.ema_val_interval == 0)
        ema_ckp = ema_on and (last or (curr_epoch + 1) % args.ckp_interval == 0)
        if ema_val or ema_ckp:
            with optimizer.ema_weights():
                if ema_val:
                    tic = time.time()
                    dsc_e, ce_e, dice_e = validate()[:3]
                    avg_e = np.mean([dsc_e[_] for _ in range(1, args.num_classes)])
                    valdice_ema[curr_epoch] = avg_e
                    logging.info("val_ema: {:03d}, loss_ce: {:.6f}, loss_dice: {:.6f}, {:.2f} s/epoch".format(
                        curr_epoch, ce_e, dice_e, time.time() - tic))
                    logging.info("[" + ", ".join("{}: {:.4f}".format(nm, dsc_e[i]) for i, nm in enumerate(names))
                                 + ", All: {:.4f}] (EMA)".format(avg_e))
                    for i, nm in enumerate(names):
                        scalars.add(f'DSC_EMA/{nm}', dsc_e[i], curr_epoch)
                    scalars.add('DSC_EMA/All', avg_e, curr_epoch)
                    scalars.add('DSC_EMA/Best', max(best_ema['avg'], avg_e), curr_epoch)
                    if avg_e > best_ema['avg']:
                        best_ema = dict(avg=avg_e, epoch=curr_epoch, avg_class=[dsc_e[_] for _ in range(1, args.num_classes)])
                        torch.save(model.state_dict(), args.child + '/best_ema_ckp.pth')
                if ema_ckp:
                    torch.save(model.state_dict(), os.path.join(args.child, 'ckps', 'ema_ckp_{:d}.pth'.format(curr_epoch)))
        if args.state_interval and ((curr_epoch + 1) % args.state_interval == 0 or curr_epoch + 1 == args.epoch):
            resume.atomic_save(resume.capture(args, curr_epoch, model, optimizer, (best_avg, best_epoch, best_avg_class), valdice,
                                              resume.gather_rng_states(device, augmenter, 1), 1,
                                              ema=(best_ema, valdice_ema) if ema_on else None),
                               resume.state_path(args.child, curr_epoch))
    logging.info("The best at epoch: {:d}, ".format(best_epoch)
                 + ", ".join("{}: {:.4f}".format(nm, v) for nm, v in zip(names[1:], best_avg_class))
                 + ", All: {:.4f}".format(best_avg))
    if ema_on:
        logging.info("The best EMA at epoch: {:d}, ".format(best_ema['epoch'])
                     + ", ".join("{}: {:.4f}".format(nm, v) for nm, v in zip(names[1:], best_ema['avg_class']))
                     + ", All: {:.4f}".format(best_ema['avg']))
        np.savez(os.path.join(args.child, 'valdice'), valdice=valdice, valdice_ema=valdice_ema)
    else:
        np.savez(os.path.join(args.child, 'valdice'), valdice=valdice)
    return valdice


def parse_args(argv=None):
    """parser.parse_args plus the check that spans --optimizer and --wd_exempt_1d (an argparse error: exit status 2)."""
    args = parser.parse_args(argv)
    check_optimizer_flags(parser, args)
    return args


def train_main(argv=None):
    from .train import DATASETS, apply_dataset_preset, split_dir
    args = apply_dataset_preset(parse_args(argv))
    if args.ramp_up_loss_boundary < 0 or not np.isfinite(args.loss_boundary_weight):
        parser.error('--loss_boundary_weight must be finite and --ramp_up_loss_boundary >= 0')
    if args.ramp_up_loss_lovasz < 0 or not np.isfinite(args.loss_lovasz_weight):
        parser.error('--loss_lovasz_weight must be finite and --ramp_up_loss_lovasz >= 0')
    # one process: the upper bound has no data-parallel path
    state_file, resume_state = resume.open_state(parser, args, 1) if args.resume else (None, None)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    sub = DATASETS.get(args.dataset, DATASETS['chaos'])['split_subdir'].format(modality=args.modality)
    if resume_state is not None:
        args.child = resume.run_dir_of(state_file)          # the run continues in its own directory
        resume.truncate_scalars(os.path.join(args.child, 'tb_summary', 'scalars.jsonl'), resume_state['epoch'])
    else:
        args.child = os.path.join(os.path.join(args.root, sub) if sub else args.root, args.session,
                                  f'{args.session}-{time.strftime("%H-%M-%S-%m%d")}-fold{args.fold}-{args.tag}')
        os.makedirs(args.child, exist_ok=False)
        os.makedirs(os.path.join(args.child, 'ckps'), exist_ok=True)
        os.makedirs(os.path.join(args.child, 'tb_summary'), exist_ok=True)
        if os.path.isfile(sys.argv[0]):
            shutil.copy(sys.argv[0], os.path.join(args.child, os.path.basename(sys.argv[0])))
    log = logging.getLogger()
    log.setLevel(logging.INFO)
    fh = logging.FileHandler(args.child + "/log.txt")
    fh.setFormatter(logging.Formatter('[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S'))
    log.addHandler(fh)
    log.addHandler(logging.StreamHandler(sys.stdout))
    logging.info(''.join(f'{k}={v}\n' for k, v in args._get_kwargs()))
    if resume_state is not None:
        logging.info("resumed from {} (epoch {:03d} done): continuing at epoch {:03d}".format(
            state_file, resume_state['epoch'], resume_state['epoch'] + 1))
    if not args.synthetic:
        data_root, base = split_dir(args.dataset, args.modality)
        with open(f'{base}/train_fold{args.fold}.txt', 'r') as f:
            args.train_ls = [(data_root + '/' + p).rstrip('\n') for p in f.readlines()]
        with open(f'{base}/test_fold{args.fold}.txt', 'r') as f:
            args.val_ls = [(data_root + '/' + p).rstrip('\n') for p in f.readlines()]
    return train_interface(args, resume_state)


if __name__ == '__main__':
    train_main()
