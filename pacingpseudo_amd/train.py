"""Training driver with the flag surface, run-directory layout, log lines and checkpoint files of the reference's
``train_chaos.py`` (train_chaos.py:23-179 flags, :431-463 run dir, :318,:396-399,:426 log lines, :405-413 checkpoints),
running the step on MI355X through ``pacingpseudo_amd``.

Kept from the reference: every flag name / type / default; ``{root}/{modality}/{session}/{session}-{time}-fold{k}-{tag}/``
with ``ckps/``, ``log.txt`` and ``valdice.npz``; per-epoch poly LR (utils.poly_lr_decay); the loss assembly of
train_chaos.py:273-310; ``model.eval()`` after the first epoch's validation and never back (train_chaos.py:370);
``ckps/ckp_{last}.pth`` + ``best_ckp.pth`` holding ``model.state_dict()`` (165 entries, reference key layout).

Changed on purpose: ``choices`` of --batch_size / --epoch / --lr / --wd / --init_ch / --max_ch are widened (the
reference rejects the benchmark's batch 32, train_chaos.py:93); loss meters stay on the GPU and are read once per
epoch instead of five ``.item()`` syncs per iteration; validation runs at the native slice size with its meters on the
GPU (one host sync per epoch, slices sharded over the ranks); the TensorBoard scalar tags (train_chaos.py:362-367,
:416-423) go to ``tb_summary/scalars.jsonl`` (tensorboard is not installed); its figures are dropped.
New flags: --synthetic N (phantom slices when no dataset is on disk), --image_size, --max_iters, and the
data-parallel launch is picked up from torch.distributed.run's environment (one process per GPU, RCCL).
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
from .regop import REGULARISERS, active_regularisers
from .optim import WD_HELP, add_clip_flag, add_ema_flags, add_wd_exempt_flag, check_optimizer_flags, log_clip_stats, positive_float, positive_int
from .utils.random_walker import add_rw_flags, add_rw_refresh_flags, check_rw_params, check_rw_refresh_flags
from .utils.geodesic import add_geo_flags, check_geo_params
from .utils.uncertainty import check_uncertainty_params, uncertainty_threshold

parser = argparse.ArgumentParser(description='PacingPseudo training on MI355X (flag surface of the reference driver)')


def _flags(title, ref, table):
    """One argparse group per block of the reference's flag list; `ref` = its line range in train_chaos.py.
    Names, types, defaults and choices are the reference's (tests/golden/flags.json); the help texts say what the
    flag selects in THIS implementation."""
    grp = parser.add_argument_group(f'{title} (train_chaos.py:{ref})')
    for name, kw in table:
        grp.add_argument('--' + name, **kw)


_on = dict(action='store_true')
_flags('run', '26-41', [
    ('gpu', dict(type=str, default='0', help='CUDA_VISIBLE_DEVICES of a single-process run (ignored under torch.distributed.run)')),
    ('seed', dict(type=int, default=1, help='python / numpy / torch seed; with the same seed the initial weights equal the reference\'s')),
    ('dataset', dict(type=str, default='chaos', help='chaos | acdc | lvsc: preset of class count, ignored index, crop size, class names')),
    ('root', dict(type=str, default='./outputs/chaos', help='run directories are created below <root>/<modality>/<session>/')),
    ('session', dict(type=str, default='Control', choices=['Control', 'Experiment'], help='first level of the run directory')),
    ('tag', dict(type=str, required=True, help='suffix of the run directory')),
])
_flags('data', '43-61', [
    ('fold', dict(type=int, default=1, choices=[0, 1, 2, 3, 4], help='which five-fold split files to read')),
    ('modality', dict(type=str, default='t1', choices=['t1', 't2'], help='sub-directory of the split files and of the outputs')),
    ('num_classes', dict(type=int, default=None, help='segmentation classes incl. background, excl. the ignored label (default: the --dataset preset, 5 for chaos)')),
    ('num_workers', dict(type=int, default=4, help='DataLoader worker processes')),
    ('augmentation_configs', dict(type=str, default='datasets.chaos.chaos_aug_configs',
                                  help='kept for compatibility; the transform list of all three data sets is built into augment.py')),
    ('augmentations', dict(type=str, default='TransformsColor',
                           choices=['TransformsColor', 'TransformsColorBlur', 'TransformsColorMixup', 'TransformsColorLow'],
                           help='strong-view recipe (colour transforms, + GaussianBlur / Mixup / SimulationLowRes)')),
])
_flags('network', '63-84', [
    ('input_ch', dict(type=int, default=1, help='image channels')),
    ('init_ch', dict(type=int, default=32, help='width of the first encoder stage; doubles per stage')),
    ('max_ch', dict(type=int, default=512, help='cap of the stage width')),
    ('output_stride', dict(type=int, default=8, choices=[32, 16, 8], help='encoder stride; deeper stages dilate instead of pooling')),
    ('is_stride_conv', dict(type=bool, default=False, help='stride-2 first convolution instead of max-pooling (models/unet.py:113; needs --is_trans_conv too)')),
    ('is_trans_conv', dict(type=bool, default=False, help='ConvTranspose2d instead of bilinear up-sampling (models/unet.py:140; needs --is_stride_conv too)')),
    ('elab_end_points', dict(type=bool, default=True, help='expose per-stage features (the aux path needs them)')),
])
_flags('optimisation', '86-112', [
    ('ignored_index', dict(type=int, default=None, help='label value of unlabelled pixels (= the extra scribble plane; default: the --dataset preset, 5 for chaos)')),
    ('epoch', dict(type=int, default=400, help='epochs; also the horizon of the LR schedule and of the memory momentum')),
    ('batch_size', dict(type=int, default=12, help='images per GPU and step')),
    ('optimizer', dict(type=str, default='adam', choices=['adam', 'momentum', 'adamw'],
                       help='FusedAdam, FusedSGD or FusedAdamW (one kernel over the flat parameter slab); adamw decouples --wd from the gradient')),
    ('momentum', dict(type=float, default=0.9, help='momentum of --optimizer momentum')),
    ('lr', dict(type=float, default=0.0001, help='learning rate at epoch 0')),
    ('lr_decay', dict(type=str, default='poly', choices=['linear', 'poly', 'cosine'], help='per-epoch schedule')),
    ('wd', dict(type=float, default=0.0003, help=WD_HELP)),
    ('ckp_interval', dict(type=int, default=10000, help='write ckps/ckp_<epoch>.pth every this many epochs (and at the end)')),
])
_flags('entropy minimisation', '114-126', [
    ('do_loss_ent', dict(default=False, help='add the entropy of the weak-view prediction', **_on)),
    ('loss_ent_weight', dict(type=float, default=1., help='its weight')),
    ('ramp_up_loss_ent', dict(default=True, help='Gaussian ramp-up of that weight over the epochs', **_on)),
    ('ramp_up_scale', dict(type=float, default=8., choices=[5., 8., 10.], help='sharpness of the ramp-ups')),
])
_flags('decoder consistency', '128-145', [
    ('do_decoder_consistency', dict(default=False, help='second (strong-view) pass + consistency loss between the two predictions', **_on)),
    ('ramp_up_loss_cr', dict(default=True, help='Gaussian ramp-up of its weight', **_on)),
    ('detach_weak_cr', dict(default=False, help='treat the weak-view probabilities as a constant target', **_on)),
    ('loss_cr_variants', dict(type=str, default='ce_loss', choices=['ce_loss', 'l1_loss', 'l2_loss', 'kl_loss', 'bikl_loss', 'js_loss', 'hard_ce_loss'],
                              help='form of the consistency loss (all seven in pp_seg_losses_*; the last three -- symmetric KL, '
                                   'Jensen-Shannon, cross entropy against the weak arg-max -- are additions to the reference)')),
    ('strength', dict(type=float, default=1., choices=[0.125, 0.25, 0.5, 1.], help='range of the strong view\'s colour transforms')),
    ('loss_cr_weight', dict(type=float, default=1., help='weight of the consistency loss')),
])
_flags('auxiliary path', '147-169', [
    ('do_aux_path', dict(default=False, help='low-resolution classification head on the encoder output', **_on)),
    ('feat_stage', dict(type=list, default=['encoder/stage6', 'encoder/stage5'], help='encoder features it concatenates')),
    ('feat_ch', dict(type=list, default=[512, 512], help='their channel counts')),
    ('loss_aux_weight', dict(type=float, default=0.01, choices=[1., 0.01, 0.001], help='weight of its partial cross-entropy')),
    ('hid_ch', dict(type=int, default=64, choices=[256, 128, 64], help='embedding width = width of a memory-bank row')),
    ('aux_drop_prob', dict(type=float, default=0., choices=[0., 0.5, 0.8], help='Dropout2d on the embedding')),
])
_flags('memory bank', '171-179', [
    ('do_memory', dict(default=False, help='class prototypes updated from labelled pixels + their classification loss', **_on)),
    ('loss_memory_weight', dict(type=float, default=1, choices=[1., 0.01], help='weight of that loss')),
    ('update_momentum', dict(type=float, default=0.9, help='start of the EMA momentum schedule of the prototypes')),
    ('ensemble_mode', dict(type=str, default='cosine_similarity', choices=['cosine_similarity', 'mean'],
                           help='how labelled pixel embeddings are pooled into a prototype')),
])
# ---- additions of this implementation
parser.add_argument('--synthetic', type=int, default=0,
                    help='train on N synthetic phantom slices (and N//4 validation slices) instead of ./data')
parser.add_argument('--gpu_augment', action='store_true',
                    help='accepted for compatibility: the two-stream augmentation pipeline of datasets/augmentations.py on the GPU '
                         '(augment.py) is the default input path')
parser.add_argument('--cpu_input', action='store_true',
                    help='minimal CPU input path of data.py (MeanStdNorm, centre crop, colour jitter only: no Scaling / Elastic / '
                         'Rotation / Mirroring / Noise / RandomCrop) instead of the GPU pipeline')
parser.add_argument('--image_size', type=int, default=None, help='network input size of the TRAINING crops (default: the --dataset preset, 256 for chaos); validation runs at the native slice size')
parser.add_argument('--max_iters', type=int, default=0, help='stop each epoch after this many iterations (0 = all)')
parser.add_argument('--precision', type=str, default='fp32', choices=['fp32', 'fp16'],
                    help='fp32: every matrix product at fp32 grade (three fp16 MFMA products of split operands); fp16: the forward / '
                         'data-gradient products of the halo-tile and Winograd kernels use fp16 operands with fp32 accumulation '
                         '(mixed precision, BASELINE config 5; so does the Winograd weight-gradient GEMM; tensors in HBM stay fp32 unless --storage fp16)')
parser.add_argument('--storage', type=str, default='fp32', choices=['fp32', 'fp16', 'bf16'],
                    help='fp16 / bf16: activations and activation gradients of the TRAINING step live in HBM as IEEE fp16 / bfloat16 '
                         '(16-bit storage, BASELINE config 5 -- which names bf16: half the activation traffic; fp32 accumulation, '
                         'statistics, weights and parameter gradients; static loss scale).  fp16 keeps 11 significand bits, bf16 8 '
                         '(tests/test_gpu_h16.py states both tolerances).  Validation / inference stay fp32')
parser.add_argument('--graph_step', action='store_true',
                    help='replay the iteration (forward, losses, backward, optimizer) from a hipGraph captured once per epoch '
                         '(pacingpseudo_amd/graph.py): ONE host call per step instead of ~300 launches -- for hosts that cannot keep '
                         'ahead of the GPU; bit-identical to the eager step (single process or RCCL)')
parser.add_argument('--sync_bn', action='store_true',
                    help='data-parallel runs: BatchNorm batch statistics over the GLOBAL batch during epoch 0 '
                         '(= the single-process step on the concatenated batch); default: per-rank statistics, '
                         'running buffers averaged before the switch to eval mode; no effect on --norm_op group blocks')
parser.add_argument('--norm_op', type=str, default='batch', choices=['batch', 'group'],
                    help='block normaliser of the U-Net: batch = nn.BatchNorm2d (the reference); group = nn.GroupNorm(--norm_groups, C): '
                         'per-image statistics, no running state, the same function in train and eval mode (fp32 storage only)')
parser.add_argument('--norm_groups', type=int, default=8, help='channel groups of --norm_op group; must divide every block width')
# gated-CRF / Potts regulariser on the weak-view prediction (pp_crf_loss_*); the reference has no such loss
parser.add_argument('--do_loss_crf', action='store_true',
                    help='add the local pairwise gated-CRF loss: neighbouring pixels of similar intensity are pulled towards the same '
                         'class (bilateral kernel on position and image intensity, one tiled HIP kernel per step)')
parser.add_argument('--loss_crf_weight', type=float, default=0.1, help='its weight')
parser.add_argument('--ramp_up_loss_crf', action='store_true', help='Gaussian ramp-up of that weight over the epochs (--ramp_up_scale)')
parser.add_argument('--crf_radius', type=positive_int, default=5, help='neighbourhood radius r: offsets dy, dx in [-r, r] (1 .. 8)')
parser.add_argument('--crf_dilation', type=positive_int, default=1, help='spacing d of the neighbourhood offsets in pixels (1 .. 4, r * d <= 16)')
parser.add_argument('--crf_sigma_xy', type=positive_float, default=6.0, help='width of the position kernel, in offsets')
parser.add_argument('--crf_sigma_rgb', type=positive_float, default=0.1, help='width of the intensity kernel, in units of the network input')
# normalised cut on the weak-view prediction over the same local bilateral window (pp_nc_loss_*); the reference has
# no such loss.  It divides each class's cut by that class's volume, so it lacks the Potts term's shrinking bias; the two may be on together
parser.add_argument('--do_loss_nc', action='store_true',
                    help='add the normalised-cut loss: per image and class, 1 - association / volume over a local bilateral window '
                         '(--nc_radius, --nc_dilation, --nc_sigma_xy, --nc_sigma_rgb)')
parser.add_argument('--loss_nc_weight', type=float, default=0.1, help='its weight (an untuned first value)')
parser.add_argument('--ramp_up_loss_nc', action='store_true', help='Gaussian ramp-up of that weight over the epochs (--ramp_up_scale)')
parser.add_argument('--nc_radius', type=positive_int, default=5, help='neighbourhood radius r: offsets dy, dx in [-r, r] (1 .. 8)')
parser.add_argument('--nc_dilation', type=positive_int, default=1, help='spacing d of the neighbourhood offsets in pixels (1 .. 4, r * d <= 16)')
parser.add_argument('--nc_sigma_xy', type=positive_float, default=6.0, help='width of the position kernel, in offsets')
parser.add_argument('--nc_sigma_rgb', type=positive_float, default=0.1, help='width of the intensity kernel, in units of the network input')
# Mumford-Shah level-set loss with a total-variation term on the weak-view prediction (pp_ms_loss_*); the reference
# has no such loss.  It asks that each class region be piecewise constant in the image (a per-image region statistic) and that the class
# maps have short boundaries; it may be on together with the CRF and the normalised-cut losses
parser.add_argument('--do_loss_ms', action='store_true',
                    help='add the Mumford-Shah level-set loss: per image and class the soft-region variance of the image intensities, '
                         'plus --ms_tv_weight times the anisotropic total variation of the class maps')
parser.add_argument('--loss_ms_weight', type=float, default=0.1, help='its weight (an untuned first value)')
parser.add_argument('--ramp_up_loss_ms', action='store_true', help='Gaussian ramp-up of that weight over the epochs (--ramp_up_scale)')
parser.add_argument('--ms_tv_weight', type=float, default=1.0,
                    help='weight of the total-variation term inside that loss, >= 0 (an untuned first value)')
# mean teacher: the weak side of the consistency term from the EMA weights (engine.py: a forward-only pass reading the optimizer's
# shadow slab); the reference has no such option
parser.add_argument('--cr_teacher', type=str, default='none', choices=['none', 'ema'],
                    help='ema: the consistency loss pulls the strong-view prediction towards the prediction of the EMA weights for the '
                         'weak view (mean teacher; needs --do_decoder_consistency and --ema_decay > 0; the teacher gets no gradient, '
                         'so --detach_weak_cr has nothing to do); none: towards the weak-view prediction of the same weights')
# ... and its uncertainty mask (UA-MT / USTM; libpacingpseudo_unc.so, utils/uncertainty.py): the teacher call acts
# only where the entropy of the teacher's mean soft-max over T noise-perturbed passes is below a threshold relaxed over the epochs
parser.add_argument('--cr_uncertainty', type=int, default=0,
                    help='T noisy teacher passes per step for the uncertainty mask of the consistency term, 1..16 (needs --cr_teacher '
                         'ema; 0: off, the step as it was; untuned first value)')
parser.add_argument('--cr_uncertainty_sigma', type=float, default=0.1,
                    help='standard deviation of the Gaussian input noise of those passes, >= 0; 0 needs --cr_uncertainty 1 and masks '
                         'by the plain entropy of the clean teacher pass (untuned first value)')
parser.add_argument('--cr_uncertainty_clip', type=float, default=0.2,
                    help='the noise is clamped to [-clip, +clip], >= 0 (untuned first value)')
parser.add_argument('--cr_uncertainty_start', type=float, default=0.75,
                    help='the entropy threshold starts at this fraction of ln K and ramps up to ln K (--ramp_up_scale), in (0, 1] '
                         '(untuned first value)')
add_clip_flag(parser)                         # --clip_grad_norm X (pacingpseudo_amd/optim.py)
add_ema_flags(parser)                         # --ema_decay D / --ema_val_interval N (pacingpseudo_amd/optim.py)
add_wd_exempt_flag(parser)                    # --wd_exempt_1d, with --optimizer adamw (pacingpseudo_amd/optim.py)
resume.add_flags(parser)                      # --state_interval N / --resume PATH (pacingpseudo_amd/resume.py)
finetune.add_flags(parser)                    # --freeze_encoder N / --init_from PATH / --init_reset_head (pacingpseudo_amd/finetune.py)
# random-walker expansion of the training scribbles, once before the first step (libpacingpseudo_prep.so); the
# reference has no such stage.  It acts on the labels, not on a loss: everything downstream sees an ordinary scribble map
add_rw_flags(parser)                          # --rw_scribbles / --rw_beta / --rw_threshold / --rw_eps / --rw_tol / --rw_max_iters
# ... and its second half: every N epochs the walker runs again with the network's own soft-max as a unary prior beside the seeds
# (libpacingpseudo_rwp.so) and the pseudo-labels are replaced, between epochs, never inside a step
add_rw_refresh_flags(parser)                  # --rw_refresh / --rw_refresh_start / --rw_prior_gamma
# the other classical expansion, also once before the first step: geodesic distance of the seeds on the normalised image
# (libpacingpseudo_geo.so).  One of the two: --geo_scribbles with --rw_scribbles is an error
add_geo_flags(parser)                         # --geo_scribbles / --geo_lambda / --geo_ratio / --geo_max_dist / --geo_max_sweeps


# The reference ships ONE driver (train_chaos.py) and three dataset packages that differ only in class tables and
# crop size (datasets/{chaos,acdc,lvsc}/*_dataset.py:17-24, *_aug_configs.py:9-13).  --dataset selects the preset; the
# explicit --num_classes / --ignored_index / --image_size flags still win when they are given.
# `split_subdir`: where the five-fold split files live below ./data/<dataset>/train_test_split/five_fold_split/ and which
# sub-directory of --root the runs go to: CHAOS has one per modality, ACDC / LVSC have none (reference inference.py:301-318).
DATASETS = {
    'chaos': dict(num_classes=5, ignored_index=5, image_size=256, names=['BG', 'Liver', 'R-Kidney', 'L-Kidney', 'Spleen'],
                  split_subdir='{modality}'),
    'acdc': dict(num_classes=4, ignored_index=4, image_size=224, names=['BG', 'RV', 'Myo', 'LV'], split_subdir=''),
    'lvsc': dict(num_classes=2, ignored_index=2, image_size=224, names=['BG', 'Myo'], split_subdir=''),
}


def split_dir(dataset: str, modality: str = 't1'):
    """(data root, directory of the train_fold<k>.txt / test_fold<k>.txt lists) -- shared with inference.py."""
    sub = DATASETS[dataset]['split_subdir'].format(modality=modality)
    root = f'./data/{dataset}'
    return root, os.path.join(root, 'train_test_split', 'five_fold_split', sub).rstrip('/')


def _class_names(n, dataset='chaos'):
    names = list(DATASETS.get(dataset, DATASETS['chaos'])['names'])
    return names[:n] + [f'C{i}' for i in range(len(names), n)]


def apply_dataset_preset(args, argv=None):
    """Fill num_classes / ignored_index / image_size from the --dataset preset unless the flag was given: the three flags
    default to None, so whatever argparse accepted (abbreviations included) counts as given."""
    preset = DATASETS.get(args.dataset, DATASETS['chaos'])
    for key in ('num_classes', 'ignored_index', 'image_size'):
        if getattr(args, key, None) is None:
            setattr(args, key, preset[key])
    return args


def parse_args(argv=None):
    """parser.parse_args plus the checks that span several flags (argparse errors: exit status 2)."""
    args = parser.parse_args(argv)
    check_optimizer_flags(parser, args)
    for r in REGULARISERS.values():
        try:
            r.check(**r.args_params(args))
        except (ValueError, NotImplementedError) as e:
            parser.error(' / '.join(f'--{r.name}_{p}' for p in r.params) + f': {e}')
    try:
        check_rw_params(args.rw_beta, args.rw_eps, args.rw_tol, args.rw_max_iters, args.rw_threshold)
    except (ValueError, NotImplementedError) as e:
        parser.error(f'--rw_beta / --rw_eps / --rw_tol / --rw_max_iters / --rw_threshold: {e}')
    try:
        check_rw_refresh_flags(args.rw_refresh, args.rw_refresh_start, args.rw_prior_gamma)
    except ValueError as e:
        parser.error(f'--rw_refresh / --rw_refresh_start / --rw_prior_gamma: {e}')
    try:
        check_geo_params(args.geo_lambda, args.geo_ratio, args.geo_max_dist, args.geo_max_sweeps)
    except (ValueError, NotImplementedError) as e:
        parser.error(f'--geo_lambda / --geo_ratio / --geo_max_dist / --geo_max_sweeps: {e}')
    if args.geo_scribbles and args.rw_scribbles:
        parser.error('--geo_scribbles and --rw_scribbles both expand the scribbles before the first step: give one of them')
    if args.cr_teacher == 'ema':
        if not args.do_decoder_consistency:
            parser.error('--cr_teacher ema: the teacher is the weak side of the consistency term; add --do_decoder_consistency')
        if not args.ema_decay > 0.0:
            parser.error('--cr_teacher ema: the teacher is the EMA of the weights; set --ema_decay D with 0 < D < 1')
    if args.cr_uncertainty:
        if args.cr_teacher != 'ema':
            parser.error('--cr_uncertainty: the mask acts on the EMA teacher\'s side of the consistency term; add --cr_teacher ema')
        try:
            check_uncertainty_params(args.cr_uncertainty, args.cr_uncertainty_sigma, args.cr_uncertainty_clip, args.cr_uncertainty_start,
                                     K=DATASETS.get(args.dataset, DATASETS['chaos'])['num_classes'] if args.num_classes is None
                                     else args.num_classes)
        except (ValueError, NotImplementedError) as e:
            parser.error(f'--cr_uncertainty / --cr_uncertainty_sigma / --cr_uncertainty_clip / --cr_uncertainty_start: {e}')
    return args


def train_interface(args, resume_state=None):
    from . import parallel
    from .data import SyntheticPhantoms, collate_by_shape, dataset_class, expand_compact, loader_context
    from .models import ConsistencyRegulr
    from .models.unet import norm_kwargs
    from .optim import FusedAdam, FusedAdamW, FusedSGD
    from .utils import AvgMeter, cosine_lr_decay, gaussian_ramp_up, linear_lr_decay, poly_lr_decay
    from .losses.losses import weighted_loss_sum
    from .utils.metrics import ValAccumulator
    from .utils.scalars import ScalarLog

    world, rank, local_rank = parallel.init_from_env('nccl')
    device = torch.device('cuda', local_rank)
    torch.cuda.set_device(device)
    best_avg, best_epoch, best_avg_class = 0, 0, []
    from ._lib import lib
    lib.pp_set_matrix_products(1 if getattr(args, 'precision', 'fp32') == 'fp16' else 3)

    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=args.input_ch, init_ch=args.init_ch, max_ch=args.max_ch,
                         num_classes=args.num_classes, output_stride=args.output_stride,
                         is_stride_conv=args.is_stride_conv, is_trans_conv=args.is_trans_conv,
                         elab_end_points=args.elab_end_points, **norm_kwargs(args)),
        kwargs_aux_path=dict(num_classes=args.num_classes, feat_stage=args.feat_stage, feat_ch=args.feat_ch,
                             hid_ch=args.hid_ch, aux_drop_prob=args.aux_drop_prob, do_memory=args.do_memory,
                             max_step=args.epoch, update_momentum=args.update_momentum,
                             ensemble_mode=args.ensemble_mode),
        args_parser=args).cuda()
    # --init_from / --freeze_encoder: before the optimizer, the EMA slab and the data-parallel broadcast see the parameters
    finetune.init_model(args, model, parser, logging.info if rank == 0 else None)
    if world > 1:
        parallel.attach(model, sync_bn=args.sync_bn)
    if rank == 0:
        logging.info(model)

    if args.optimizer == 'adam':
        optimizer = FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wd, max_grad_norm=args.clip_grad_norm or None,
                              ema_decay=args.ema_decay or None)
    elif args.optimizer == 'momentum':
        optimizer = FusedSGD(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.wd,
                             max_grad_norm=args.clip_grad_norm or None, ema_decay=args.ema_decay or None)
    elif args.optimizer == 'adamw':
        optimizer = FusedAdamW(model.parameters(), lr=args.lr, weight_decay=args.wd, exempt_1d=args.wd_exempt_1d,
                               max_grad_norm=args.clip_grad_norm or None, ema_decay=args.ema_decay or None)
    else:
        raise ValueError('Unimplemented optimizer')
    if args.cr_teacher == 'ema':                  # the shadow slab exists from here on (resume.restore then loads the saved one)
        # --cr_uncertainty: behind parallel.attach (the noise seed is mixed with the rank); resume.restore puts the saved step back
        model.attach_teacher(optimizer, uncertainty=dict(passes=args.cr_uncertainty, sigma=args.cr_uncertainty_sigma,
                                                         clip=args.cr_uncertainty_clip, start=args.cr_uncertainty_start,
                                                         seed=int(args.seed) & ((1 << 64) - 1)) if args.cr_uncertainty else None)

    args.gpu_augment = not args.cpu_input          # the reference's recipe is the default; --cpu_input opts out
    if args.augmentations != 'TransformsColor' and not args.gpu_augment:
        raise NotImplementedError(f'--augmentations {args.augmentations} is not available with --cpu_input: the minimal CPU '
                                  'input path of data.py only has the colour jitter')
    ds_kw = dict(num_classes=args.num_classes, size=args.image_size, strength=args.strength, seed=args.seed)
    augmenter, collate = None, None
    if args.gpu_augment:
        # the reference's two-stream pipeline (chaos_dataset.py:58-90) on the device: the loader hands over raw slices
        from .augment import AugConfig, DeviceAugmenter, collate_raw
        augmenter = DeviceAugmenter(AugConfig(num_classes=args.num_classes, crop_size=(args.image_size, args.image_size),
                                              strength=args.strength, do_strong=args.do_decoder_consistency,
                                              recipe=args.augmentations),
                                    device=device, seed=args.seed + 7919 * rank)
        collate = collate_raw
    if args.synthetic:
        train_dataset = SyntheticPhantoms(args.synthetic, do_strong=args.do_decoder_consistency, train=True,
                                          raw=args.gpu_augment, **ds_kw)
        val_dataset = SyntheticPhantoms(max(args.synthetic // 4, 1), train=False, native=True, compact=True, **ds_kw)
    else:
        train_dataset = dataset_class(args.dataset)(args.train_ls, do_strong=args.do_decoder_consistency, train=True, raw=args.gpu_augment,
                                  **ds_kw)
        val_dataset = dataset_class(args.dataset)(args.val_ls, train=False, native=True, compact=True, **ds_kw)
        # Mixup blends with a slice drawn from the whole training list (datasets/augmentations.py:66): the loader draws it
        train_dataset.mix_partner = bool(args.gpu_augment and args.augmentations == 'TransformsColorMixup')
    rw_summary = None
    if getattr(args, 'rw_scribbles', False):
        # every training slice once, before any loader worker exists; every rank computes the full list (the same bits on each),
        # a resumed run recomputes it.  Validation data are not touched.
        from .utils.random_walker import expand_dataset, summarize, summary_line
        prm = check_rw_params(args.rw_beta, args.rw_eps, args.rw_tol, args.rw_max_iters, args.rw_threshold, K=args.num_classes)
        train_dataset.scribble_override, rw_report = expand_dataset(train_dataset, args.num_classes, device, prm)
        rw_summary = summarize(rw_report)
        if rank == 0:
            logging.info(summary_line(rw_summary))
            if rw_summary['unconverged']:
                logging.warning('random-walker scribbles: %d systems stopped at --rw_max_iters %d before --rw_tol %g, first slices: %s',
                                rw_summary['unconverged'], prm['max_iters'], prm['tol'], rw_summary['unconverged_slices'][:8])
            np.savez(os.path.join(args.child, 'rw_scribbles.npz'), **rw_report, **{'param_' + k: v for k, v in prm.items()})
    if getattr(args, 'geo_scribbles', False):
        # the same place and the same contract as --rw_scribbles: every rank computes the full list (the same bits on each, and
        # in a resumed run), --rw_refresh starts from it, validation data are not touched
        from .utils.geodesic import expand_dataset_geo, summarize_geo, summary_line_geo
        gprm = check_geo_params(args.geo_lambda, args.geo_ratio, args.geo_max_dist, args.geo_max_sweeps, K=args.num_classes)
        train_dataset.scribble_override, geo_report = expand_dataset_geo(train_dataset, args.num_classes, device, gprm)
        geo_summary = summarize_geo(geo_report)
        if rank == 0:
            logging.info(summary_line_geo(geo_summary))
            if geo_summary['unconverged']:
                logging.warning('geodesic scribbles: %d planes stopped at --geo_max_sweeps %d, first slices: %s',
                                geo_summary['unconverged'], gprm['max_sweeps'], geo_summary['unconverged_slices'][:8])
            np.savez(os.path.join(args.child, 'geo_scribbles.npz'), **geo_report, **{'param_' + k: v for k, v in gprm.items()})
    # --rw_refresh: the maps live in ONE shared-memory buffer from before the loaders exist, so that the persistent workers see what
    # a refresh writes into it.  Until the first refresh it holds the --rw_scribbles expansion if given, else the scribbles on disk;
    # a resumed run loads the maps of the last refresh the saved epoch had seen.
    rw_every, rw_start, rw_gamma = check_rw_refresh_flags(args.rw_refresh, args.rw_refresh_start, args.rw_prior_gamma)
    rw_shared = None
    if rw_every:
        from .utils.random_walker import SharedMaps
        first = train_dataset.scribble_override
        if first is None:
            first = [np.asarray(train_dataset.raw_arrays(i)[2]).astype(np.uint8) for i in range(len(train_dataset))]
        rw_shared = SharedMaps(first)
        if resume_state is not None:
            saved = resume.load_refresh_maps(args.child, resume_state['epoch'], rw_every, rw_start, rw_shared.shapes)
            for i, m in enumerate(saved or ()):
                rw_shared.update(i, m)
        train_dataset.scribble_override = rw_shared
    sampler = torch.utils.data.distributed.DistributedSampler(train_dataset, world, rank, shuffle=True,
                                                              seed=args.seed, drop_last=True) if world > 1 else None
    train_loader = torch.utils.data.DataLoader(train_dataset, batch_size=args.batch_size, shuffle=sampler is None,
                                               sampler=sampler, num_workers=args.num_workers, drop_last=True,
                                               collate_fn=collate,
                                               # raw slices carry no per-epoch state: keep the workers alive across epochs
                                               # (re-forking them cost a third of a 1.5 s epoch in the r02 end-to-end run)
                                               persistent_workers=bool(args.gpu_augment and args.num_workers > 0),
                                               multiprocessing_context=loader_context(args.num_workers),
                                               pin_memory=bool(args.gpu_augment))
    # validation as train_chaos.py:235-241 runs it (MeanStdNorm only, native slice size), but: every rank scores its share of
    # the slices (strided, no padding duplicates), the workers stay alive across epochs, the meters live on the device
    val_subset = torch.utils.data.Subset(val_dataset, list(range(rank, len(val_dataset), world))) if world > 1 else val_dataset
    val_loader = torch.utils.data.DataLoader(val_subset, batch_size=args.batch_size, shuffle=False,
                                             num_workers=args.num_workers, drop_last=False, collate_fn=collate_by_shape,
                                             persistent_workers=args.num_workers > 0, pin_memory=True,
                                             multiprocessing_context=loader_context(args.num_workers))
    names = _class_names(args.num_classes, args.dataset)
    scalars = ScalarLog(os.path.join(args.child, 'tb_summary', 'scalars.jsonl')) if rank == 0 else None
    if scalars is not None and rw_summary is not None and resume_state is None:      # a resumed run keeps the first run's two lines
        scalars.add('RW/coverage', rw_summary['coverage_after'], 0)
        scalars.add('RW/agreement', rw_summary['agreement'], 0)
    valdice = np.zeros(args.epoch)
    # --ema_decay: the same bookkeeping a second time for the averaged weights (epochs without an EMA validation pass stay 0)
    ema_on = bool(args.ema_decay)
    valdice_ema = np.zeros(args.epoch) if ema_on else None
    best_ema = dict(avg=0, epoch=0, avg_class=[])
    graph_step = None                            # --graph_step: pacingpseudo_amd.graph.GraphedStep, built on first use
    aug_stream = torch.cuda.Stream() if (augmenter is not None and os.environ.get('PP_AUG_STREAM', '1') != '0') else None
    start_epoch = 0
    if resume_state is not None:
        best_avg, best_epoch, best_avg_class = resume.restore(resume_state, model, optimizer, valdice)
        if ema_on:
            best_ema = resume.restore_ema(resume_state, valdice_ema)
        train_dataset.set_epoch(0)                 # what the uninterrupted run's persistent workers were forked with
        resume.prime_persistent_loaders([train_loader, val_loader])
        resume.set_rng_states(resume_state['rng'][rank], device, augmenter)
        start_epoch = resume_state['epoch'] + 1

    def validate():
        """One pass over this rank's share of the validation slices with the weights the model holds: (per-class Dice, loss_pce)."""
        meters = ValAccumulator(args.num_classes, device)
        for groups in val_loader:
            for batch in groups:                   # same-shape groups of one loader batch (collate_by_shape)
                batch = expand_compact(batch, args.num_classes, device)      # uint8 class maps -> one-hot planes, on the device
                with torch.no_grad():
                    net_outputs = model(batch, mode='val')
                meters.update(net_outputs['segmentation/logits'], batch['label'], net_outputs['loss_pce'])
        dsc, loss_pce_val, _ = meters.result(parallel.all_reduce_sum if world > 1 else None)   # the one host sync
        return dsc, loss_pce_val

    def rw_refresh(epoch):
        """--rw_refresh: new pseudo-labels for every training slice from the live weights (every rank computes the whole set: the same
        bits on each), written into the shared maps before this epoch's loader iterator exists.  Leaves nothing else behind."""
        from .utils.random_walker import refresh_dataset, refresh_forward, refresh_summary_line, summarize
        prm = dict(check_rw_params(args.rw_beta, args.rw_eps, args.rw_tol, args.rw_max_iters, args.rw_threshold, K=args.num_classes),
                   gamma=rw_gamma)
        tic = time.time()
        maps, rep = refresh_dataset(train_dataset, refresh_forward(model, args.num_classes), args.num_classes, device, prm,
                                    args.output_stride)
        for i, m in enumerate(maps):
            rw_shared.update(i, m)
        if rank == 0:
            s = summarize(rep)
            skipped, changed = int(rep['skipped'].sum()), float(rep['changed'].mean())
            logging.info(refresh_summary_line(s, epoch, skipped, changed) + ', {:.2f} s'.format(time.time() - tic))
            scalars.add('RW/refresh_coverage', s['coverage_after'], epoch)
            scalars.add('RW/refresh_agreement', s['agreement'], epoch)
            scalars.add('RW/refresh_changed', changed, epoch)
            resume.save_refresh_maps(resume.refresh_maps_path(args.child, epoch), maps, rep, prm)

    for curr_epoch in range(start_epoch, args.epoch):
        if rw_every and curr_epoch >= rw_start and (curr_epoch - rw_start) % rw_every == 0:
            rw_refresh(curr_epoch)
        epoch_tic = time.time()
        if sampler is not None:
            sampler.set_epoch(curr_epoch)
        train_dataset.set_epoch(curr_epoch)           # strong-view jitter differs per epoch (workers re-fork per epoch)
        if args.lr_decay == 'poly':
            optimizer, new_lr = poly_lr_decay(optimizer, curr_epoch, args.epoch, args.lr)
        elif args.lr_decay == 'cosine':
            optimizer, new_lr = cosine_lr_decay(optimizer, curr_epoch, args.epoch, args.lr)
        elif args.lr_decay == 'linear':
            optimizer, new_lr = linear_lr_decay(optimizer, curr_epoch, args.epoch, args.lr)
        else:
            raise ValueError('Unimplemented learning rate decay policy.')

        # loss meters live on the GPU: [sum pce*n, sum ent*n, sum cr*n, sum aux*n, sum mem, n, iterations]
        acc = torch.zeros(7, device=device, dtype=torch.float64)
        # the regularisers that are on, in the table's order, as (output key, weight of this epoch); their meters: sum loss*n each
        regs = [(r.key, gaussian_ramp_up(t=curr_epoch, base_value=getattr(args, r.weight), scale=args.ramp_up_scale)
                 if getattr(args, r.ramp) else getattr(args, r.weight)) for r in active_regularisers(args)]
        acc_reg = torch.zeros(len(regs), device=device, dtype=torch.float64)
        # --cr_uncertainty: [sum over steps of kept / valid pixels, sum of the mean entropy over valid pixels]
        unc_on = bool(args.cr_uncertainty)
        acc_unc = torch.zeros(2, device=device, dtype=torch.float64) if unc_on else None
        if unc_on and rank == 0:
            logging.info("epoch: {:03d}, uncertainty threshold theta: {:.6f} (ln K = {:.6f})".format(
                curr_epoch, uncertainty_threshold(curr_epoch, args.cr_uncertainty_start, args.num_classes, args.ramp_up_scale),
                np.log(args.num_classes)))
        n_img = 0
        for idx, batch in enumerate(train_loader):
            if args.max_iters and idx >= args.max_iters:
                break
            if augmenter is not None:
                # upload + augmentation on their own stream: the host runs a step ahead of the GPU, so the 25 MB host-to-device copy
                # and the ~1.4 ms of augmentation kernels of THIS batch execute beside the previous training step instead of in
                # front of this one (round 5: 1,045 -> ~1,130 images/s through the driver in the reference's steady state)
                batch = augmenter.ahead(aug_stream, batch['img'], batch['lab'], batch['scb'], batch['sizes'], batch.get('mix'), batch.get('mix_sizes'))
            batch.pop('label', None)
            batch.pop('label_strong', None)
            batch = {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
            n = batch['image'].shape[0]
            # loss assembly of train_chaos.py:273-310; the ramp-up weights depend on the epoch only
            w_ent = gaussian_ramp_up(t=curr_epoch, base_value=args.loss_ent_weight, scale=args.ramp_up_scale) if args.ramp_up_loss_ent else 1.0
            w_cr = gaussian_ramp_up(t=curr_epoch, base_value=args.loss_cr_weight, scale=args.ramp_up_scale) if args.ramp_up_loss_cr else 1.0

            def assemble(out, _epoch=None):
                # train_chaos.py:273-310: pce + ent * w_ent + cr * w_cr + aux * w_aux + memory * w_mem -- one launch each way
                # (weighted_loss_sum: the same fp32 products and sums in the same order as the chain of torch operations)
                terms, weights = [out['loss_pce']], [1.0]
                if args.do_loss_ent:
                    terms.append(out['loss_ent']); weights.append(w_ent)
                if args.do_decoder_consistency:
                    terms.append(out['loss_cr']); weights.append(w_cr)
                if args.do_aux_path:
                    terms.append(out['loss_aux_cls']); weights.append(args.loss_aux_weight)
                    if args.do_memory:
                        terms.append(out['loss_memory']); weights.append(args.loss_memory_weight)
                for key, w in regs:
                    terms.append(out[key]); weights.append(w)
                return weighted_loss_sum(terms, weights)
            if args.graph_step and n == args.batch_size:      # (a ragged last batch runs eagerly: another shape, another plan)
                if graph_step is None:
                    from .graph import GraphedStep
                    graph_step = GraphedStep(model, optimizer, assemble, warmup=2)
                graph_step.loss_fn = assemble
                _, net_outputs = graph_step(batch, curr_epoch)
            else:
                net_outputs = model(batch, mode='train', step=curr_epoch)
                loss = assemble(net_outputs)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            acc[0] += net_outputs['loss_pce'].detach() * n
            if args.do_loss_ent:
                acc[1] += net_outputs['loss_ent'].detach() * (w_ent * n)
            if args.do_decoder_consistency:
                acc[2] += net_outputs['loss_cr'].detach() * (w_cr * n)
            if args.do_aux_path:
                acc[3] += net_outputs['loss_aux_cls'].detach() * (args.loss_aux_weight * n)
                if args.do_memory:
                    acc[4] += net_outputs['loss_memory'].detach() * args.loss_memory_weight
            for i, (key, w) in enumerate(regs):
                acc_reg[i] += net_outputs[key].detach() * (w * n)
            if unc_on:
                ust = model.engine.uncertainty_stats()          # double[3] on the device: (sum m, sum u over valid, valid pixels)
                acc_unc += ust[:2] / ust[2].clamp(min=1.0)
            acc[5] += n
            acc[6] += 1
            n_img += n
        a = (torch.cat([acc, acc_reg]) if regs else acc).cpu().numpy()      # the one host sync of the epoch; [7 + i]: regs[i]
        epoch_toc = time.time()
        cnt, its = max(a[5], 1), max(a[6], 1)
        # 16-bit storage: optimizer steps the overflow guard skipped this epoch (a static loss scale that keeps
        # overflowing used to skip every update silently).  Read with the epoch's one host sync; when MOST of the epoch's updates
        # were skipped the scale is halved for the following epochs (a power of two: exact to remove), never silently.
        flat = getattr(model, 'flat', None)
        if flat is not None and getattr(flat, 'guard_on', False):
            total_skipped = int(flat.guard[1])
            skipped = total_skipped - getattr(flat, '_skipped_logged', 0)
            flat._skipped_logged = total_skipped
            if skipped:
                msg = "epoch: {:03d}: {} of {} optimizer steps skipped (non-finite gradients at loss scale {:g})".format(
                    curr_epoch, skipped, int(its), model.engine.loss_scale)
                if skipped * 2 > its:
                    new_scale = model.engine.set_loss_scale(model.engine.loss_scale / 2.0)
                    msg += "; loss scale halved to {:g}".format(new_scale)
                if rank == 0:
                    logging.warning(msg)
                if skipped >= its and model.engine.loss_scale < 1.0:
                    raise FloatingPointError('every optimizer step of the epoch was skipped even at loss scale < 1: the gradients '
                                             'themselves are not finite')
        if rank == 0:
            reg_cols = "".join(", {}: {:.6f}".format(key, a[7 + i] / cnt) for i, (key, _) in enumerate(regs))
            logging.info("epoch: {:03d}, lr: {:.6f}, loss_pce: {:.6f}, loss_ent: {:.6f}, loss_cr: {:.6f}, loss_aux_cls: {:.6f}, "
                         "loss_memory: {:.6f}{}, {:.2f} s/epoch".format(curr_epoch, new_lr, a[0] / cnt, a[1] / cnt, a[2] / cnt,
                                                                       a[3] / cnt, a[4] / its, reg_cols, epoch_toc - epoch_tic))
            logging.info("throughput: {:.1f} images/sec ({} GPU)".format(n_img * world / max(epoch_toc - epoch_tic, 1e-9), world))
        # --clip_grad_norm: the epoch's gradient-norm statistics (every rank holds the same ones: the norm is taken behind the
        # all-reduce), read behind the sync above; every rank starts them over
        log_clip_stats(optimizer, curr_epoch, scalars if rank == 0 else None, logging.info if rank == 0 else None)

        # ---- validation (train_chaos.py:369-399); model.eval() is never undone, as in the reference
        if world > 1 and model.training and not args.sync_bn:
            parallel.sync_bn_buffers(model)        # per-rank epoch-0 statistics -> one set of running buffers
        model.eval()
        tic = time.time()
        dsc, loss_pce_val = validate()
        toc = time.time()
        avg_all = np.mean([dsc[_] for _ in range(1, args.num_classes)])
        if rank == 0:
            logging.info("val: {:03d}, loss_pce: {:.6f}, time: {:.2f} s/epoch".format(curr_epoch, loss_pce_val, toc - tic))
            logging.info("[" + ", ".join("{}: {:.4f}".format(nm, dsc[i]) for i, nm in enumerate(names))
                         + ", All: {:.4f}]".format(avg_all))
            # the scalar tags of train_chaos.py:362-367 and :416-423 (TensorBoard there; one JSON line per scalar here)
            scalars.add('losses/loss_pce_train', a[0] / cnt, curr_epoch)
            scalars.add('losses/loss_cr', a[2] / cnt, curr_epoch)
            scalars.add('losses/loss_ent', a[1] / cnt, curr_epoch)
            scalars.add('losses/loss_aux_cls', a[3] / cnt, curr_epoch)
            scalars.add('losses/loss_memory', a[4] / its, curr_epoch)
            for i, (key, _) in enumerate(regs):
                scalars.add(f'train/{key}', a[7 + i] / cnt, curr_epoch)
            if unc_on:
                au = acc_unc.cpu().numpy()
                scalars.add('CR/uncertainty_kept', au[0] / its, curr_epoch)
                scalars.add('CR/uncertainty_mean', au[1] / its, curr_epoch)
            scalars.add('lr/current_lr', new_lr, curr_epoch)
            scalars.add('losses/loss_pce_val', loss_pce_val, curr_epoch)
            for i, nm in enumerate(names):
                scalars.add(f'DSC/{nm}', dsc[i], curr_epoch)
            scalars.add('DSC/All', avg_all, curr_epoch)
            scalars.add('DSC/Best', max(best_avg, avg_all), curr_epoch)
        valdice[curr_epoch] = avg_all
        if rank == 0:
            if curr_epoch + 1 == args.epoch or (curr_epoch + 1) % args.ckp_interval == 0:
                torch.save(model.state_dict(), os.path.join(args.child, 'ckps', 'ckp_{:d}.pth'.format(curr_epoch)))
            if avg_all > best_avg:
                best_epoch, best_avg = curr_epoch, avg_all
                best_avg_class = [dsc[_] for _ in range(1, args.num_classes)]
                torch.save(model.state_dict(), args.child + '/best_ckp.pth')
        # ---- --ema_decay: the same validation on the averaged weights, swapped in place for the pass (every rank swaps its own
        # identical slab and scores its share; BatchNorm running statistics stay the live model's), and the EMA checkpoints
        last = curr_epoch + 1 == args.epoch
        ema_val = ema_on and (last or (curr_epoch + 1) % args.ema_val_interval == 0)
        ema_ckp = ema_on and (last or (curr_epoch + 1) % args.ckp_interval == 0)
        if ema_val or ema_ckp:
            with optimizer.ema_weights():
                if ema_val:
                    tic = time.time()
                    dsc_e, loss_e = validate()
                    toc = time.time()
                    avg_e = np.mean([dsc_e[_] for _ in range(1, args.num_classes)])
                    valdice_ema[curr_epoch] = avg_e
                    if rank == 0:
                        logging.info("val_ema: {:03d}, loss_pce: {:.6f}, time: {:.2f} s/epoch".format(curr_epoch, loss_e, toc - tic))
                        logging.info("[" + ", ".join("{}: {:.4f}".format(nm, dsc_e[i]) for i, nm in enumerate(names))
                                     + ", All: {:.4f}] (EMA)".format(avg_e))
                        for i, nm in enumerate(names):
                            scalars.add(f'DSC_EMA/{nm}', dsc_e[i], curr_epoch)
                        scalars.add('DSC_EMA/All', avg_e, curr_epoch)
                        scalars.add('DSC_EMA/Best', max(best_ema['avg'], avg_e), curr_epoch)
                    if avg_e > best_ema['avg']:
                        best_ema = dict(avg=avg_e, epoch=curr_epoch, avg_class=[dsc_e[_] for _ in range(1, args.num_classes)])
                        if rank == 0:
                            torch.save(model.state_dict(), args.child + '/best_ema_ckp.pth')
                if ema_ckp and rank == 0:
                    torch.save(model.state_dict(), os.path.join(args.child, 'ckps', 'ema_ckp_{:d}.pth'.format(curr_epoch)))
        if args.state_interval and ((curr_epoch + 1) % args.state_interval == 0 or curr_epoch + 1 == args.epoch):
            rngs = resume.gather_rng_states(device, augmenter, world)          # every rank's generators (a collective)
            if rank == 0:
                resume.atomic_save(resume.capture(args, curr_epoch, model, optimizer, (best_avg, best_epoch, best_avg_class),
                                                  valdice, rngs, world, ema=(best_ema, valdice_ema) if ema_on else None),
                                   resume.state_path(args.child, curr_epoch))
    if rank == 0:
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


def train_main(argv=None):
    args = apply_dataset_preset(parse_args(argv), argv)
    state_file, resume_state = resume.open_state(parser, args, int(os.environ.get('WORLD_SIZE', '1'))) if args.resume else (None, None)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    rank = int(os.environ.get('RANK', '0'))
    sub = DATASETS.get(args.dataset, DATASETS['chaos'])['split_subdir'].format(modality=args.modality)
    if resume_state is not None:
        args.child = resume.run_dir_of(state_file)          # the run continues in its own directory
    else:
        args.child = os.path.join(os.path.join(args.root, sub) if sub else args.root, args.session,
                                  f'{args.session}-{time.strftime("%H-%M-%S-%m%d")}-fold{args.fold}-{args.tag}')
    if rank == 0:
        if resume_state is not None:
            resume.truncate_scalars(os.path.join(args.child, 'tb_summary', 'scalars.jsonl'), resume_state['epoch'])
        else:
            os.makedirs(args.child, exist_ok=False)
            os.makedirs(os.path.join(args.child, 'ckps'), exist_ok=True)
            os.makedirs(os.path.join(args.child, 'tb_summary'), exist_ok=True)        # train_chaos.py:184-185
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
            train_ls = f.readlines()
        with open(f'{base}/test_fold{args.fold}.txt', 'r') as f:
            val_ls = f.readlines()
        args.train_ls = [(data_root + '/' + p).rstrip('\n') for p in train_ls]
        args.val_ls = [(data_root + '/' + p).rstrip('\n') for p in val_ls]
    return train_interface(args, resume_state)


if __name__ == '__main__':
    train_main()
