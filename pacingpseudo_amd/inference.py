"""Post-training evaluation on the GPU: the reference's ``inference.py`` (``main_interface`` :97-194, ``main`` :256-320).

What it does, as the reference: build a bare ``UNet``, load a checkpoint written by either trainer (a ``ConsistencyRegulr``
checkpoint is reduced to its ``backbone.`` entries, :138-146), run the test fold in eval mode, report per-slice / per-class
Dice (:196-215) and 95 % Hausdorff distance in millimetres (:217-237, ``medpy.metric.hd95`` with the data set's pixel
spacing), write ``eval_data.npz`` (``dicearr``, ``hd95arr``: slices x classes, NaN = class absent) and the summary line.

How it differs: slices are evaluated in batches -- soft-max / arg-max, the Dice counts (``pp_dice_counts``) and both
directed surface-distance sets of HD95 (``pp_hd95_surface_distances``) are computed on the GPU for the whole batch, the
per-slice ``.cpu().numpy()`` round trips and medpy's scipy distance transforms are gone.  Like the reference, every slice
is fed at its NATIVE size with MeanStdNorm only (:125-133) -- never cropped or padded, so every pixel is scored; a loader
batch of differently sized slices is split into same-shape groups, and a slice whose size is not a multiple of the encoder
stride is an error here as it is in the reference (its skip concatenation fails).  ``--synthetic N`` evaluates phantom
slices when no data set is on disk."""
from __future__ import annotations

import argparse
import logging
import os
import random
import shutil
import sys
from collections import OrderedDict

import numpy as np
import torch

SPACING = {'acdc': (1.51, 1.51), 'chaost1': (1.62, 1.62), 'chaost2': (1.62, 1.62), 'lvsc': (1.48, 1.48)}   # mm, inference.py:52-57
CLASSES = {'acdc': 4, 'chaost1': 5, 'chaost2': 5, 'lvsc': 2}                                                # :59-64
CROP = {'acdc': 224, 'chaost1': 256, 'chaost2': 256, 'lvsc': 224}

parser = argparse.ArgumentParser(description='evaluate a checkpoint: Dice + HD95 per slice and class (flags of the reference inference.py)')
parser.add_argument('--gpu', type=str, default='1')
parser.add_argument('--seed', type=int, default=1)
parser.add_argument('--root', type=str, default='./outputs', help='outputs go to <root>/<session>/<dataset>/<checkpoint name>/')
parser.add_argument('--session', type=str, default='Inference')
parser.add_argument('--fold', type=int, required=True, help='test fold; must appear as "fold<k>" in --checkpoint_file')
parser.add_argument('--checkpoint_file', type=str, required=True,
                    help='run directory of a training session (ckps/ckp_399.pth, or ckp_39.pth for lvsc, is taken) or a .pth file')
parser.add_argument('--best_ckp', action='store_true', default=False, help='take best_ckp.pth of the run directory instead')
parser.add_argument('--ema', action='store_true', default=False,
                    help='evaluate the averaged weights of a run trained with --ema_decay: ckps/ema_ckp_399.pth (ema_ckp_39.pth for '
                         'lvsc) of the run directory, best_ema_ckp.pth with --best_ckp; the files have the ordinary keys')
parser.add_argument('--dataset', type=str, default='acdc', choices=['acdc', 'chaost1', 'chaost2', 'lvsc'])
parser.add_argument('--num_classes', type=int, default=None,
                    help='segmentation classes incl. background the checkpoint was trained with, 1 .. 32 (default: the --dataset preset)')
parser.add_argument('--num_workers', type=int, default=4)
parser.add_argument('--batch_size', type=int, default=1, help='slices per forward pass (metrics stay per slice)')
parser.add_argument('--input_ch', type=int, default=1)
parser.add_argument('--init_ch', type=int, default=32)
parser.add_argument('--max_ch', type=int, default=512)
parser.add_argument('--output_stride', type=int, default=8, choices=[32, 16, 8])
parser.add_argument('--is_stride_conv', type=bool, default=False)
parser.add_argument('--is_trans_conv', type=bool, default=False)
parser.add_argument('--elab_end_points', type=bool, default=False)
# ---- additions of this implementation
parser.add_argument('--image_size', type=int, default=0, help='size of the --synthetic phantoms (0 = the data set\'s training crop); real slices are evaluated at their native size')
parser.add_argument('--synthetic', type=int, default=0, help='evaluate N phantom slices instead of ./data')
parser.add_argument('--norm_op', type=str, default='batch', choices=['batch', 'group'],
                    help='block normaliser the checkpoint was trained with: batch = nn.BatchNorm2d (the reference); group = nn.GroupNorm(--norm_groups, C): '
                         'per-image statistics, no running state, the same function in train and eval mode (fp32 storage only)')
parser.add_argument('--norm_groups', type=int, default=8, help='channel groups of --norm_op group; must divide every block width')
parser.add_argument('--keep_largest_cc', action='store_true', default=False,
                    help='post-process the arg-max on the device before scoring: of every foreground class keep only the largest connected '
                         'component of each slice (ties: the one holding the lowest row-major pixel), the rest becomes background; '
                         'eval_data.npz gains ncomp and removed')
parser.add_argument('--cc_connectivity', type=int, default=1, choices=[1, 2],
                    help='neighbourhood of --keep_largest_cc: 1 = 4-neighbourhood (what HD95 uses), 2 = 8-neighbourhood')
parser.add_argument('--tta', type=str, default='none', choices=['none', 'flips', 'd4'],
                    help='test-time augmentation: score the mean soft-max over the views of each slice, mapped back on the device '
                         '(flips = identity + the three mirror images, d4 = all eight flips and quarter turns; transposed views of a '
                         'non-square slice run at the swapped size); eval_data.npz gains tta_changed')


def _tolerance_mm(text):
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'{text!r} is not a number')
    if not (np.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f'{text!r}: a finite distance in millimetres, >= 0')
    return value


parser.add_argument('--surface_metrics', action='store_true', default=False,
                    help='score the Hausdorff distance (the reference\'s _compute_hd), the average symmetric surface distance and the '
                         'surface Dice at --nsd_tolerance beside HD95, all four reduced on the device from one pair of surface-distance '
                         'sets per slice and class; eval_data.npz gains hdarr, assdarr and nsdarr')
parser.add_argument('--nsd_tolerance', type=_tolerance_mm, default=2.0, metavar='MM',
                    help='tolerance of the surface Dice of --surface_metrics in millimetres: the share of surface pixels within MM of the other surface')


# mean-field CRF refinement of the (TTA-averaged) soft-max before the arg-max (utils/crf_refine.py); the window and
# the two sigmas of the bilateral kernel carry the training driver's names and defaults (--do_loss_crf)
parser.add_argument('--crf_refine', type=int, default=0, metavar='T',
                    help='refine the probabilities with T mean-field CRF iterations on the device before the arg-max (0 = off; 1 .. 64): '
                         'bilateral (position x image intensity) and smoothness messages over a local window, after --tta and before '
                         '--keep_largest_cc; eval_data.npz gains crf_changed')
parser.add_argument('--crf_radius', type=int, default=5, help='neighbourhood radius r: offsets dy, dx in [-r, r] (1 .. 8)')
parser.add_argument('--crf_dilation', type=int, default=1, help='spacing d of the neighbourhood offsets in pixels (1 .. 4, r * d <= 16)')
parser.add_argument('--crf_sigma_xy', type=float, default=6.0, help='width of the position factor of the bilateral kernel, in offsets')
parser.add_argument('--crf_sigma_rgb', type=float, default=0.1, help='width of its intensity factor, in units of the network input')
parser.add_argument('--crf_sigma_smooth', type=float, default=1.5, help='width of the smoothness kernel, in offsets (an untuned first value)')
parser.add_argument('--crf_w_bilateral', type=float, default=4.0, help='weight of the bilateral message, in logit units (an untuned first value)')
parser.add_argument('--crf_w_smooth', type=float, default=1.0, help='weight of the smoothness message, in logit units (an untuned first value)')


# volume-wise evaluation (utils/volume.py): beside the per-slice scores, which stay what they are, the slices are
# stacked per patient volume, filtered in 3-D and scored as volumes
def _spacing_mm(text):
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'{text!r} is not a number')
    if not (np.isfinite(value) and value > 0.0):
        raise argparse.ArgumentTypeError(f'{text!r}: a finite distance in millimetres, > 0')
    return value


parser.add_argument('--volumes', action='store_true', default=False,
                    help='also score per patient volume: the class maps that leave the --tta / --crf_refine stage are stacked by volume id and '
                         'slice number (--volume_regex), filtered in 3-D with --keep_largest_cc, and scored with Dice and HD95 in 3-D '
                         '(and HD, ASSD, NSD with --surface_metrics); eval_data.npz gains vol_ids, vol_slices, vol_dicearr, vol_hd95arr, ...; '
                         'needs --slice_spacing on real data')
parser.add_argument('--volume_regex', type=str, default=None, metavar='REGEX',
                    help='how a slice\'s file name (without directory and extension) splits into the named groups (?P<volume>...) and '
                         '(?P<slice>digits); default: the trailing run of digits is the slice number, everything before it -- less a '
                         'separating "_", "-" or "slice" -- the volume id')
parser.add_argument('--slice_spacing', type=_spacing_mm, default=None, metavar='MM',
                    help='distance between neighbouring slices in millimetres for --volumes; slice thickness is not in the .npz files, so '
                         'there is no per-data-set default (with --synthetic: the in-plane spacing)')
parser.add_argument('--cc_connectivity_3d', type=int, default=1, choices=[1, 2, 3],
                    help='neighbourhood of the 3-D --keep_largest_cc of --volumes: 1 = 6 neighbours (what the surfaces use), 2 = 18, 3 = 26')
parser.add_argument('--synthetic_depth', type=int, default=0, metavar='D',
                    help='with --synthetic N: the phantom slices are cross-sections of N / D volumes of D slices each (ellipsoids), named '
                         'vol###_slice###; N must be a multiple of D')
# a size threshold and hole filling around --keep_largest_cc (utils/morphology.py): threshold -> keep-largest -> fill
parser.add_argument('--min_component_size', type=int, default=0, metavar='P',
                    help='post-process the arg-max on the device before scoring: components of a foreground class with fewer than P pixels '
                         'of their slice become background (0 = off; neighbourhood: --cc_connectivity); runs before --keep_largest_cc; '
                         'eval_data.npz gains small_removed')
parser.add_argument('--fill_holes', action='store_true', default=False,
                    help='post-process the arg-max on the device before scoring: a background region of a slice that does not reach the '
                         'slice border and touches one single class takes that class (one that touches several classes is left); runs '
                         'after --keep_largest_cc; eval_data.npz gains holes_filled and holes_mixed; with --volumes the stacked maps are '
                         'filled in 3-D')
parser.add_argument('--fill_holes_connectivity', type=int, default=1, choices=[1, 2],
                    help='neighbourhood of --fill_holes: 1 = 4-neighbourhood (scipy.ndimage.binary_fill_holes\' default), 2 = 8-neighbourhood')
parser.add_argument('--min_component_size_3d', type=int, default=0, metavar='V',
                    help='with --volumes: 3-D components of a foreground class with fewer than V voxels become background before the 3-D '
                         '--keep_largest_cc (0 = off; neighbourhood: --cc_connectivity_3d); eval_data.npz gains vol_small_removed')
parser.add_argument('--fill_holes_connectivity_3d', type=int, default=1, choices=[1, 2, 3],
                    help='neighbourhood of the 3-D --fill_holes of --volumes: 1 = 6 neighbours, 2 = 18, 3 = 26')
MORPH_FLAGS = ('min_component_size', 'fill_holes', 'fill_holes_connectivity', 'min_component_size_3d', 'fill_holes_connectivity_3d')
VOLUME_FLAGS = ('volumes', 'volume_regex', 'slice_spacing', 'cc_connectivity_3d', 'synthetic_depth')
CRF_FLAGS = ('crf_refine', 'crf_radius', 'crf_dilation', 'crf_sigma_xy', 'crf_sigma_rgb', 'crf_sigma_smooth', 'crf_w_bilateral', 'crf_w_smooth')


def crf_settings(args):
    """None with --crf_refine 0, else the checked keyword arguments of utils.crf_refine (ValueError / NotImplementedError)."""
    from .utils.crf_refine import check_crf_refine_params
    if getattr(args, 'crf_refine', 0) == 0:
        return None
    return check_crf_refine_params(args.crf_refine, args.crf_radius, args.crf_dilation, args.crf_sigma_xy, args.crf_sigma_rgb,
                                   args.crf_sigma_smooth, args.crf_w_bilateral, args.crf_w_smooth)


def morph_settings(args):
    """The checked values of MORPH_FLAGS as utils.morphology.check_morph_params returns them (ValueError otherwise)."""
    from .utils.morphology import check_morph_params
    return check_morph_params(getattr(args, 'min_component_size', 0), getattr(args, 'fill_holes', False),
                              getattr(args, 'fill_holes_connectivity', 1), getattr(args, 'min_component_size_3d', 0),
                              getattr(args, 'fill_holes_connectivity_3d', 1), volumes=getattr(args, 'volumes', False))


def morph_used(args):
    """Whether any of MORPH_FLAGS differs from its default: only then do they show in the log's argument dump."""
    return any(getattr(args, f, parser.get_default(f)) != parser.get_default(f) for f in MORPH_FLAGS)


def parse_args(argv=None):
    """parser.parse_args plus the checks that span several flags (argparse errors: exit status 2), before anything is built."""
    args = parser.parse_args(argv)
    try:
        crf_settings(args)
    except (ValueError, NotImplementedError) as e:
        parser.error(f'--crf_refine / --crf_radius / --crf_dilation / --crf_sigma_* / --crf_w_*: {e}')
    try:
        morph_settings(args)
    except ValueError as e:
        parser.error(str(e))
    if args.fill_holes_connectivity != 1 and not args.fill_holes:
        parser.error('--fill_holes_connectivity belongs to --fill_holes: pass --fill_holes as well')
    if args.fill_holes_connectivity_3d != 1 and not args.fill_holes:
        parser.error('--fill_holes_connectivity_3d belongs to --fill_holes: pass --fill_holes as well')
    if args.synthetic_depth < 0:
        parser.error(f'--synthetic_depth {args.synthetic_depth}: a number of slices per volume, >= 1')
    if args.synthetic_depth and not args.synthetic:
        parser.error('--synthetic_depth shapes the phantoms of --synthetic N: pass --synthetic as well')
    if args.synthetic_depth and args.synthetic % args.synthetic_depth != 0:
        parser.error(f'--synthetic {args.synthetic} is not a multiple of --synthetic_depth {args.synthetic_depth}: the slices do not stack to whole volumes')
    if args.volumes:
        if args.synthetic and not args.synthetic_depth:
            parser.error('--volumes with --synthetic N needs --synthetic_depth D: the phantoms of --synthetic alone are unrelated slices')
        if not args.synthetic and args.slice_spacing is None:
            parser.error('--volumes needs --slice_spacing MM on real data: slice thickness is not in the .npz files, so there is no per-data-set default')
        if args.volume_regex is not None:
            from .utils.volume import group_volumes
            try:
                group_volumes([], args.volume_regex)
            except ValueError as e:
                parser.error(f'--volume_regex: {e}')
    else:
        given = [f for f in ('volume_regex', 'slice_spacing') if getattr(args, f)] + (['cc_connectivity_3d'] if args.cc_connectivity_3d != 1 else [])
        if given:
            parser.error(f'--{given[0]} belongs to --volumes: pass --volumes as well')
    return args


def load_backbone(model, state_dict):
    """inference.py:138-146: a full-model checkpoint is reduced to its `backbone.` entries."""
    from .models.unet import check_checkpoint_norm
    check_checkpoint_norm(model, state_dict)
    head = [v for k, v in state_dict.items() if k in ('final_conv.weight', 'backbone.final_conv.weight')]
    if head and head[0].shape[0] != model.num_classes:
        raise ValueError(f'the checkpoint\'s head has {head[0].shape[0]} classes, the model was built with {model.num_classes}: '
                         f'pass --num_classes {head[0].shape[0]}')
    try:
        model.load_state_dict(state_dict)
    except RuntimeError:
        stripped = OrderedDict((k.partition('.')[-1], v) for k, v in state_dict.items() if 'backbone' in k)
        model.load_state_dict(stripped)
    return model


def evaluate(model, loader, num_classes, spacing, device, keep_largest_cc=False, cc_connectivity=1, tta='none', extra=None,
             surface_metrics=False, nsd_tolerance=2.0, crf=None, volume_maps=None, min_component_size=0, fill_holes=False,
             fill_holes_connectivity=1):
    """-> (dicearr, hd95arr), both (slices, classes) float32 with NaN where the reference skips a class.  With keep_largest_cc the
    arg-max is filtered on the device first (utils.postprocess.keep_largest_components) and both metrics score the filtered map;
    then -> (dicearr, hd95arr, ncomp, removed): ncomp (slices, classes) int32 = components per class before filtering, removed
    (slices,) int64 = pixels set to background.  With tta 'flips' / 'd4' the probabilities and the class map are the mean over
    the views (utils.tta.tta_predict) wherever the logits and their arg-max are used otherwise; the returned values keep their
    number and meaning, and a dict passed as `extra` receives tta_changed: (slices,) int64 = pixels whose class differs from
    the identity view's arg-max.  With surface_metrics the same hard map is scored by one utils.metrics.batch_surface_metrics call
    per batch instead of batch_hd95: hd95arr is its percentile distance, and `extra` receives hdarr, assdarr and nsdarr (Hausdorff
    distance, average symmetric surface distance, surface Dice at nsd_tolerance mm), each (slices, classes) float32 with NaN as in
    hd95arr.  With crf = a dict of utils.crf_refine's keyword arguments (iterations, radius, ...) the logits -- with tta the log of
    the mean probabilities, clamped at 1e-30 -- are refined against the image before anything else sees them: the refined
    probabilities and their class map take the place of the logits and their arg-max in the filter and in every metric, and `extra`
    receives crf_changed: (slices,) int64 = pixels whose class differs from the unrefined arg-max.  A list passed as `volume_maps`
    receives one (class map, label) pair of uint8 (H, W) device tensors per slice, in data-set order: the hard map that leaves the
    tta / crf stage, BEFORE the 2-D filter, for score_volumes; nothing else changes.  With min_component_size = P > 0 the
    components of a foreground class with fewer than P pixels become background (utils.morphology.remove_small_components,
    cc_connectivity) BEFORE the keep-largest filter, with fill_holes the cavities of one class are closed
    (utils.morphology.fill_holes, fill_holes_connectivity) AFTER it -- threshold, keep-largest, fill -- and every metric scores the
    result.  `removed` stays what the keep-largest stage alone set to background, the number of returned values depends on
    keep_largest_cc alone, and `extra` receives small_removed and holes_filled, (slices, classes) int32 pixel counts, and
    holes_mixed (slices,) int32 = cavities left because they touch several classes."""
    from .data import expand_compact
    from .utils.metrics import batch_dice_counts, batch_hd95, batch_surface_metrics
    from .utils.postprocess import keep_largest_components
    from .utils.tta import tta_ops, tta_predict
    use_tta = len(tta_ops(tta)) > 1
    do_small, do_fill = min_component_size > 0, bool(fill_holes)
    if do_small or do_fill:
        from .utils.morphology import fill_holes as fill_holes_2d
        from .utils.morphology import remove_small_components
    small_rows, filled_rows, mixed_rows = [], [], []
    if crf is not None:
        from .utils.crf_refine import check_crf_refine_params, crf_refine
        crf = check_crf_refine_params(**crf)
    dice_rows, hd_rows, ncomp_rows, removed_rows, changed_rows, crf_rows = [], [], [], [], [], []
    surf_rows = {'hd': [], 'assd': [], 'nsd': []}
    model.eval()
    for groups in loader:
        for batch in (groups if isinstance(groups, list) else [groups]):   # same-shape groups (data.collate_by_shape)
            batch = expand_compact(batch, num_classes, device)          # uint8 class maps -> one-hot planes, on the device
            image, label = batch['image'], batch['label']
            with torch.no_grad():
                if use_tta:
                    single = []                                            # the arg-max of the identity view, which runs first

                    def forward(x):
                        z = model(x)['segmentation/logits']
                        if not single:
                            single.append(z.argmax(1))
                        return z
                    logits, tta_cls = tta_predict(forward, image, tta)      # mean probabilities and their first-maximum arg-max
                    changed_rows.extend((tta_cls != single[0]).flatten(1).sum(1).tolist())
                else:
                    logits = model(image)['segmentation/logits']
                if crf is not None:
                    before = tta_cls if use_tta else logits.argmax(1)
                    logits, crf_cls = crf_refine(logits.clamp_min(1e-30).log() if use_tta else logits, image, **crf)
                    crf_rows.extend((crf_cls != before).flatten(1).sum(1).tolist())
            # the first-maximum arg-max the last stage left beside its probabilities; None: logits.argmax(1), taken where it is needed
            argmax = crf_cls if crf is not None else (tta_cls if use_tta else None)
            if volume_maps is not None:
                unfiltered = (argmax if argmax is not None else logits.argmax(1)).to(torch.uint8)
                volume_maps.extend(zip(unfiltered.unbind(0), label.argmax(1).to(torch.uint8).unbind(0)))
            filtered = keep_largest_cc or do_small or do_fill
            if filtered:
                raw = argmax if argmax is not None else logits.argmax(1)
                if do_small:                                               # threshold -> keep-largest -> fill
                    raw, stats = remove_small_components(raw, num_classes, min_component_size, cc_connectivity, return_stats=True)
                    small_rows.extend(stats[..., 1].tolist())
                pred = raw
                if keep_largest_cc:
                    pred, stats = keep_largest_components(raw, num_classes, cc_connectivity, return_stats=True)
                    ncomp_rows.extend(stats[..., 0].tolist())
                    removed_rows.extend((pred != raw).flatten(1).sum(1).tolist())
                if do_fill:
                    pred, stats = fill_holes_2d(pred, num_classes, fill_holes_connectivity, return_stats=True)
                    filled_rows.extend(stats[..., 1].tolist())
                    mixed_rows.extend(stats[:, 0, 0].tolist())
                # the counting kernel takes an arg-max itself: the arg-max of a one-hot map is the map, exactly
                scores = torch.nn.functional.one_hot(pred, num_classes).permute(0, 3, 1, 2)
            else:
                scores = logits
            c = batch_dice_counts(scores, label)                           # |P & T|, |P|, |T| per (slice, class), one launch
            inter, ps, ts = c[..., 0], c[..., 1], c[..., 2]
            with np.errstate(invalid='ignore', divide='ignore'):
                dice = 2.0 * inter / np.maximum(ps + ts, 1e-8)             # inference.py:211-213 (no smoothing term here)
            dice[(ps == 0) & (ts == 0)] = np.nan                           # :208-209
            dice_rows.extend(dice.tolist())
            hard = pred if filtered else (argmax if argmax is not None else logits.argmax(1))
            if surface_metrics:
                sm = batch_surface_metrics(hard, label.argmax(1), num_classes, spacing, tolerance=nsd_tolerance)
                hd_rows.extend(sm['hdp'].tolist())
                for key, rows in surf_rows.items():
                    rows.extend(sm[key].tolist())
            else:
                hd_rows.extend(batch_hd95(hard, label.argmax(1), num_classes, spacing).tolist())
    if use_tta and extra is not None:
        extra['tta_changed'] = np.array(changed_rows, np.int64)
    if crf is not None and extra is not None:
        extra['crf_changed'] = np.array(crf_rows, np.int64)
    if surface_metrics and extra is not None:
        for key, rows in surf_rows.items():
            extra[key + 'arr'] = np.array(rows, np.float32).reshape(-1, num_classes)
    if do_small and extra is not None:
        extra['small_removed'] = np.array(small_rows, np.int32).reshape(-1, num_classes)
    if do_fill and extra is not None:
        extra['holes_filled'] = np.array(filled_rows, np.int32).reshape(-1, num_classes)
        extra['holes_mixed'] = np.array(mixed_rows, np.int32)
    if keep_largest_cc:
        return (np.array(dice_rows, np.float32), np.array(hd_rows, np.float32),
                np.array(ncomp_rows, np.int32).reshape(-1, num_classes), np.array(removed_rows, np.int64))
    return np.array(dice_rows, np.float32), np.array(hd_rows, np.float32)


def score_volumes(volume_maps, groups, num_classes, spacing, keep_largest_cc=False, connectivity=1, surface_metrics=False,
                  nsd_tolerance=2.0, min_component_size=0, fill_holes=False, fill_holes_connectivity=1):
    """The per-volume half of --volumes.  volume_maps: evaluate's list of (class map, label) per slice; groups: utils.group_volumes'
    {volume id: slice indices in slice order}; spacing (sz, sy, sx) in mm.  Per volume the slices are stacked on the device, filtered
    in 3-D (keep_largest_cc) and scored.  -> dict of the vol_* arrays of eval_data.npz: vol_ids, vol_slices, vol_dicearr, vol_hd95arr
    (volumes, K) float32 with NaN as in the slice arrays; with surface_metrics vol_hdarr, vol_assdarr, vol_nsdarr; with
    keep_largest_cc vol_ncomp, vol_removed (volumes, K) int32 = components per class before filtering, voxels set to background.
    With min_component_size = V > 0 the 3-D components of a foreground class with fewer than V voxels go first (connectivity), with
    fill_holes the 3-D cavities of one class are closed last (fill_holes_connectivity): vol_small_removed, vol_holes_filled
    (volumes, K) int32 voxel counts and vol_holes_mixed (volumes,) int32 = cavities left because they touch several classes."""
    from .utils.volume import keep_largest_components_3d, volume_dice, volume_surface_metrics
    rows = {'dice': [], 'hdp': [], 'hd': [], 'assd': [], 'nsd': [], 'ncomp': [], 'removed': [], 'small': [], 'filled': [], 'mixed': []}
    if min_component_size > 0 or fill_holes:
        from .utils.morphology import fill_holes_3d, remove_small_components_3d
    out = {}
    for vid, idx in groups.items():
        shapes = {tuple(volume_maps[i][0].shape) for i in idx}
        if len(shapes) != 1:
            raise ValueError(f'volume {vid!r}: its {len(idx)} slices have different shapes {sorted(shapes)}; they do not stack')
        raw = torch.stack([volume_maps[i][0] for i in idx])
        lab = torch.stack([volume_maps[i][1] for i in idx])
        pred = raw.to(torch.int64)
        if min_component_size > 0:                                        # threshold -> keep-largest -> fill, as in evaluate
            pred, stats = remove_small_components_3d(pred, num_classes, min_component_size, connectivity, return_stats=True)
            rows['small'].append(stats[:, 1].cpu().numpy())
        if keep_largest_cc:
            pred, stats = keep_largest_components_3d(pred, num_classes, connectivity, return_stats=True)
            stats = stats.cpu().numpy()
            rows['ncomp'].append(stats[:, 0])
            rows['removed'].append(stats[:, 1])
        if fill_holes:
            pred, stats = fill_holes_3d(pred, num_classes, fill_holes_connectivity, return_stats=True)
            stats = stats.cpu().numpy()
            rows['filled'].append(stats[:, 1])
            rows['mixed'].append(stats[0, 0])
        rows['dice'].append(volume_dice(pred, lab, num_classes))
        sm = volume_surface_metrics(pred, lab, num_classes, spacing, tolerance=nsd_tolerance)
        for key in ('hdp', 'hd', 'assd', 'nsd'):
            rows[key].append(sm[key])
    out['vol_ids'] = np.array(list(groups))
    out['vol_slices'] = np.array([len(idx) for idx in groups.values()], np.int64)
    out['vol_dicearr'] = np.array(rows['dice'], np.float32).reshape(-1, num_classes)
    out['vol_hd95arr'] = np.array(rows['hdp'], np.float32).reshape(-1, num_classes)
    if surface_metrics:
        for key in ('hd', 'assd', 'nsd'):
            out[f'vol_{key}arr'] = np.array(rows[key], np.float32).reshape(-1, num_classes)
    if keep_largest_cc:
        out['vol_ncomp'] = np.array(rows['ncomp'], np.int32).reshape(-1, num_classes)
        out['vol_removed'] = np.array(rows['removed'], np.int32).reshape(-1, num_classes)
    if min_component_size > 0:
        out['vol_small_removed'] = np.array(rows['small'], np.int32).reshape(-1, num_classes)
    if fill_holes:
        out['vol_holes_filled'] = np.array(rows['filled'], np.int32).reshape(-1, num_classes)
        out['vol_holes_mixed'] = np.array(rows['mixed'], np.int32)
    return out


def _foreground_mean(arr, num_classes):
    """The slice line's rule on any (items, classes) array: per class the mean of its values that are not NaN (0 for a class without
    one: AvgMeter.avg of an empty meter), then the mean over the foreground classes."""
    means = []
    for cls in range(1, num_classes):
        col = arr[:, cls]
        col = col[~np.isnan(col)]
        means.append(float(np.mean(col.astype(np.float64))) if col.size else 0.0)
    return np.mean(means)


def _volume_scores(args, volume_maps, groups, num_classes, spacing):
    m = morph_settings(args)
    morph = {}                                             # without the flags the score_volumes call is the parent's
    if m['min_component_size_3d']:
        morph['min_component_size'] = m['min_component_size_3d']
    if m['fill_holes']:
        morph.update(fill_holes=True, fill_holes_connectivity=m['fill_holes_connectivity_3d'])
    return score_volumes(volume_maps, groups, num_classes, spacing, keep_largest_cc=args.keep_largest_cc,
                         connectivity=args.cc_connectivity_3d, surface_metrics=getattr(args, 'surface_metrics', False),
                         nsd_tolerance=args.nsd_tolerance, **morph)


def main_interface(args):
    from .data import NpzSlices, SyntheticPhantoms, collate_by_shape, loader_context
    from .models import UNet
    from .models.unet import norm_kwargs
    from .utils import AvgMeter
    num_classes = args.num_classes if args.num_classes is not None else CLASSES[args.dataset]
    spacing = SPACING[args.dataset]
    size = args.image_size or CROP[args.dataset]          # only the size of --synthetic phantoms; real slices keep theirs
    logging.info(f'Number of classes: {num_classes}')
    logging.info(f'Spacing: {spacing}')
    device = torch.device('cuda', 0)
    model = UNet(input_ch=args.input_ch, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=num_classes,
                 output_stride=args.output_stride, is_stride_conv=args.is_stride_conv, is_trans_conv=args.is_trans_conv,
                 elab_end_points=args.elab_end_points, **norm_kwargs(args)).to(device)
    volumes = getattr(args, 'volumes', False)
    if args.synthetic and getattr(args, 'synthetic_depth', 0):
        from .data import SyntheticVolumes
        test_dataset = SyntheticVolumes(args.synthetic, num_classes, args.synthetic_depth, size=size, train=False, seed=args.seed)
    elif args.synthetic:
        test_dataset = SyntheticPhantoms(args.synthetic, num_classes, size=size, train=False, seed=args.seed, native=True, compact=True)
    else:
        test_dataset = NpzSlices(args.test_ls, num_classes, size=size, train=False, seed=args.seed, native=True, compact=True)
    loader = torch.utils.data.DataLoader(test_dataset, batch_size=args.batch_size, shuffle=False,
                                         num_workers=args.num_workers, drop_last=False, collate_fn=collate_by_shape,
                                         multiprocessing_context=loader_context(args.num_workers))
    logging.info('Length {}'.format(len(loader)))
    load_backbone(model, torch.load(args.checkpoint_file, map_location=device))
    tta = getattr(args, 'tta', 'none')
    extra = {}                                             # tta_changed with --tta flips / d4, hdarr / assdarr / nsdarr with --surface_metrics, crf_changed with --crf_refine
    surface = dict(surface_metrics=True, nsd_tolerance=args.nsd_tolerance) if getattr(args, 'surface_metrics', False) else {}
    crf = crf_settings(args)
    refine = dict(crf=crf) if crf is not None else {}      # without the flag the evaluate call is the parent's
    morph = morph_settings(args)
    if morph['min_component_size']:
        refine['min_component_size'] = morph['min_component_size']
    if morph['fill_holes']:
        refine.update(fill_holes=True, fill_holes_connectivity=morph['fill_holes_connectivity'])
    if volumes:                                            # the grouping first: a file name that does not fit fails before the model runs
        from .utils.volume import group_volumes
        names = test_dataset.names if args.synthetic else [os.path.splitext(os.path.basename(f))[0] for f in args.test_ls]
        groups = group_volumes(names, args.volume_regex)
        slice_spacing = args.slice_spacing if args.slice_spacing is not None else spacing[0]
        volume_maps = []
        refine['volume_maps'] = volume_maps
        logging.info('Volumes: {} of {} slices, spacing (z, y, x) = {} mm'.format(len(groups), len(names), (slice_spacing,) + tuple(spacing)))
    if args.keep_largest_cc:
        dicearr, hd95arr, ncomp, removed = evaluate(model, loader, num_classes, spacing, device, True, args.cc_connectivity, tta, extra, **surface,
                                                    **refine)
        vol = _volume_scores(args, volume_maps, groups, num_classes, (slice_spacing,) + tuple(spacing)) if volumes else {}
        np.savez(os.path.join(args.child, 'eval_data'), dicearr=dicearr, hd95arr=hd95arr, ncomp=ncomp, removed=removed, **extra, **vol)
        logging.info('Largest-component filter (connectivity {}): {} pixels set to background, {} of {} slices changed'.format(
            args.cc_connectivity, int(removed.sum()), int((removed > 0).sum()), len(removed)))
    else:
        dicearr, hd95arr = evaluate(model, loader, num_classes, spacing, device, tta=tta, extra=extra, **surface, **refine)
        vol = _volume_scores(args, volume_maps, groups, num_classes, (slice_spacing,) + tuple(spacing)) if volumes else {}
        np.savez(os.path.join(args.child, 'eval_data'), dicearr=dicearr, hd95arr=hd95arr, **extra, **vol)
    if morph['min_component_size']:
        small = extra['small_removed']
        logging.info('Size threshold ({} pixels, connectivity {}): {} pixels set to background, {} of {} slices changed'.format(
            morph['min_component_size'], args.cc_connectivity, int(small.sum()), int((small.sum(1) > 0).sum()), len(small)))
    if morph['fill_holes']:
        filled = extra['holes_filled']
        logging.info('Hole filling (connectivity {}): {} pixels filled, {} of {} slices changed, {} cavities between several classes left'.format(
            morph['fill_holes_connectivity'], int(filled.sum()), int((filled.sum(1) > 0).sum()), len(filled), int(extra['holes_mixed'].sum())))
    if tta != 'none':
        from .utils.tta import tta_ops
        changed = extra['tta_changed']
        logging.info('Test-time augmentation ({}, {} views): {} pixels differ from the identity view, {} of {} slices changed'.format(
            tta, len(tta_ops(tta)), int(changed.sum()), int((changed > 0).sum()), len(changed)))
    if crf is not None:
        changed = extra['crf_changed']
        logging.info('CRF refinement ({} iterations, radius {} x dilation {}): {} pixels differ from the unrefined arg-max, {} of {} slices changed'.format(
            crf['iterations'], crf['radius'], crf['dilation'], int(changed.sum()), int((changed > 0).sum()), len(changed)))
    meter_dice = [AvgMeter() for _ in range(num_classes)]
    meter_hd95 = [AvgMeter() for _ in range(num_classes)]
    for drow, hrow in zip(dicearr, hd95arr):
        for cls in range(num_classes):
            if not np.isnan(drow[cls]):
                meter_dice[cls].update(float(drow[cls]))
            if not np.isnan(hrow[cls]):
                meter_hd95[cls].update(float(hrow[cls]))
    logging.info('Dataset: {}'.format(args.dataset))
    logging.info('Number of clases: {}'.format(num_classes))
    foldavgdice = np.mean([meter_dice[_].avg for _ in range(1, num_classes)])
    foldavghd95 = np.mean([meter_hd95[_].avg for _ in range(1, num_classes)])
    logging.info('Fold {}, overall Dice: {:.4f}, overall HD95: {:.2f}'.format(args.fold, foldavgdice, foldavghd95))
    if surface:
        means = []
        for key in ('hdarr', 'assdarr', 'nsdarr'):
            meters = [AvgMeter() for _ in range(num_classes)]
            for row in extra[key]:
                for cls in range(num_classes):
                    if not np.isnan(row[cls]):
                        meters[cls].update(float(row[cls]))
            means.append(np.mean([meters[_].avg for _ in range(1, num_classes)]))
        logging.info('Fold {}, overall HD: {:.2f}, overall ASSD: {:.2f}, overall NSD at {:g} mm: {:.4f}'.format(
            args.fold, means[0], means[1], args.nsd_tolerance, means[2]))
    if volumes:
        line = 'Fold {}, overall volume Dice: {:.4f}, overall volume HD95: {:.2f}'.format(
            args.fold, _foreground_mean(vol['vol_dicearr'], num_classes), _foreground_mean(vol['vol_hd95arr'], num_classes))
        if surface:
            line += ', overall volume HD: {:.2f}, overall volume ASSD: {:.2f}, overall volume NSD at {:g} mm: {:.4f}'.format(
                _foreground_mean(vol['vol_hdarr'], num_classes), _foreground_mean(vol['vol_assdarr'], num_classes), args.nsd_tolerance,
                _foreground_mean(vol['vol_nsdarr'], num_classes))
        logging.info(line)
        if args.keep_largest_cc:
            logging.info('Largest-component filter in 3-D (connectivity {}): {} voxels set to background in {} volumes'.format(
                args.cc_connectivity_3d, int(vol['vol_removed'].sum()), len(groups)))
        if morph['min_component_size_3d']:
            logging.info('Size threshold in 3-D ({} voxels, connectivity {}): {} voxels set to background in {} volumes'.format(
                morph['min_component_size_3d'], args.cc_connectivity_3d, int(vol['vol_small_removed'].sum()), len(groups)))
        if morph['fill_holes']:
            logging.info('Hole filling in 3-D (connectivity {}): {} voxels filled in {} volumes, {} cavities between several classes left'.format(
                morph['fill_holes_connectivity_3d'], int(vol['vol_holes_filled'].sum()), len(groups), int(vol['vol_holes_mixed'].sum())))
    logging.info('Shape of the Dice array: {}'.format(dicearr.shape))
    logging.info('Shape of the HD95 array: {}'.format(hd95arr.shape))
    return dicearr, hd95arr


def main(argv=None):
    args = parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    assert f'fold{args.fold}' in args.checkpoint_file, 'the checkpoint must come from the same fold (inference.py:264)'
    args.child = os.path.join(args.root, args.session, args.dataset, os.path.basename(args.checkpoint_file.rstrip('/')))
    os.makedirs(args.child, exist_ok=True)
    if os.path.isdir(args.checkpoint_file):                    # a run directory: pick the file the reference picks (:274-284)
        run = args.checkpoint_file
        pre = 'ema_' if args.ema else ''
        if args.best_ckp:
            cand = [os.path.join(run, 'ckps', f'best_{pre}ckp.pth'), os.path.join(run, f'best_{pre}ckp.pth')]
        else:
            cand = [os.path.join(run, 'ckps', pre + ('ckp_39.pth' if args.dataset == 'lvsc' else 'ckp_399.pth'))]
        found = [c for c in cand if os.path.isfile(c)]
        if not found:
            raise FileNotFoundError(f'none of {cand} exists')
        args.checkpoint_file = found[0]
    if os.path.isfile(sys.argv[0]):
        shutil.copy(sys.argv[0], os.path.join(args.child, os.path.basename(sys.argv[0])))
    log = logging.getLogger()
    log.setLevel(logging.INFO)
    for h in list(log.handlers):
        log.removeHandler(h)
    fh = logging.FileHandler(args.child + '/log.txt', mode='w')
    fh.setFormatter(logging.Formatter('[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S'))
    log.addHandler(fh)
    log.addHandler(logging.StreamHandler(sys.stdout))
    # without --surface_metrics the log is what it was before the flag existed: its two entries are left out of the dump
    shown = [(k, v) for k, v in args._get_kwargs() if (args.surface_metrics or k not in ('surface_metrics', 'nsd_tolerance'))
             and (args.crf_refine or k not in CRF_FLAGS)         # the same for --crf_refine and its eight entries
             and (args.volumes or args.synthetic_depth or k not in VOLUME_FLAGS)       # ... and for --volumes and its companions
             and (morph_used(args) or k not in MORPH_FLAGS)]     # ... and for the size threshold and hole filling
    logging.info(''.join(f'{k}={v}\n' for k, v in shown))
    if not args.synthetic:
        from .train import split_dir                              # the same table the trainers read their fold lists from
        ds, mod = {'acdc': ('acdc', ''), 'lvsc': ('lvsc', ''), 'chaost1': ('chaos', 't1'), 'chaost2': ('chaos', 't2')}[args.dataset]
        data_root, base = split_dir(ds, mod)
        with open(f'{base}/test_fold{args.fold}.txt', 'r') as f:
            args.test_ls = [(data_root + '/' + p).rstrip('\n') for p in f.readlines()]
    return main_interface(args)


if __name__ == '__main__':
    main()
