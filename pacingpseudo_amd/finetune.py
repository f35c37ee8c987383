"""Fine-tuning: start a run from the weights of another one, optionally with a frozen encoder prefix.

``--init_from PATH [--init_reset_head]`` copies a checkpoint of either driver (``ckp_*.pth`` / ``best_ckp.pth`` / ``ema_ckp_*.pth``:
the bare U-Net's ``state_dict()`` or the full model's, ``backbone.`` / ``aux_path.`` keys) into a freshly built model of either
kind; ``--freeze_encoder N`` then holds ``enc_block1 .. enc_block<N>`` fixed (``UNet.freeze_encoder``).  Pre-train the upper
bound on dense labels and adapt with scribbles, or go from CHAOS T1 to T2 with the low encoder stages kept.  Unlike ``--resume``
(pacingpseudo_amd/resume.py) nothing but weights and buffers is taken over: optimizer state, schedules and the epoch count start
afresh.  ``inference.load_backbone`` stays the loader for evaluation; it refuses what this one adapts.
"""
from __future__ import annotations

import os

import torch

from .models.unet import check_checkpoint_norm

# the tensors whose shape depends on the class count K: 1x1 head, auxiliary classifier, class-prototype bank
HEAD_KEYS = ('backbone.final_conv.weight', 'backbone.final_conv.bias', 'aux_path.fc_cls.1.weight', 'aux_path.memory_bank')


def add_flags(parser) -> None:
    parser.add_argument('--freeze_encoder', type=int, default=0, choices=list(range(7)), metavar='N',
                        help='hold encoder stages 1 .. N (0 .. 6) fixed: constant weights, BatchNorm from the running statistics, and '
                             'no backward launches for them (the backward walk stops in front of stage N); 0 trains everything')
    parser.add_argument('--init_from', type=str, default=None, metavar='PATH',
                        help='initialise the model from this checkpoint (ckp_*.pth / best_ckp.pth / ema_ckp_*.pth of either driver) '
                             'before training; optimizer state and schedules start afresh (--resume continues a run instead and wins)')
    parser.add_argument('--init_reset_head', action='store_true',
                        help='with --init_from: keep the fresh initialisation of every tensor whose shape depends on --num_classes '
                             '(1x1 head, auxiliary classifier, memory bank), so a checkpoint of another class count can be used')


def load_pretrained(model, state_dict, reset_head: bool = False):
    """Copy `state_dict` into `model` in place (slab views and engine pointers stay valid; packed weights are forgotten by the
    models' ``load_state_dict`` hooks).  Either checkpoint layout goes into either model kind: a bare ``UNet`` checkpoint
    fills the backbone of a ``ConsistencyRegulr`` and leaves its auxiliary path at the fresh initialisation; the ``aux_path.``
    entries of a full-model checkpoint are dropped for a bare ``UNet``.

    Refused (ValueError): the other block normaliser (as ``check_checkpoint_norm``), a head of another class count unless
    `reset_head` (the message names ``--init_reset_head``), any other shape difference, backbone entries the model lacks or
    misses.  With `reset_head` the head, the auxiliary classifier and the memory bank keep their fresh values.

    Returns (loaded, reset, absent): lists of the model's keys taken from the checkpoint, kept fresh on purpose, and not in
    the checkpoint."""
    check_checkpoint_norm(model, state_dict)
    full_model = hasattr(model, 'backbone')
    full_ckpt = any(k.startswith(('backbone.', 'aux_path.')) for k in state_dict)
    src = {k if full_ckpt else 'backbone.' + k: v for k, v in state_dict.items()}        # keyed like the full model
    own = model.state_dict()
    want = {k if full_model else 'backbone.' + k: (k, v) for k, v in own.items()}          # full-model key -> (own key, tensor)
    unknown = sorted(k for k in src if k not in want and (full_model or not k.startswith('aux_path.')))
    if unknown:
        raise ValueError(f'the checkpoint holds entries this model does not have (another U-Net variant or width?): {unknown[:4]}'
                         + (' ...' if len(unknown) > 4 else ''))
    loaded, reset, absent, take = [], [], [], {}
    for fk, (k, t) in want.items():
        if fk not in src:
            if fk.startswith('backbone.') and not (reset_head and fk in HEAD_KEYS):
                raise ValueError(f'the checkpoint lacks {fk}: the whole backbone must come from it')
            (reset if (reset_head and fk in HEAD_KEYS) else absent).append(k)
            continue
        if fk in HEAD_KEYS:
            if reset_head:
                reset.append(k)
                continue
            if tuple(src[fk].shape) != tuple(t.shape):
                raise ValueError(f'{fk}: the checkpoint was trained with {src[fk].shape[0]} classes, the model is built for '
                                 f'{t.shape[0]}; pass --init_reset_head to keep the head, the auxiliary classifier and the '
                                 'memory bank at their fresh initialisation')
        elif tuple(src[fk].shape) != tuple(t.shape):
            raise ValueError(f'{fk}: shape {tuple(src[fk].shape)} in the checkpoint, {tuple(t.shape)} in the model '
                             '(--init_ch / --max_ch / --input_ch / --hid_ch must match the checkpoint)')
        take[k] = src[fk]
        loaded.append(k)
    model.load_state_dict(take, strict=False)
    return loaded, reset, absent


def init_model(args, model, parser, log=None) -> None:
    """The drivers' call, after ``.cuda()`` and before the optimizer, EMA and ``parallel.attach``: --init_from (ignored under
    --resume, whose state file holds the weights), then --freeze_encoder.  A checkpoint that does not fit is a usage error of
    `parser` (exit status 2).  `log`: rank 0's logging function."""
    say = log or (lambda *_: None)
    path = getattr(args, 'init_from', None)
    if path and getattr(args, 'resume', None):
        say(f'--init_from {path} ignored: --resume takes the weights from the state file')
    elif path:
        try:
            if not os.path.isfile(path):
                raise ValueError(f'no such checkpoint file: {path}')
            try:
                sd = torch.load(path, map_location='cpu', weights_only=True)
            except Exception as e:                  # truncated / not a torch file / foreign pickle
                raise ValueError(f'{path} is not a readable checkpoint ({type(e).__name__})') from None
            if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
                raise ValueError(f'{path} is not a model checkpoint (a state_dict of tensors)')
            loaded, reset, absent = load_pretrained(model, sd, reset_head=bool(getattr(args, 'init_reset_head', False)))
        except ValueError as e:
            parser.error(f'--init_from: {e}')
        say(f'initialised from {path}: {len(loaded)} tensors loaded, {len(reset)} kept fresh (--init_reset_head): {reset}, '
            f'{len(absent)} not in the checkpoint: {absent}')
    n = int(getattr(args, 'freeze_encoder', 0) or 0)
    if n:
        model.freeze_encoder(n)
        bb = getattr(model, 'backbone', model)
        held = sum(p.numel() for k in range(1, n + 1) for p in getattr(bb, f'enc_block{k}').parameters())
        say(f'--freeze_encoder {n}: encoder stages 1 .. {n} are fixed ({held} parameter values outside the optimizer, eval-mode norms)')
