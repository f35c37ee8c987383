"""float64 reference of a training step with a frozen encoder prefix (``freeze_encoder(n)``), composed of the oracle's own public
functions: the stage loop of ``O.unet_forward`` with ``training=False`` for the stages k <= n, ``O.aux_forward`` and the oracle's
loss functions as ``O.consistency_forward`` assembles them.  Host code only; tests/test_gpu_freeze.py compares the device with it.

What "frozen" means here is what the engine implements: a frozen stage normalises with its running statistics and leaves
``running_mean`` / ``running_var`` / ``num_batches_tracked`` alone whatever the mode of the rest; its parameters receive no
gradient.  Everything behind the prefix is the oracle's ordinary step.  The oracle's branch alignment (``O.MASKS`` / ``O.POOLS``) is
honoured because the layers are evaluated through ``O.double_conv`` / ``O.max_pool_choice`` under their usual prefixes.
"""
import torch
import torch.nn.functional as F

from oracle import pacing_oracle as O


def frozen_prefixes(n):
    return tuple(f'backbone.enc_block{k}.' for k in range(1, n + 1))


def to_double(sd):
    """The state in float64 (integer buffers as they are)."""
    return {k: (v.detach().double().clone() if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}


def unet_forward(sd, x, args, training, frozen):
    """O.unet_forward (max-pool / bilinear and strided / transposed variants) with per-stage BatchNorm mode."""
    plan = O.stage_plan(args)
    enc = []
    h = x
    for k, e in enumerate(plan['enc'], start=1):
        if e['pool']:
            h = O.max_pool_choice(h, f'backbone.enc_block{k}.pooling')
        h = O.double_conv(sd, f'backbone.enc_block{k}.conv_block', h, e['dil'], bool(training and k > frozen), e['stride'])
        enc.append(h)
    d = enc[5]
    decs = {}
    for k in (5, 4, 3, 2, 1):
        up = plan['dec'][k]['up']
        if plan['dec'][k]['trans']:
            u = F.conv_transpose2d(d, sd[f'backbone.dec_block{k}.up_samp.weight'], None, up)
        else:
            u = F.interpolate(d, scale_factor=up, mode='bilinear', align_corners=True)
        d = O.double_conv(sd, f'backbone.dec_block{k}.conv_block', torch.cat((u, enc[k - 1]), 1), 1, training)
        decs[k] = d
    ep = {f'encoder/stage{k}': enc[k - 1] for k in range(1, 7)}
    ep.update({f'decoder/stage{k}': decs[k] for k in (5, 4, 3, 2, 1)})
    ep['segmentation/logits'] = F.conv2d(d, sd['backbone.final_conv.weight'], sd['backbone.final_conv.bias'])
    return ep


def consistency_forward(sd, batch, step, args, training, frozen):
    """O.consistency_forward in 'train' mode over the per-stage forward above (same order of the two backbone passes, the
    auxiliary path on the last one)."""
    out = {}
    ep = unet_forward(sd, batch['image'], args, training, frozen)
    lw = ep['segmentation/logits']
    out['segmentation/logits'] = lw
    out['loss_pce'] = O.partial_cross_entropy_loss(lw, batch['scribble'].argmax(1).long(), args.ignored_index)
    vm = batch.get('valid_mask')
    if args.do_loss_ent:
        out['loss_ent'] = O.entropy_minimization_loss(lw, vm)
    if args.do_decoder_consistency:
        assert args.loss_cr_variants == 'ce_loss' and not args.detach_weak_cr
        ep = unet_forward(sd, batch['image_strong'], args, training, frozen)
        ls = ep['segmentation/logits']
        out['loss_cr'] = O.soft_label_cross_entropy_loss(ls, torch.softmax(lw, 1), vm)
        out['segmentation/logits_strong'] = ls
    if args.do_aux_path:
        aux = O.aux_forward(sd, ep, batch['scribble'], step, args, training)
        out['logits_aux_cls'] = aux['logits_aux_cls']
        out['loss_aux_cls'] = O.partial_cross_entropy_loss(aux['logits_aux_cls'], aux['aux_targets'], args.ignored_index)
        if args.do_memory:
            out['loss_memory'] = O.cross_entropy_loss(aux['logits_memory'].squeeze(-1).squeeze(-1), aux['memory_target'])
    return out


def train_step(sd, batch, epoch, args, training, frozen):
    """One iteration in float64 on `sd` (float32 or float64 tensors; converted, `sd` itself is left alone).  Returns
    (outputs, {key: gradient} of the trainable keys OUTSIDE the frozen prefix, total loss, the state after the forward -- the
    BatchNorm buffers and the memory bank as the step left them)."""
    sd = to_double(sd)
    batch = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    O._CALLS.clear()
    del O.MASK_STATS[:]
    del O.POOL_STATS[:]
    skip = frozen_prefixes(frozen)
    keys = [k for k in O.trainable_keys(sd) if not (skip and k.startswith(skip))]
    for k in keys:
        sd[k].requires_grad_(True)
    out = consistency_forward(sd, batch, epoch, args, training, frozen)
    total = sum(out[name] * wt for name, wt in O.loss_weights(args, epoch).items())
    total.backward()
    grads = {k: (sd[k].grad.detach().clone() if sd[k].grad is not None else None) for k in keys}
    for k in keys:
        sd[k].requires_grad_(False)
        sd[k].grad = None
    return {k: v.detach() for k, v in out.items()}, grads, float(total.detach()), {k: v.detach() for k, v in sd.items()}
