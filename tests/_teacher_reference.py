"""Float64 reference of the mean-teacher consistency term (--cr_teacher ema): the seven forms of --loss_cr_variants with the
TEACHER's logits as a constant target -- autograd runs through the student only -- and the teacher's forward, the oracle's U-Net in
eval mode under a state dict that holds the averaged parameters.

The four forms of the reference are the oracle's own functions, called as oracle.pacing_oracle.consistency_forward calls them;
the three additions are those of tests/_cr_reference.py.  Signature as the functional API: (student logits, teacher logits,
variant, valid_mask), all (N, K, H, W) / (N, 1, H, W) float64.
"""
import torch

from oracle import pacing_oracle as O
from tests import _cr_reference as R

VARIANTS = ['ce_loss', 'l1_loss', 'l2_loss', 'kl_loss', 'bikl_loss', 'js_loss', 'hard_ce_loss']


def teacher_consistency(student_logits, teacher_logits, variant='ce_loss', valid_mask=None):
    zt = teacher_logits.detach()
    q = torch.softmax(zt, 1)
    if variant == 'ce_loss':
        return O.soft_label_cross_entropy_loss(student_logits, q, valid_mask)
    if variant == 'l1_loss':
        return O.l1_loss(torch.softmax(student_logits, 1), q, valid_mask)
    if variant == 'l2_loss':
        return O.l2_loss(torch.softmax(student_logits, 1), q, valid_mask)
    if variant == 'kl_loss':
        return O.kl_loss(student_logits, zt, valid_mask)
    return R.BY_NAME[variant](student_logits, zt, valid_mask)


def teacher_logits(sd, ema_sd, image, args):
    """The teacher's prediction in float64: the oracle's U-Net in eval mode on `image` with the parameters of `ema_sd` and every
    buffer (BatchNorm running statistics) of the live state `sd`."""
    mixed = {k: (ema_sd[k] if (k in ema_sd and not _is_buffer(k)) else v).double() for k, v in sd.items()}
    with torch.no_grad():
        return O.unet_forward(mixed, image.double(), args, training=False)['segmentation/logits']


def _is_buffer(key):
    return key.endswith(('running_mean', 'running_var', 'num_batches_tracked', 'memory_bank'))


def train_step(sd, batch, epoch, args, training, teacher, variant):
    """oracle.train_step with the consistency term student-strong against the constant `teacher` logits: the oracle is given
    'kl_loss' -- the form that hands both LOGIT tensors to its loss -- and its kl_loss is replaced for the call by the form
    `variant` against the teacher (the weak logits it is handed are ignored: they get no consistency gradient)."""
    import copy
    oargs = copy.copy(args)
    oargs.loss_cr_variants = 'kl_loss'
    zt = teacher.double()
    real = O.kl_loss
    O.kl_loss = lambda a, b, m=None: teacher_consistency(a, zt, variant, m)
    try:
        return O.train_step(sd, batch, epoch, oargs, training)
    finally:
        O.kl_loss = real
