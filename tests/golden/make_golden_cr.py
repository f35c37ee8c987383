"""Capture the reference's own bidirectional_kl_loss (losses/losses.py:118-145) on the CPU into tests/golden/cr_bikl.npz.

Run where a checkout of the reference exists, with PP_REFERENCE naming it:

    PP_REFERENCE=<reference checkout> python tests/golden/make_golden_cr.py

Only numbers are stored: float64 inputs (2, 5, 6, 7) at logit spreads 1 and 60, a (2, 1, 6, 7) mask, and for each of the four
(spread, masked) cases the loss and the gradients with respect to both logit tensors.  tests/test_cr_variants.py requires
tests/_cr_reference.py to reproduce them to 1e-12.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get('PP_REFERENCE')
if not REF or not os.path.isdir(REF):
    sys.exit('set PP_REFERENCE to a checkout of the reference')
sys.path.insert(0, REF)

from losses.losses import bidirectional_kl_loss  # noqa: E402  (the reference's)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cr_bikl.npz')
SHAPE = (2, 5, 6, 7)
SPREADS = (1, 60)


def main():
    g = torch.Generator().manual_seed(20)
    zs0 = torch.randn(SHAPE, generator=g, dtype=torch.float64) * 2
    zw0 = torch.randn(SHAPE, generator=g, dtype=torch.float64) * 2
    mask = (torch.rand((SHAPE[0], 1) + SHAPE[2:], generator=g) > 0.3).double()
    d = {'input': zs0.numpy(), 'target': zw0.numpy(), 'valid_mask': mask.numpy(), 'spreads': np.asarray(SPREADS, dtype=np.float64)}
    for spread in SPREADS:
        for masked in (False, True):
            zs = (zs0 * spread).requires_grad_(True)
            zw = (zw0 * spread).requires_grad_(True)
            loss = bidirectional_kl_loss(zs, zw, mask.clone() if masked else None)
            loss.backward()
            tag = f's{spread}_{"masked" if masked else "unmasked"}'
            d[f'{tag}/loss'] = np.asarray(loss.item(), dtype=np.float64)
            d[f'{tag}/grad_input'] = zs.grad.numpy()
            d[f'{tag}/grad_target'] = zw.grad.numpy()
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
