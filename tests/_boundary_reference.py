"""float64 reference of the boundary loss (libpacingpseudo_dist.so): scipy's exact Euclidean distance transform, the signed level-set
maps built from it, and the loss with its gradient in float64 torch.  No GPU.

Two stated deviations from scipy / Kervadec's one_hot2dist, written out below where they apply:
  1. a plane without any zero pixel: scipy.ndimage.distance_transform_edt returns meaningless values there, `edt` returns +inf;
  2. a class that fills the whole image: one_hot2dist would return -(edt(pos) - 1) with that meaningless edt, `signed_maps` returns
     0 everywhere (no boundary, no force) -- as it does, like one_hot2dist, for a class that is absent."""
import numpy as np
import torch
from scipy import ndimage


def edt(mask, spacing=(1.0, 1.0), squared=False):
    """(..., H, W) -> float64: per plane distance_transform_edt(mask, sampling=spacing); +inf in a plane without a zero pixel."""
    mask = np.asarray(mask) != 0
    flat = mask.reshape((-1,) + mask.shape[-2:])
    out = np.empty(flat.shape, dtype=np.float64)
    for p, m in enumerate(flat):
        if m.all():
            out[p] = np.inf                                  # deviation 1
        else:
            out[p] = ndimage.distance_transform_edt(m, sampling=tuple(float(s) for s in spacing))
    out = out.reshape(mask.shape)
    return out * out if squared else out


def edt_squared_int(mask):
    """Unit spacing: the squared distances as exact integers (from the nearest-zero indices scipy returns), -1 where there is none."""
    mask = np.asarray(mask) != 0
    flat = mask.reshape((-1,) + mask.shape[-2:])
    out = np.empty(flat.shape, dtype=np.int64)
    yy, xx = np.indices(flat.shape[1:])
    for p, m in enumerate(flat):
        if m.all():
            out[p] = -1
        else:
            iy, ix = ndimage.distance_transform_edt(m, return_distances=False, return_indices=True)
            out[p] = (iy - yy) ** 2 + (ix - xx) ** 2
    return out.reshape(mask.shape)


def brute_edt(mask, spacing=(1.0, 1.0)):
    """(H, W): the distance to the nearest zero pixel by search over all pairs (the check of the reference itself)."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    zy, zx = np.nonzero(~mask)
    if len(zy) == 0:
        return np.full((H, W), np.inf)
    yy, xx = np.indices((H, W))
    d2 = ((yy[..., None] - zy) * float(spacing[0])) ** 2 + ((xx[..., None] - zx) * float(spacing[1])) ** 2
    return np.where(mask, np.sqrt(d2.min(-1)), 0.0)


def signed_maps(class_map, K, spacing=(1.0, 1.0)):
    """(N, H, W) integers -> phi float64 (N, K, H, W).  A value outside [0, K) is outside every class."""
    class_map = np.asarray(class_map)
    N, H, W = class_map.shape
    off = float(min(spacing))
    phi = np.zeros((N, K, H, W), dtype=np.float64)
    for n in range(N):
        for k in range(K):
            pos = class_map[n] == k
            if not pos.any():                                # absent class: 0, as in one_hot2dist
                continue
            if pos.all():                                    # deviation 2
                continue
            neg = ~pos
            phi[n, k] = edt(neg, spacing) * neg - (edt(pos, spacing) - off) * pos
    return phi


def foreground(K):
    return [0] if K == 1 else list(range(1, K))


def loss(z, phi):
    """z, phi: float64 torch (N, K, H, W); mean over n, k in I, x of softmax_k(z) phi_k."""
    idx = foreground(z.shape[1])
    p = torch.softmax(z, dim=1)
    return (p[:, idx] * phi[:, idx]).mean()


def loss_and_grad(z, phi, upstream=1.0):
    """-> (loss float, d(upstream * loss)/dz float64 numpy) for fp32 or fp64 inputs (numpy or torch)."""
    zt = torch.as_tensor(np.asarray(z), dtype=torch.float64).clone().requires_grad_(True)
    pt = torch.as_tensor(np.asarray(phi), dtype=torch.float64)
    val = loss(zt, pt)
    (val * upstream).backward()
    return float(val.detach()), zt.grad.numpy()
