"""float64 oracle of the random walker with priors (pacingpseudo_amd/utils/random_walker.py and include/pacingpseudo_rwp.h have the
definition), on top of tests/_rw_reference.py: that module's Laplacian of the unknown pixels plus gamma I, the right-hand sides
plus gamma times this module's own soft-max, factorised directly (splu), one right-hand side per class.  Nothing here is shared
with the kernels."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from tests import _rw_reference as R


def softmax(z):
    """softmax over axis 0 in float64, max-subtracted."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def onehot(lab, K):
    return (np.arange(K)[:, None, None] == np.asarray(lab)[None]).astype(np.float64)


def prior_logits(seed, lab, K):
    """The test prior of phantom `seed`: 3 on the true class plus unit noise."""
    rng = np.random.default_rng(100 + seed)
    return (3.0 * onehot(lab, K) + rng.normal(0, 1, (K,) + np.asarray(lab).shape)).astype(np.float32)


def system(img, scb, logits, K, gamma, beta=13.0, eps=1e-4):
    """(L_UU + gamma I csc, B + gamma q|U (nU, K) dense, unknown mask)."""
    Luu, B, unk = R.system(img, scb, K, beta, eps)
    q = softmax(logits)[:, unk].T                                          # (nU, K)
    return (Luu + gamma * sp.identity(Luu.shape[0], format='csc')).tocsc(), B + gamma * q, unk


def rw_prob(img, scb, logits, K, gamma, beta=13.0, eps=1e-4):
    """prob (K, h, w) float64 of one slice; gamma = 0 is the plain walker (a class without a seed exactly 0)."""
    if gamma == 0:
        return R.rw_prob(img, scb, K, beta, eps)
    scb = np.asarray(scb)
    prob = np.zeros((K,) + scb.shape)
    for k in range(K):
        prob[k][scb == k] = 1.0
    A, B, unk = system(img, scb, logits, K, gamma, beta, eps)
    if unk.any():
        lu = splu(A)
        for k in range(K):
            prob[k][unk] = lu.solve(B[:, k])
    return prob


def relres(img, scb, logits, K, gamma, k, x_plane, beta=13.0, eps=1e-4):
    """||b_k + gamma q_k - (L_UU + gamma I) x|| / ||b_k + gamma q_k|| for x = x_plane (h, w) restricted to the unknown pixels."""
    A, B, unk = system(img, scb, logits, K, gamma, beta, eps)
    x = np.asarray(x_plane, dtype=np.float64)[unk]
    return float(np.linalg.norm(B[:, k] - A @ x) / np.linalg.norm(B[:, k]))


def truncation_error(img, scb, logits, K, gamma, tol=1e-6, max_iters=10000, beta=13.0, eps=1e-4):
    """What the stopping rule leaves on the SHIFTED system: per class, max |x - x*| of the Jacobi-preconditioned conjugate-gradient
    iteration carried out in float64 (x0 = 0, stop at ||r||^2 <= tol^2 ||rhs||^2 on the recurrence residual) against the direct
    solve x*.  A float64 property of the slice: no kernel and no fp32 in it."""
    if gamma == 0:
        return R.truncation_error(img, scb, K, tol, max_iters, beta, eps)
    A, B, unk = system(img, scb, logits, K, gamma, beta, eps)
    out = np.zeros(K)
    if A.shape[0] == 0:
        return out
    d, lu = A.diagonal(), splu(A)
    for k in range(K):
        b = B[:, k]
        bb = float(b @ b)
        if bb == 0.0:
            continue
        x, r = np.zeros_like(b), b.copy()
        p = r / d
        rz = float(r @ p)
        for _ in range(max_iters):
            q = A @ p
            a = rz / float(p @ q)
            x += a * p
            r -= a * q
            if float(r @ r) <= tol * tol * bb:
                break
            z = r / d
            rz_new = float(r @ z)
            p = z + (rz_new / rz) * p
            rz = rz_new
        out[k] = np.abs(x - lu.solve(b)).max()
    return out
