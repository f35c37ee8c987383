"""float64 oracle of the random-walker expansion (pacingpseudo_amd/utils/random_walker.py has the definition), written from that
definition: the Laplacian of the unknown pixels is assembled as a scipy sparse matrix and factorised directly (splu), one right-hand
side per seeded class.  Nothing here is shared with the kernels."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu


def normalise(img):
    img = np.asarray(img, dtype=np.float64)
    return (img - img.mean()) / (img.std() + 1e-8)


def edge_weights(img, beta=13.0, eps=1e-4):
    """(w_right (h, w-1), w_down (h-1, w)) of one slice."""
    g = normalise(img)
    return np.exp(-beta * (g[:, 1:] - g[:, :-1]) ** 2) + eps, np.exp(-beta * (g[1:, :] - g[:-1, :]) ** 2) + eps


def system(img, scb, K, beta=13.0, eps=1e-4):
    """(L_UU csc, B (nU, K) dense, unknown mask): column k of B is b_k."""
    img, scb = np.asarray(img), np.asarray(scb)
    h, w = scb.shape
    wr, wd = edge_weights(img, beta, eps)
    idx = np.arange(h * w).reshape(h, w)
    i = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    j = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    v = np.concatenate([wr.ravel(), wd.ravel()])
    A = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(h * w, h * w)).tocsr()
    L = (sp.diags(np.asarray(A.sum(1)).ravel()) - A).tocsr()
    flat = scb.ravel()
    unk = flat == K
    u, s = np.nonzero(unk)[0], np.nonzero(~unk)[0]
    onehot = np.zeros((len(s), K))
    onehot[np.arange(len(s)), flat[s]] = 1.0
    B = -(L[u][:, s] @ onehot) if len(s) and len(u) else np.zeros((len(u), K))
    return L[u][:, u].tocsc(), np.asarray(B), unk.reshape(h, w)


def rw_prob(img, scb, K, beta=13.0, eps=1e-4):
    """prob (K, h, w) float64 of one slice."""
    scb = np.asarray(scb)
    h, w = scb.shape
    prob = np.zeros((K, h, w))
    for k in range(K):
        prob[k][scb == k] = 1.0
    Luu, B, unk = system(img, scb, K, beta, eps)
    seeded = [k for k in range(K) if (scb == k).any()]
    if unk.any() and seeded:
        lu = splu(Luu)
        for k in seeded:
            prob[k][unk] = lu.solve(B[:, k])
    return prob


def rw_labels(prob, scb, K, threshold=0.9):
    scb = np.asarray(scb)
    best, arg = prob.max(0), prob.argmax(0)
    out = np.where(best >= threshold, arg, K)
    return np.where(scb < K, scb, out).astype(np.int64)


def undecided(prob, threshold, margin=1e-3):
    """Pixels whose label a result within `margin` of the oracle may legitimately flip: the maximum lies within `margin` of the
    threshold, or the two largest classes within `margin` of each other."""
    srt = np.sort(prob, axis=0)
    top = srt[-1]
    second = srt[-2] if prob.shape[0] > 1 else np.full_like(top, -np.inf)
    return (np.abs(top - threshold) <= margin) | (top - second <= margin)


def relres(img, scb, K, k, x_plane, beta=13.0, eps=1e-4):
    """||b_k - L_UU x|| / ||b_k|| for x = x_plane (h, w) restricted to the unknown pixels."""
    Luu, B, unk = system(img, scb, K, beta, eps)
    x = np.asarray(x_plane, dtype=np.float64)[unk]
    return float(np.linalg.norm(B[:, k] - Luu @ x) / np.linalg.norm(B[:, k]))


def truncation_error(img, scb, K, tol=1e-6, max_iters=10000, beta=13.0, eps=1e-4):
    """What the definition's OWN stopping rule leaves: per class, max |x - x*| of the Jacobi-preconditioned conjugate-gradient iteration
    carried out in float64 (x0 = 0, stop at ||r||^2 <= tol^2 ||b||^2 on the recurrence residual) against the direct solve x*.  A
    float64 property of the slice: no kernel and no fp32 in it."""
    Luu, B, unk = system(img, scb, K, beta, eps)
    out = np.zeros(K)
    if Luu.shape[0] == 0:
        return out
    d, lu = Luu.diagonal(), splu(Luu)
    for k in range(K):
        b = B[:, k]
        bb = float(b @ b)
        if bb == 0.0:
            continue
        x, r = np.zeros_like(b), b.copy()
        p = r / d
        rz = float(r @ p)
        for _ in range(max_iters):
            q = Luu @ p
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


def phantom(seed, size=32, K=5):
    """(img, lab, scb) of SyntheticPhantoms(1, K, size, seed=seed, raw=True)[0]."""
    from pacingpseudo_amd.data import SyntheticPhantoms
    d = SyntheticPhantoms(1, K, size=size, seed=seed, raw=True)[0]
    return d['img'], d['lab'], d['scb']
