"""Float64 reference of the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1) on the CPU, written from the paper
and the definition in include/pacingpseudo_lov.h.  Every function takes the errors AND an order, so a caller can hand it any order
(the device's own, or torch's stable sort of any set of errors).

A segment: errors e (n,), fg (n,) in {0, 1}, `order` a permutation of the segment's VALID slots, by e descending.  Along the order,
with G = sum fg and c_i the running sum of fg (1-based i): J_i = 1 - (G - c_i) / (G + i - c_i), g_i = J_i - J_{i-1}, J_0 = 0."""
import itertools

import numpy as np
import torch


def stable_order(e):
    """torch's stable descending order of a 1-D tensor (ties in ascending index)."""
    return torch.sort(torch.as_tensor(e), descending=True, stable=True).indices


def jaccard_increments(fg_sorted):
    """g (float64) along the order from the integer counts; for G = 0: J_i = 1 for every i, so g = (1, 0, 0, ...)."""
    fg = np.asarray(fg_sorted, dtype=np.float64)
    n = fg.shape[0]
    if n == 0:
        return np.zeros(0)
    G = fg.sum()
    c = np.cumsum(fg)
    i = np.arange(1, n + 1, dtype=np.float64)
    J = 1.0 - (G - c) / (G + i - c)
    g = J.copy()
    g[1:] = J[1:] - J[:-1]
    return g


def jaccard_set_function(fg, M):
    """Delta(M) = 1 - (|G| - |M n G|) / (|G| + |M \\ G|): the Jaccard loss when exactly the pixels of M are mispredicted."""
    fg = np.asarray(fg).astype(bool)
    inM = np.zeros(fg.shape[0], dtype=bool)
    inM[list(M)] = True
    G = int(fg.sum())
    union = G + int((inM & ~fg).sum())
    if union == 0:
        return 0.0
    return 1.0 - (G - int((inM & fg).sum())) / union


def segment_loss(e, fg, order):
    """(loss, g in ORIGINAL slot order (0 outside `order`)) of one segment; e a float64 torch tensor (differentiable), fg 0/1."""
    order = torch.as_tensor(order, dtype=torch.long)
    g_sorted = torch.from_numpy(jaccard_increments(np.asarray(fg)[order.numpy()]))
    g = torch.zeros(e.shape[0], dtype=torch.float64)
    g[order] = g_sorted
    return (e[order] * g_sorted).sum(), g


def valid_mask(target, K, ignore_index=None):
    t = torch.as_tensor(target)
    v = (t >= 0) & (t < K)
    if ignore_index is not None:
        v &= t != ignore_index
    return v


def errors(logits, target, ignore_index=None):
    """e (K, N*H*W) float64 (differentiable in logits), fg (K, N*H*W) bool, valid (N*H*W,) bool."""
    N, K, H, W = logits.shape
    p = torch.softmax(logits.double(), dim=1).permute(1, 0, 2, 3).reshape(K, -1)
    t = torch.as_tensor(target).reshape(-1)
    valid = valid_mask(t, K, ignore_index)
    fg = (t[None, :] == torch.arange(K)[:, None]) & valid[None, :]
    return (fg.double() - p).abs(), fg, valid


def loss(logits, target, ignore_index=None, per_image=False, classes='present', orders=None, sort_errors=None):
    """(loss, g (K, N*H*W) float64 in pixel order, perm: per segment the flattened pixel indices in sorted order, ignored last).
    The order of a segment is orders[seg] (flattened pixel indices of the valid pixels) when given, else torch's stable descending
    sort of sort_errors (K, N*H*W) -- default: the float64 errors themselves -- over the segment's valid pixels."""
    N, K, H, W = logits.shape
    e, fg, valid = errors(logits, target, ignore_index)
    P = N * H * W
    key = e.detach() if sort_errors is None else torch.as_tensor(sort_errors)
    g_all = torch.zeros(K, P, dtype=torch.float64)
    images = [torch.arange(n * H * W, (n + 1) * H * W) for n in range(N)] if per_image else [torch.arange(P)]
    total, perms = torch.zeros((), dtype=torch.float64), []
    for im, pix in enumerate(images):
        vp, ip = pix[valid[pix]], pix[~valid[pix]]
        acc, cnt = torch.zeros((), dtype=torch.float64), 0
        for c in range(K):
            seg = im * K + c
            order = vp[stable_order(key[c, vp])] if orders is None else torch.as_tensor(orders[seg], dtype=torch.long)
            perms.append(torch.cat([order, ip]))
            fgc = fg[c].numpy()
            val, g = segment_loss(e[c], fgc, order)
            g_all[c] += g
            if classes == 'all' or fgc[pix.numpy()].any():
                acc, cnt = acc + val, cnt + 1
        if cnt:
            total = total + acc / cnt
    return total / len(images), g_all, perms


def brute_force_increments(fg_sorted):
    """g_i as differences of the set function on the prefixes of the order."""
    n = len(fg_sorted)
    vals = [jaccard_set_function(fg_sorted, range(i)) for i in range(n + 1)]
    return np.diff(np.asarray(vals))


def all_tie_orders(e):
    """Every order that sorts e descending (permutations within groups of equal values); small n only."""
    e = np.asarray(e)
    groups = [list(np.nonzero(e == v)[0]) for v in sorted(set(e.tolist()), reverse=True)]
    for combo in itertools.product(*[itertools.permutations(g) for g in groups]):
        yield [i for grp in combo for i in grp]
