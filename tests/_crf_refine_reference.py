"""Float64 definition of the mean-field CRF refinement (plain torch, CPU), term by term over padded, shifted slices, and the test
inputs the CPU and GPU tests share.

    j = i + (dy, dx) * d,  dy, dx in [-r, r] without (0, 0),  j inside the image (outside: nothing, also not in the normalisers)
    kb_ij = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))
    ks_ij = exp(-(dy^2 + dx^2) / (2 sigma_smooth^2))
    Sb_i = sum_j kb_ij,  Ss_i = sum_j ks_ij,  Q^0 = softmax(logits),  u = log_softmax(logits)
    Q^{t+1}_i = softmax_c(u_ic + w_bilateral (sum_j kb_ij Q^t_jc) / (Sb_i + 1e-6) + w_smooth (sum_j ks_ij Q^t_jc) / (Ss_i + 1e-6))

`dtype=torch.float32` restates the same formulas in single precision: its distance from the float64 result is the yardstick the
GPU tolerance is stated against.
"""
import functools

import torch
import torch.nn.functional as F

from tests._crf_reference import smooth_image

EPS = 1e-6
DEFAULTS = dict(sigma_xy=6.0, sigma_rgb=0.1, sigma_smooth=1.5, w_bilateral=4.0, w_smooth=1.0)
# (N, K, H, W, C, r, d): halo larger than the image, single row / pixel / class, partial and exact tiles, W % 4 != 0, every
# class-chunk regime (<= 8, 9, 17, 32), compile-time (1, 3) and run-time (2, 4) channel counts
CASES = [(2, 5, 37, 53, 1, 5, 1), (1, 5, 64, 96, 1, 5, 1), (2, 2, 5, 3, 1, 8, 2), (1, 17, 33, 64, 3, 3, 2), (1, 32, 16, 70, 1, 2, 4),
         (2, 1, 9, 9, 1, 1, 1), (1, 5, 1, 130, 1, 5, 1), (1, 3, 1, 1, 1, 2, 1), (1, 8, 40, 72, 4, 8, 1), (1, 9, 40, 72, 2, 4, 4)]


def case_id(case):
    return 'N{}K{}_{}x{}_C{}r{}d{}'.format(*case)


def refine_steps(logits, image, iterations=5, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, sigma_smooth=1.5, w_bilateral=4.0,
                 w_smooth=1.0, dtype=torch.float64):
    """[Q^1, ..., Q^iterations], each (N, K, H, W) in `dtype`; no autograd."""
    with torch.no_grad():
        z, x = logits.detach().to(dtype), image.detach().to(dtype)
        N, K, H, W = z.shape
        R = radius * dilation
        pad = (R, R, R, R)
        xp, mp = F.pad(x, pad), F.pad(torch.ones(N, 1, H, W, dtype=dtype), pad)     # zero padding: no neighbour outside the image

        def shifted(t, dy, dx):
            return t[:, :, R + dy * dilation:R + dy * dilation + H, R + dx * dilation:R + dx * dilation + W]
        offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]
        kb, ks = [], []
        for dy, dx in offsets:
            mj, xj = shifted(mp, dy, dx), shifted(xp, dy, dx)
            o = torch.tensor(float(dy * dy + dx * dx), dtype=dtype)
            kb.append(mj * torch.exp(-o / (2.0 * sigma_xy ** 2)) * torch.exp(-((x - xj) ** 2).sum(1, keepdim=True) / (2.0 * sigma_rgb ** 2)))
            ks.append(mj * torch.exp(-o / (2.0 * sigma_smooth ** 2)))
        Sb = sum(kb) if kb else torch.zeros(N, 1, H, W, dtype=dtype)
        Ss = sum(ks) if ks else torch.zeros(N, 1, H, W, dtype=dtype)
        u = torch.log_softmax(z, 1)
        q = torch.softmax(z, 1)
        out = []
        for _ in range(iterations):
            qp = F.pad(q, pad)
            Gb, Gs = torch.zeros_like(q), torch.zeros_like(q)
            for (dy, dx), b, s in zip(offsets, kb, ks):
                qj = shifted(qp, dy, dx)
                Gb += b * qj
                Gs += s * qj
            q = torch.softmax(u + w_bilateral * Gb / (Sb + EPS) + w_smooth * Gs / (Ss + EPS), 1)
            out.append(q)
        return out


def refine(logits, image, iterations=5, **kw):
    """Q^iterations in float64 (or `dtype`)."""
    return refine_steps(logits, image, iterations, **kw)[-1]


def noise_logits(N, K, H, W, seed):
    """Low-resolution noise up-sampled bilinearly, times 3, plus 0.5 * white noise: regions with ragged borders."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(N, K, max(H // 8, 2), max(W // 8, 2), generator=g)
    z = F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True) * 3.0 + 0.5 * torch.randn(N, K, H, W, generator=g)
    return z.contiguous()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(logits, image) of a case of CASES, fp32 on the CPU; the same tensors for every caller."""
    N, K, H, W, C, r, d = case
    seed = 1000 * H + 10 * W + K
    return noise_logits(N, K, H, W, seed), smooth_image(N, C, H, W, seed + 1)


@functools.lru_cache(maxsize=None)
def oracle(case, iterations=5):
    """-> (steps64, err32): the float64 Q^1 .. Q^iterations of the case at the default sigmas and weights, and the largest
    distance of the float32 restatement from them over all steps.  Computed once, shared, never written to."""
    z, x = inputs(case)
    r, d = case[5], case[6]
    s64 = refine_steps(z, x, iterations, r, d, **DEFAULTS)
    s32 = refine_steps(z, x, iterations, r, d, dtype=torch.float32, **DEFAULTS)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(s32, s64))
    return s64, err


def top_two_gap(q):
    """(N, H, W): the difference of the two largest probabilities (the only class's own value for K = 1)."""
    if q.shape[1] == 1:
        return q[:, 0]
    top = q.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]
