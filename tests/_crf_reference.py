"""Float64 comparison functions for the gated-CRF loss (plain torch, CPU): the definition as a direct double sum over padded,
shifted slices -- differentiated by autograd -- and the gather form the kernels evaluate.

    k_ij  = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))     j = i + (dy, dx) * d
    L     = (1/D) sum_n sum_i sum_j m_i m_j k_ij (1 - sum_c p_ic p_jc),    dy, dx in [-r, r] without (0, 0), j inside the image
    D     = N H W without a mask, max(sum m, 1e-8) with one
"""
import torch
import torch.nn.functional as F


def _shifted(t, R, dy, dx, d, H, W):
    return t[:, :, R + dy * d:R + dy * d + H, R + dx * d:R + dx * d + W]


def _prepare(logits, image, valid_mask, radius, dilation):
    z = logits.double()
    x = image.detach().double()
    N, K, H, W = z.shape
    m = torch.ones(N, 1, H, W, dtype=torch.float64) if valid_mask is None else valid_mask.detach().double().reshape(N, 1, H, W)
    R = radius * dilation
    pad = (R, R, R, R)
    D = float(N * H * W) if valid_mask is None else max(float(m.sum()), 1e-8)
    return z, x, m, R, pad, D


def crf_loss_direct(logits, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, denominator=None):
    """The definition, term by term; differentiable in `logits` (float64 throughout).  `denominator` replaces D (a rank's share of
    a data-parallel batch is divided by the GLOBAL denominator)."""
    z, x, m, R, pad, D = _prepare(logits, image, valid_mask, radius, dilation)
    N, K, H, W = z.shape
    p = torch.softmax(z, 1)
    pp, xp, mp = F.pad(p, pad), F.pad(x, pad), F.pad(m, pad)            # zero padding: m_j = 0 outside the image
    num = z.new_zeros(())
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            pj, xj, mj = (_shifted(t, R, dy, dx, dilation, H, W) for t in (pp, xp, mp))
            k = torch.exp(torch.tensor(-(dy * dy + dx * dx) / (2.0 * sigma_xy ** 2), dtype=torch.float64)) \
                * torch.exp(-((x - xj) ** 2).sum(1, keepdim=True) / (2.0 * sigma_rgb ** 2))
            num = num + (m * mj * k * (1.0 - (p * pj).sum(1, keepdim=True))).sum()
    return num / (D if denominator is None else denominator)


def crf_loss_and_grad(logits, image, valid_mask=None, **kw):
    """(loss, d loss / d logits) of the direct form by autograd, float64."""
    z = logits.detach().double().requires_grad_(True)
    loss = crf_loss_direct(z, image, valid_mask, **kw)
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), g


def crf_gather_form(logits, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1):
    """The form the kernels evaluate: G_ic = sum_j m_j k_ij p_jc, S_i = sum_j m_j k_ij; pixel i adds m_i (S_i - p_i.G_i) to the
    numerator and dL/dz_ic = -(2/D) m_i p_ic (G_ic - p_i.G_i).  Returns (loss, gradient, S), float64, no autograd."""
    with torch.no_grad():
        z, x, m, R, pad, D = _prepare(logits.detach(), image, valid_mask, radius, dilation)
        N, K, H, W = z.shape
        p = torch.softmax(z, 1)
        pp, xp, mp = F.pad(p, pad), F.pad(x, pad), F.pad(m, pad)
        G = torch.zeros_like(p)
        S = torch.zeros(N, 1, H, W, dtype=torch.float64)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dy == 0 and dx == 0:
                    continue
                pj, xj, mj = (_shifted(t, R, dy, dx, dilation, H, W) for t in (pp, xp, mp))
                k = mj * torch.exp(-(dy * dy + dx * dx) / (2.0 * sigma_xy ** 2) - ((x - xj) ** 2).sum(1, keepdim=True) / (2.0 * sigma_rgb ** 2))
                S += k
                G += k * pj
        pg = (p * G).sum(1, keepdim=True)
        loss = (m * (S - pg)).sum() / D
        grad = -(2.0 / D) * m * p * (G - pg)
        return loss, grad, S


def smooth_image(N, C, H, W, seed, scale=0.15):
    """A piecewise-smooth test image: low-resolution noise up-sampled bilinearly, so that neighbouring intensities differ by
    fractions of sigma_rgb = 0.1 and the bilateral kernel is neither 0 nor 1 everywhere."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(N, C, max(H // 8, 2), max(W // 8, 2), generator=g)
    return (F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True) * scale).contiguous()


def rel(a, b):
    """The `rel` measure of tests/test_gpu_ops.py: max |a - b| / (max |b| + 1e-30)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))
