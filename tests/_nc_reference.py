"""Float64 comparison functions for the normalised-cut loss (plain torch, CPU): the definition as a direct double sum over padded,
shifted slices -- differentiated by autograd -- and the gather form the kernels evaluate.

    k_ij  = exp(-(dy^2 + dx^2) / (2 sigma_xy^2)) * exp(-|x_i - x_j|^2 / (2 sigma_rgb^2))     j = i + (dy, dx) * d
    A_nc  = sum_{i in n} sum_j m_i m_j k_ij p_ic p_jc          V_nc = sum_{i in n} sum_j m_i m_j k_ij p_ic
    NC_nc = 1 - A_nc / V_nc if V_nc > 1e-6, else 0             L = (1/D) sum_n sum_c NC_nc,  D = N K
    dy, dx in [-r, r] without (0, 0), j inside the image
"""
import torch
import torch.nn.functional as F

from tests._crf_reference import _shifted, rel, smooth_image  # noqa: F401  (smooth_image and rel are what the tests use)

V_MIN = 1e-6


def _prepare(logits, image, valid_mask, radius, dilation):
    z = logits.double()
    x = image.detach().double()
    N, K, H, W = z.shape
    m = torch.ones(N, 1, H, W, dtype=torch.float64) if valid_mask is None else valid_mask.detach().double().reshape(N, 1, H, W)
    R = radius * dilation
    return z, x, m, R, (R, R, R, R)


def _offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dy or dx]


def nc_assoc_vol(logits, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1):
    """(A, V), each (N, K), term by term; differentiable in `logits` (float64 throughout)."""
    z, x, m, R, pad = _prepare(logits, image, valid_mask, radius, dilation)
    N, K, H, W = z.shape
    p = torch.softmax(z, 1)
    pp, xp, mp = F.pad(p, pad), F.pad(x, pad), F.pad(m, pad)            # zero padding: m_j = 0 outside the image
    A, V = z.new_zeros(N, K), z.new_zeros(N, K)
    for dy, dx in _offsets(radius):
        pj, xj, mj = (_shifted(t, R, dy, dx, dilation, H, W) for t in (pp, xp, mp))
        k = torch.exp(torch.tensor(-(dy * dy + dx * dx) / (2.0 * sigma_xy ** 2), dtype=torch.float64)) \
            * torch.exp(-((x - xj) ** 2).sum(1, keepdim=True) / (2.0 * sigma_rgb ** 2))
        w = m * mj * k
        A = A + (w * p * pj).sum((2, 3))
        V = V + (w * p).sum((2, 3))
    return A, V


def nc_terms(A, V):
    """NC_nc (N, K): 1 - A / V where V > V_MIN, 0 (and no gradient) elsewhere."""
    active = V > V_MIN
    return torch.where(active, 1.0 - A / torch.where(active, V, torch.ones_like(V)), torch.zeros_like(V))


def nc_loss_direct(logits, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, denominator=None):
    """The definition; differentiable in `logits`.  `denominator` replaces D = N K (a rank's share of a data-parallel batch is
    divided by the GLOBAL count)."""
    A, V = nc_assoc_vol(logits, image, valid_mask, radius, dilation, sigma_xy, sigma_rgb)
    return nc_terms(A, V).sum() / (float(A.numel()) if denominator is None else denominator)


def nc_loss_and_grad(logits, image, valid_mask=None, **kw):
    """(loss, d loss / d logits) of the direct form by autograd, float64."""
    z = logits.detach().double().requires_grad_(True)
    loss = nc_loss_direct(z, image, valid_mask, **kw)
    if not loss.requires_grad:                                  # every class inactive: the loss is the constant 0
        return loss.detach(), torch.zeros_like(z)
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), g


def nc_gather_form(logits, image, valid_mask=None, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1):
    """The form the kernels evaluate: q_ic = sum_j m_j k_ij p_jc, d_i = sum_j m_j k_ij, A = sum m p q, V = sum m p d, then
    G_ic = m_i (a_nc q_ic + b_nc d_i) with a = -2 / V, b = A / V^2 (0 for an inactive class) and
    dL/dz_ic = (1/D) p_ic (G_ic - p_i.G_i).  Returns (loss, gradient, A, V), float64, no autograd."""
    with torch.no_grad():
        z, x, m, R, pad = _prepare(logits.detach(), image, valid_mask, radius, dilation)
        N, K, H, W = z.shape
        p = torch.softmax(z, 1)
        pp, xp, mp = F.pad(p, pad), F.pad(x, pad), F.pad(m, pad)
        q = torch.zeros_like(p)
        d = torch.zeros(N, 1, H, W, dtype=torch.float64)
        for dy, dx in _offsets(radius):
            pj, xj, mj = (_shifted(t, R, dy, dx, dilation, H, W) for t in (pp, xp, mp))
            k = mj * torch.exp(-(dy * dy + dx * dx) / (2.0 * sigma_xy ** 2) - ((x - xj) ** 2).sum(1, keepdim=True) / (2.0 * sigma_rgb ** 2))
            d += k
            q += k * pj
        A, V = (m * p * q).sum((2, 3)), (m * p * d).sum((2, 3))
        D = float(N * K)
        loss = nc_terms(A, V).sum() / D
        active = V > V_MIN
        Vs = torch.where(active, V, torch.ones_like(V))
        a = torch.where(active, -2.0 / Vs, torch.zeros_like(V))[:, :, None, None]
        b = torch.where(active, A / (Vs * Vs), torch.zeros_like(V))[:, :, None, None]
        G = m * (a * q + b * d)
        grad = p * (G - (p * G).sum(1, keepdim=True)) / D
        return loss, grad, A, V
