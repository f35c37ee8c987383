"""float64 comparison functions of the Mumford-Shah level-set loss (--do_loss_ms, pp_ms_loss_*) for the tests:
the direct definition differentiated by autograd, the analytic form the kernels evaluate, and the list of pixels whose gradient
hangs on the sign of a difference of a few fp32 ulps.  Plain torch on the CPU; nothing here runs project code.

  p = softmax(z) over K,  S_nc = sum_i m_i p_ic,  mu_ncr = sum_i m_i p_ic x_ir / S_nc if S_nc > 1e-6 (else the class is inactive),
  E_ls = sum_nci m_i p_ic sum_r (x_ir - mu_ncr)^2 [active],  E_tv = sum_nc sum_(i,j) m_i m_j |p_ic - p_jc| over the vertical and
  horizontal neighbour pairs, each once,  L = (E_ls + tv_weight E_tv) / D,  D = N H W, or max(sum m, 1e-8) with a mask."""
import torch

S_MIN = 1e-6


def _softmax(z):
    """softmax over K in float64, evaluated pixel by pixel (classes innermost): pixels with the same logits get the same bits wherever
    they lie -- torch's strided form over dim 1 vectorises across pixels and differs in the last place at the ends of a row, which
    would put a sign where the definition has an exact 0."""
    return torch.softmax(z.double().permute(0, 2, 3, 1).contiguous(), -1).permute(0, 3, 1, 2)


def _mask(z, valid_mask):
    N, K, H, W = z.shape
    return torch.ones(N, 1, H, W, dtype=torch.float64) if valid_mask is None else valid_mask.double()


def ms_stats(z, image, valid_mask=None):
    """S (N,K), mu (N,K,C) (0 for an inactive class) and the active flags (N,K) in float64."""
    p = _softmax(z)
    x, m = image.double(), _mask(z, valid_mask)
    S = (m * p).sum((2, 3))
    X = torch.einsum('nkhw,nchw->nkc', m * p, x)
    active = S > S_MIN
    mu = torch.where(active[..., None], X / S.clamp_min(1e-300)[..., None], torch.zeros_like(X))
    return S, mu, active


def ms_energy_direct(z, image, valid_mask=None, tv_weight=1.0):
    """(E_ls + tv_weight E_tv, D) of the direct definition; differentiable in z (mu is NOT detached)."""
    z = z.double()
    p = _softmax(z)
    x, m = image.double(), _mask(z, valid_mask)
    S, mu, active = ms_stats(z, image, valid_mask)                               # differentiable through p
    e = ((x[:, None] - mu[..., None, None]) ** 2).sum(2)                        # (N,K,H,W)
    E_ls = (m * p * e * active[..., None, None]).sum()
    tv_v = (m[:, :, 1:] * m[:, :, :-1] * (p[:, :, 1:] - p[:, :, :-1]).abs()).sum()
    tv_h = (m[..., 1:] * m[..., :-1] * (p[..., 1:] - p[..., :-1]).abs()).sum()
    D = torch.tensor(float(z.shape[0] * z.shape[2] * z.shape[3]), dtype=torch.float64) if valid_mask is None else m.sum().clamp_min(1e-8)
    return E_ls + tv_weight * (tv_v + tv_h), D


def ms_loss_direct(z, image, valid_mask=None, tv_weight=1.0, denominator=None):
    """The loss of the direct definition; `denominator` replaces D (a data-parallel rank's share of the global loss)."""
    E, D = ms_energy_direct(z, image, valid_mask, tv_weight)
    return E / (D if denominator is None else denominator)


def ms_loss_and_grad(z, image, valid_mask=None, tv_weight=1.0):
    """(loss, dloss/dz) by float64 autograd of the direct definition."""
    zz = z.detach().double().requires_grad_(True)
    loss = ms_loss_direct(zz, image, valid_mask, tv_weight)
    g, = torch.autograd.grad(loss, zz)
    return loss.detach(), g


def ms_analytic_form(z, image, valid_mask=None, tv_weight=1.0):
    """(loss, dloss/dz, unit gradient u, D) of the closed form: g_ic = m_i e_ic [active] + tv_weight t_ic,
    t_ic = sum_{j in 4-neighbours} m_i m_j sign(p_ic - p_jc), u_ic = p_ic (g_ic - <p_i, g_i>), dL/dz = u / D."""
    z = z.detach().double()
    p = _softmax(z)
    x, m = image.double(), _mask(z, valid_mask)
    S, mu, active = ms_stats(z, image, valid_mask)
    e = ((x[:, None] - mu[..., None, None]) ** 2).sum(2) * active[..., None, None]
    t = torch.zeros_like(p)
    sv = m[:, :, 1:] * m[:, :, :-1] * torch.sign(p[:, :, 1:] - p[:, :, :-1])     # pair (lower, upper)
    t[:, :, 1:] += sv
    t[:, :, :-1] -= sv
    sh = m[..., 1:] * m[..., :-1] * torch.sign(p[..., 1:] - p[..., :-1])
    t[..., 1:] += sh
    t[..., :-1] -= sh
    g = m * e + tv_weight * t
    u = p * (g - (p * g).sum(1, keepdim=True))
    E, D = ms_energy_direct(z, image, valid_mask, tv_weight)
    return E / D, u / D, u, D


def ambiguous_pixels(z, valid_mask=None, rel=1e-5):
    """Bool (N,H,W): pixels that touch a neighbour pair with 0 < |p_ic - p_jc| <= rel * max(p_ic, p_jc) in some class -- where fp32
    probabilities may put sign() on the other side (or on 0).  Pairs a mask removes (m_i m_j = 0) do not count."""
    p = _softmax(z.detach())
    m = _mask(z, valid_mask)
    out = torch.zeros(p.shape[0], p.shape[2], p.shape[3], dtype=torch.bool)

    def amb(a, b, w):
        d = (a - b).abs()
        return (((d > 0) & (d <= rel * torch.maximum(a, b))).any(1)) & (w[:, 0] > 0)
    v = amb(p[:, :, 1:], p[:, :, :-1], m[:, :, 1:] * m[:, :, :-1])
    out[:, 1:] |= v
    out[:, :-1] |= v
    h = amb(p[..., 1:], p[..., :-1], m[..., 1:] * m[..., :-1])
    out[..., 1:] |= h
    out[..., :-1] |= h
    return out


def offset_image(N, C, H, W, seed=0):
    """A smooth image plus pixel noise per channel, with a different intensity offset for every image of the batch (so that means
    mixed across images are wrong means) and all intensities positive (a mean has its own value as its scale); float32 values."""
    g = torch.Generator().manual_seed(1000 + seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    img = torch.empty(N, C, H, W, dtype=torch.float64)
    for n in range(N):
        for c in range(C):
            f = torch.rand(4, generator=g, dtype=torch.float64)
            img[n, c] = (0.5 * torch.sin(0.3 * (1 + f[0]) * yy + 6.28 * f[1]) * torch.cos(0.2 * (1 + f[2]) * xx + 6.28 * f[3])
                         + 0.2 * torch.rand(H, W, generator=g, dtype=torch.float64) + 1.0 + 0.7 * n + 0.4 * c)
    return img.float()
