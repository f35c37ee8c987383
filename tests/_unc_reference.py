"""Pure numpy float64 reference of the uncertainty mask (include/pacingpseudo_unc.h, pacingpseudo_amd/utils/uncertainty.py):
Philox-4x32-10, the uniform mapping, the Box-Muller pairing, the clamped noise, the mean soft-max over the passes, its entropy, the
mask, the threshold schedule and the three statistics.  Integer arithmetic is exact (uint64 products); everything else is float64."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 ints.  Returns 4 uint64 arrays holding the 32-bit outputs."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _LO for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        n0 = (p1 >> _S32) ^ c[1] ^ np.uint64(k0)
        n1 = p1 & _LO
        n2 = (p0 >> _S32) ^ c[3] ^ np.uint64(k1)
        n3 = p0 & _LO
        c = [n0, n1, n2, n3]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(r):
    """u = ((r >> 8) + 0.5) * 2^-24, in (0, 1)."""
    return ((np.asarray(r, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(n, seed, step, pass_index):
    """n_i for i in [0, n): N(0,1) values of (seed, step, pass) by element index, float64."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    quads = (int(n) + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    r = philox4x32_10((q, int(pass_index), step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    u = [uniforms(v) for v in r]
    out = np.empty((quads, 4), dtype=np.float64)
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(u[2 * h]))
        ang = 2.0 * math.pi * u[2 * h + 1]
        out[:, 2 * h] = rad * np.cos(ang)
        out[:, 2 * h + 1] = rad * np.sin(ang)
    return out.reshape(-1)[:int(n)]


def noise(n, sigma, clip, seed, step, pass_index):
    """clamp(sigma * n_i, -clip, +clip), float64."""
    return np.clip(float(sigma) * normals(n, seed, step, pass_index), -float(clip), float(clip))


def add_noise(image, sigma, clip, seed, step, pass_index):
    x = np.asarray(image, dtype=np.float64)
    return x + noise(x.size, sigma, clip, seed, step, pass_index).reshape(x.shape)


def softmax(z, axis=1):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def mean_softmax(logits_list):
    """(N, K, ...) mean over the passes, summed in the order given."""
    acc = None
    for z in logits_list:
        p = softmax(z, 1)
        acc = p if acc is None else acc + p
    return acc / len(logits_list)


def entropy(pbar):
    """-sum_k p ln p over axis 1; a term with p = 0 contributes 0."""
    p = np.asarray(pbar, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    return -t.sum(axis=1)


def mask(u, threshold, valid_mask=None):
    m = (np.asarray(u) < float(threshold)).astype(np.float64)
    if valid_mask is not None:
        m = m * np.asarray(valid_mask, dtype=np.float64).reshape(m.shape)
    return m


def stats(u, m, valid_mask=None):
    """(sum of the mask, sum of u over valid pixels, number of valid pixels)."""
    v = np.ones_like(u) if valid_mask is None else np.asarray(valid_mask, dtype=np.float64).reshape(u.shape)
    return np.array([m.sum(), (v * u).sum(), v.sum()], dtype=np.float64)


def gaussian_ramp_up(t, base_value, max_t=80, scale=5.0):
    return base_value * math.exp(-scale * (1 - t / max_t)) if t < max_t else base_value


def threshold(epoch, start, num_classes, scale=5.0):
    s = float(start)
    return (s + (1.0 - s) * gaussian_ramp_up(epoch, 1.0, scale=scale)) * math.log(num_classes)


def band_fraction(u, theta, tol):
    """Share of pixels whose reference entropy lies within `tol` of the threshold (their mask bit is not compared)."""
    return float((np.abs(np.asarray(u) - float(theta)) <= tol).mean())
