"""Float64 references, the shared case table and the comparison functions for the input-side kernels: the augmentation entry
points of pacingpseudo_amd/csrc/pp_augment.hip and the scribble-synthesis kernels at the end of pp_spatial.hip.

tests/test_gpu_input_kernels.py feeds the kernels' outputs to the comparators below; tests/test_input_kernels.py (CPU) feeds
them reference outputs with one planted mistake each and requires that they fail, measures how far the project's own fp32
restatement (oracle/augment_oracle.py: warp) lies from the float64 definition, and checks the references against scipy.

References:
  * Gaussian filters: scipy.ndimage.gaussian_filter in float64 (truncate 4, 'reflect': what the kernel restates);
  * dilation: scipy.ndimage.binary_dilation(seed, anti-diagonal, iterations, mask); end points: a neighbour count with
    scipy.ndimage.convolve; skeleton: oracle.pacing_oracle.skeletonize_zhang -- skimage (the reference's implementation) is
    NOT installed, so the oracle's restatement of Zhang-Suen thinning is the only yardstick there;
  * spline resampling: scipy.ndimage.map_coordinates(order=3, mode='nearest') on the float64 slice, directly;
  * Keys bicubic / bilinear / nearest warp: warp64 below, the definition of aug_warp_kernel evaluated in float64 from the 12 map
    floats, returning mag = sum |w_y w_x s| beside the value;
  * Philox / Box-Muller: oracle.augment_oracle, with normal_sample() generating one chosen sample without the others.

Why the warp is decidable at every pixel: the case table uses only maps whose six coefficients (and displacement fields whose
values) are multiples of 2^-6 on output grids below 2^12 pixels per side.  Every product and partial sum of a yo + b xo + c is
then a multiple of 2^-6 below 2^14, exact in fp32 and in float64, contracted or not; coordinates, floor(), the fractional parts
and the nearest-neighbour decision (ties at exactly .5 included: floor(c + 0.5), up) are identical on both sides.  warp64 refuses
anything else (exact_or_raise)."""
import functools
import os
import re

import numpy as np
import scipy.ndimage

from oracle import augment_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = 2.0 ** -24                    # half an ulp of 1.0f: one fp32 rounding, relative

# ------------------------------------------------------------------------------------------ launch geometry, from the source
AUG_SOURCE = os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_augment.hip')


@functools.lru_cache(None)
def grid_caps():
    """{entry point: (largest grid in blocks, threads per block)} read from pp_augment.hip: the `if (blocks > N) blocks = N;` of
    each extern "C" function and AUG_THREADS.  A loop-shape test asserts total > cap * threads with these numbers."""
    src = open(AUG_SOURCE).read()
    threads = int(re.search(r'#define\s+AUG_THREADS\s+(\d+)', src).group(1))
    caps = {}
    parts = re.split(r'extern "C" int (pp_aug_\w+)\(', src)
    for name, body in zip(parts[1::2], parts[2::2]):
        m = re.search(r'if \(blocks > (\d+)\) blocks = \1;', body)
        if m:
            caps[name] = (int(m.group(1)), threads)
    return caps


def loop_threads(entry):
    cap, threads = grid_caps()[entry]
    return cap * threads


# ------------------------------------------------------------------------------------------ the warp case table
HP, WP, HO, WO = 12, 16, 9, 11          # source planes, output grid
K = 5                                   # classes; lab_pad = K
IMG_PAD = -3.0
SENT_IMG, SENT_LAB = np.float32(1.0e6), 99          # plane memory outside a slice: any read of it shows
SLICES = ((12, 16), (5, 7), (2, 3), (1, 1))
RECTS = ((0, 0, HO, WO), (2, 3, 4, 5), (4, 2, 0, 6), (8, 0, 1, WO))      # full, strictly inside, empty (ph = 0), one row
MAPS = np.array([
    [1, 0, 0, 0, 1, 0],                                     # 1 identity
    [1, 0, 0.5, 0, 1, -0.25],                               # 2 shift: every row coordinate is a tie
    [2, 0, 0.5, 0, 2, 0.5],                                 # 3 x2 with pixel-centre offsets
    [0.5, 0, -0.25, 0, 0.5, -0.25],                         # 4 x1/2
    [0, -1, 8, 1, 0, -2],                                   # 5 quarter turn
    [1, 0.25, -3, -0.25, 1, 2.5],                           # 6 shear
    [0.75, 0, -0.125, 0, 1.25, 0.375],                      # 7 anisotropic
    [0.125, 0, -0.4375, 0, 0.125, -0.4375],                 # 8 1/8 scale (also the loop test's map)
], np.float64)


def planes(sizes, seed, Hp=HP, Wp=WP, sentinel=True):
    """(img, lab, scb) planes of B = len(sizes) ragged slices.  Image: 80 +- 30 with a step of 2000 at the slice's middle column
    (the Keys kernel overshoots a step by up to 10 %, more than the noise, so a [min, max] clamp engages), negated for odd samples (so the lower clamp engages too);
    everything outside the slice holds the sentinel."""
    rng = np.random.RandomState(seed)
    B = len(sizes)
    yy, xx = np.mgrid[0:Hp, 0:Wp]
    img = (rng.normal(size=(B, Hp, Wp)) * 30 + 80).astype(np.float32)
    lab = np.stack([(yy + 2 * xx + n) % K for n in range(B)]).astype(np.int32)
    scb = np.stack([np.where((3 * yy + xx + n) % 4 == 0, lab[n], K) for n in range(B)]).astype(np.int32)
    for n, (h, w) in enumerate(sizes):
        if w >= 2:
            img[n, :, w // 2:] += 2000
        if n % 2:
            img[n] = -img[n]
        if sentinel:
            for a, s in ((img, SENT_IMG), (lab, SENT_LAB), (scb, SENT_LAB)):
                a[n, h:, :] = s
                a[n, :, w:] = s
    return img, lab, scb


def map_row(coef6, rect, size):
    return np.array(list(coef6) + list(rect) + list(size), np.float32)


def warp_launch(s, r):
    """Launch (s, r) of the case table, B = 8: sample n resamples through map n + 1 a slice of size SLICES[(n + s) % 4] into the
    canvas rectangle RECTS[(n + n // 4 + r) % 4]; s, r in 0..3 run every map over every slice size and every rectangle."""
    sizes = [SLICES[(n + s) % 4] for n in range(8)]
    rects = [RECTS[(n + n // 4 + r) % 4] for n in range(8)]
    img, lab, scb = planes(sizes, 100 + 4 * s + r)
    maps = np.stack([map_row(MAPS[n], rects[n], sizes[n]) for n in range(8)])
    return dict(img=img, lab=lab, scb=scb, maps=maps, sizes=sizes, rects=rects)


def slice_clip(img, sizes):
    """[B][4] double statistics rows whose [2] / [3] are the slice's own min / max: narrower than the bicubic overshoot."""
    st = np.zeros((len(sizes), 4), np.float64)
    for n, (h, w) in enumerate(sizes):
        st[n, 2], st[n, 3] = img[n, :h, :w].min(), img[n, :h, :w].max()
    return st


def wide_clip(B):
    st = np.zeros((B, 4), np.float64)
    st[:, 2], st[:, 3] = -1.0e5, 1.0e5
    return st


def dyadic_disp(B, Ho, Wo, seed):
    """[B][2][Ho][Wo] displacement field, multiples of 1/4 with magnitude up to 3."""
    return (np.random.RandomState(seed).randint(-12, 13, size=(B, 2, Ho, Wo)) / 4.0).astype(np.float32)


def disp_launch():
    """The displacement case, B = 8 on the Keys path: identity, shift, shear and anisotropic maps over a slice smaller than the
    output (so points inside are pushed past all four edges and points outside are pushed in) and over the full plane."""
    which = [0, 0, 1, 1, 5, 5, 6, 6]
    sizes = [(5, 7), (12, 16), (5, 7), (2, 3), (5, 7), (12, 16), (5, 7), (1, 1)]
    rects = [RECTS[0]] * 6 + [RECTS[1], RECTS[0]]
    img, lab, scb = planes(sizes, 777)
    maps = np.stack([map_row(MAPS[which[n]], rects[n], sizes[n]) for n in range(8)])
    return dict(img=img, lab=lab, scb=scb, maps=maps, sizes=sizes, rects=rects, disp=dyadic_disp(8, HO, WO, 778))


def exact_or_raise(m6, disp, Ho, Wo):
    ok = Ho < 4096 and Wo < 4096 and (np.asarray(m6) * 64 == np.round(np.asarray(m6) * 64)).all() and np.abs(m6).max() <= 8
    if disp is not None:
        ok = ok and (np.asarray(disp, np.float64) * 64 == np.round(np.asarray(disp, np.float64) * 64)).all() and np.abs(disp).max() <= 8
    if not ok:
        raise ValueError('warp64: coordinates of this map are not exact in fp32; the comparison would not be decidable')


def keys_weights64(t):
    a = -0.75
    w0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w1 = ((a + 2) * t - (a + 3)) * t * t + 1
    u = 1 - t
    w2 = ((a + 2) * u - (a + 3)) * u * u + 1
    return [w0, w1, w2, 1 - w0 - w1 - w2]


def warp64(img, lab, scb, m, Ho, Wo, disp=None, clip=None, img_pad=0.0, lab_pad=4, cubic=1, mistake=None):
    """aug_warp_kernel's definition for one sample in float64 (pp_augment.hip, "the one resampling kernel").  img / lab / scb:
    (Hp, Wp) planes, lab / scb may be None; m: the 12 map floats.  Returns a dict: v (float64, NOT rounded to fp32), mag =
    sum |w_y w_x s| over the taps (padding taps included), lab, scb, valid, in_src, n_in (taps inside the slice), pre (v before
    the clamp and the padding), ys / xs.  `mistake` plants one (CPU tests): 'shift' -- the border test of a tap is off by one at
    the bottom / right edge, so the tap reads plane memory one pixel outside the slice; 'replicate' -- a tap outside the slice
    reads the clamped border pixel instead of the padding; 'tie_down' -- a nearest-neighbour tie at .5 goes down."""
    m = np.asarray(m, np.float32).astype(np.float64)
    exact_or_raise(m[:6], disp, Ho, Wo)
    top, left, ph, pw, hs, ws = (int(v) for v in m[6:12])
    yo, xo = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing='ij')
    valid = (yo >= top) & (yo < top + ph) & (xo >= left) & (xo < left + pw)
    ys, xs = m[0] * yo + m[1] * xo + m[2], m[3] * yo + m[4] * xo + m[5]
    inside = (ys >= -0.5) & (ys < hs - 0.5) & (xs >= -0.5) & (xs < ws - 0.5)
    if disp is not None:
        d = np.asarray(disp, np.float32).astype(np.float64)
        ys2, xs2 = ys + d[0], xs + d[1]
        ys = np.where(inside, np.clip(ys2, 0, hs - 1), ys2)
        xs = np.where(inside, np.clip(xs2, 0, ws - 1), xs2)
    if mistake == 'tie_down':
        yn, xn = np.ceil(ys - 0.5).astype(np.int64), np.ceil(xs - 0.5).astype(np.int64)
    else:
        yn, xn = np.floor(ys + 0.5).astype(np.int64), np.floor(xs + 0.5).astype(np.int64)
    in_src = (yn >= 0) & (yn < hs) & (xn >= 0) & (xn < ws)
    ync, xnc = np.clip(yn, 0, hs - 1), np.clip(xn, 0, ws - 1)
    keep = valid & in_src
    out = dict(valid=valid.astype(np.float32), in_src=in_src, ys=ys, xs=xs, inside=inside)
    for k, a in (('lab', lab), ('scb', scb)):
        out[k] = None if a is None else np.where(keep, a[ync, xnc], lab_pad).astype(np.int32)
    pad = float(np.float32(img_pad))
    I = np.asarray(img, np.float32).astype(np.float64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < hs) & (xx >= 0) & (xx < ws)
        s = I[np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)]
        if mistake == 'shift':                     # the bottom / right border test off by one: the tap reads plane memory
            far = (yy >= 0) & (yy <= hs) & (xx >= 0) & (xx <= ws)
            return np.where(far, I[np.clip(yy, 0, I.shape[0] - 1), np.clip(xx, 0, I.shape[1] - 1)], pad), ok
        return (s if mistake == 'replicate' else np.where(ok, s, pad)), ok

    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    ty, tx = ys - y0, xs - x0
    if cubic == 2:
        v, ok = tap(yn, xn)
        mag, n_in = np.abs(v), ok.astype(np.int64)
    else:
        if cubic:
            wy, wx, first = keys_weights64(ty), keys_weights64(tx), -1
        else:
            wy, wx, first = [1 - ty, ty], [1 - tx, tx], 0
        v, mag, n_in = np.zeros((Ho, Wo)), np.zeros((Ho, Wo)), np.zeros((Ho, Wo), np.int64)
        for r in range(len(wy)):
            row, rmag = np.zeros((Ho, Wo)), np.zeros((Ho, Wo))
            for c in range(len(wx)):
                s, ok = tap(y0 + first + r, x0 + first + c)
                row, rmag, n_in = row + wx[c] * s, rmag + np.abs(wx[c] * s), n_in + ok
            v, mag = v + wy[r] * row, mag + np.abs(wy[r]) * rmag
    out['pre'], out['taps'] = v, (1 if cubic == 2 else 16 if cubic else 4)
    if clip is not None:
        lo, hi = min(float(np.float32(clip[2])), pad), max(float(np.float32(clip[3])), pad)
        v = np.minimum(np.maximum(v, lo), hi)
    out.update(v=np.where(keep, v, pad), mag=np.where(keep, mag, 0.0), n_in=n_in, keep=keep)
    return out


def warp_bound(ref, img_pad):
    """|got - ref64| <= 8 * 2^-24 * mag + 2^-24 * |img_pad| (the margin over the fp32 restatement's measured error: see the GPU
    module's docstring)."""
    return 8 * F32_EPS * ref['mag'] + F32_EPS * abs(float(img_pad))


def check_warp(got, ref, img_pad, what=''):
    """got: dict(img=..., lab=..., scb=..., valid=...) of one sample, None where the launch had no such output.  valid, label and
    scribble bit-equal at every pixel; the image within warp_bound at every pixel and exactly the padding wherever the
    definition assigns the constant; a nearest-neighbour image (mag is |s| there, nothing is computed) bit-equal."""
    for k in ('valid', 'lab', 'scb'):
        if got.get(k) is not None:
            bad = np.argwhere(got[k] != ref[k])
            assert len(bad) == 0, f'{what}: {k} differs at {len(bad)} pixels, first {bad[0]}: {got[k][tuple(bad[0])]} != {ref[k][tuple(bad[0])]}'
    g = np.asarray(got['img'])
    assert g.dtype == np.float32 and np.isfinite(g).all(), f'{what}: image not finite'
    d = np.abs(g.astype(np.float64) - ref['v'])
    bad = np.argwhere(d > warp_bound(ref, img_pad))
    assert len(bad) == 0, (f'{what}: image outside the bound at {len(bad)} pixels, first {bad[0]}: got {g[tuple(bad[0])]!r}, '
                           f'ref {ref["v"][tuple(bad[0])]!r}, mag {ref["mag"][tuple(bad[0])]!r}')
    const = ~ref['keep']
    assert (g[const] == np.float32(img_pad)).all(), f'{what}: padding pixels do not hold img_pad'
    if ref.get('exact'):
        assert (g == ref['v'].astype(np.float32)).all(), f'{what}: nearest-neighbour image is not a copy'


def warp_refs(launch, cubic, clip=None, img_pad=IMG_PAD, lab_pad=K):
    refs = []
    for n in range(len(launch['sizes'])):
        r = warp64(launch['img'][n], launch['lab'][n], launch['scb'][n], launch['maps'][n], HO, WO,
                   None if launch.get('disp') is None else launch['disp'][n], None if clip is None else clip[n], img_pad, lab_pad, cubic)
        r['exact'] = cubic == 2
        refs.append(r)
    return refs


def coverage(refs):
    """The pad-read classes of a list of warp64 results (of one mode): counts of kept pixels with every tap inside, with some
    taps reading the padding, of pixels of the canvas whose taps all read the padding, and of canvas pixels outside the slice
    by the nearest rule."""
    c = dict(all_in=0, some_pad=0, all_pad=0, outside=0)
    for r in refs:
        full, v = r['taps'], r['valid'] > 0
        c['all_in'] += int((r['keep'] & (r['n_in'] == full)).sum())
        c['some_pad'] += int((r['keep'] & (r['n_in'] < full) & (r['n_in'] > 0)).sum())
        c['all_pad'] += int((v & (r['n_in'] == 0)).sum())
        c['outside'] += int((v & ~r['in_src']).sum())
    return c


# ------------------------------------------------------------------------------------------ the spline path
SPLINE_SLICES = ((12, 16), (5, 7), (1, 4), (2, 3))
SPLINE_USE = (1, 0, 1, 1)


def spline_launch():
    """B = 4 over the planes above, identity map, output = the plane, a seeded float64 field of up to 3 px."""
    sizes = list(SPLINE_SLICES)
    img, lab, scb = planes(sizes, 555)
    rect = (0, 0, HP, WP)
    maps = np.stack([map_row(MAPS[0], rect, sizes[n]) for n in range(4)])
    disp64 = np.random.RandomState(556).uniform(-3.0, 3.0, size=(4, 2, HP, WP))
    return dict(img=img, lab=lab, scb=scb, maps=maps, sizes=sizes, disp64=disp64, use=np.array(SPLINE_USE, np.int32),
                clip=slice_clip(img, sizes))


def spline_ref(launch, n, img_pad=IMG_PAD, lab_pad=K):
    """Sample n of the spline launch: scipy.ndimage.map_coordinates(order=3, mode='nearest') on the float64 slice at the
    unclamped displaced coordinates, clipped like the kernel clips, padding where the (clamped-if-inside) nearest pixel lies
    outside the slice; class maps order 0 from the clamped double coordinates.  Returns dict(v, lab, scb, valid, scale, coords)."""
    hs, ws = launch['sizes'][n]
    Ho, Wo = launch['disp64'].shape[2:]
    yo, xo = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing='ij')
    inside = (yo < hs - 0.5) & (xo < ws - 0.5)
    yu, xu = yo + launch['disp64'][n, 0], xo + launch['disp64'][n, 1]
    yd, xd = np.where(inside, np.clip(yu, 0, hs - 1), yu), np.where(inside, np.clip(xu, 0, ws - 1), xu)
    yn, xn = np.floor(yd + 0.5).astype(np.int64), np.floor(xd + 0.5).astype(np.int64)
    in_src = (yn >= 0) & (yn < hs) & (xn >= 0) & (xn < ws)
    sl = launch['img'][n, :hs, :ws].astype(np.float64)
    v = scipy.ndimage.map_coordinates(sl, np.stack([yu.ravel(), xu.ravel()]), order=3, mode='nearest').reshape(Ho, Wo)
    pad = float(np.float32(img_pad))
    lo, hi = min(float(np.float32(launch['clip'][n, 2])), pad), max(float(np.float32(launch['clip'][n, 3])), pad)
    v = np.where(in_src, np.clip(v, lo, hi), pad)
    ync, xnc = np.clip(yn, 0, hs - 1), np.clip(xn, 0, ws - 1)
    return dict(v=v, valid=np.ones((Ho, Wo), np.float32), in_src=in_src,
                lab=np.where(in_src, launch['lab'][n][ync, xnc], lab_pad).astype(np.int32),
                scb=np.where(in_src, launch['scb'][n][ync, xnc], lab_pad).astype(np.int32),
                scale=float(np.abs(sl).max()), coords=(yd, xd))


def check_spline(got, ref, what=''):
    """|got - ref| <= 2^-22 * max(|ref|, max |slice|): float64 arithmetic on both sides, one fp32 rounding, and one ulp of room
    for a rounding-boundary flip.  Class maps and valid bit-equal."""
    for k in ('valid', 'lab', 'scb'):
        assert np.array_equal(got[k], ref[k]), f'{what}: {k} differs at {np.argwhere(got[k] != ref[k])[:3].tolist()}'
    g = np.asarray(got['img'])
    assert np.isfinite(g).all(), f'{what}: {int((~np.isfinite(g)).sum())} pixels not finite (a coefficient the prefilter never wrote?)'
    d = np.abs(g.astype(np.float64) - ref['v'])
    bound = 2.0 ** -22 * np.maximum(np.abs(ref['v']), ref['scale'])
    bad = np.argwhere(d > bound)
    assert len(bad) == 0, f'{what}: {len(bad)} pixels outside 2^-22, first {bad[0]}: {g[tuple(bad[0])]!r} vs {ref["v"][tuple(bad[0])]!r}'


# ------------------------------------------------------------------------------------------ Philox
def normal_sample(n, HW, seed):
    """Row n of AO.normal_field(B, HW, seed) for any B > n, without generating the other rows."""
    quads = (HW + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    r = AO.philox4x32_10(q, 0, n, 0, seed & 0xFFFFFFFF, seed >> 32)
    u = [((x >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for x in r]
    z = np.zeros((quads, 4), np.float32)
    for h in range(2):
        rad = np.sqrt(np.float32(-2.0) * np.log(u[2 * h]))
        ang = np.float32(6.283185307179586) * u[2 * h + 1]
        z[:, 2 * h], z[:, 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(-1)[:HW]


def noise_ref(x, n, sigma, rect, seed):
    """x[n] + sigma * N(0, 1) inside rect (None: the whole plane), float64."""
    H, W = x.shape[1:]
    z = normal_sample(n, H * W, seed).reshape(H, W).astype(np.float64) * float(np.float32(sigma))
    return x[n].astype(np.float64) + z * rect_mask(rect, H, W)


def check_noise(got, ref, sigma, what=''):
    """The existing tolerance 2e-4 * sigma / 2 (logf / cosf / sinf of the device against numpy's)."""
    d = np.abs(got.astype(np.float64) - ref)
    assert d.max() <= 1e-4 * sigma, f'{what}: noise off by {d.max()} at {np.unravel_index(d.argmax(), d.shape)}'


# ------------------------------------------------------------------------------------------ elementwise maps, float64
def rect_mask(rect, H, W):
    m = np.zeros((H, W), bool)
    if rect is None:
        m[:] = True
    else:
        t, l, h, w = (int(v) for v in rect)
        m[t:t + h, l:l + w] = True
    return m


def scalar_map64(x, c, rect=None):
    c = np.asarray(c, np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    return np.where(rect_mask(rect, *x.shape), np.minimum(np.maximum(c[0] * x64 + c[1], c[2]), c[3]), x64)


def gamma_map64(x, c, rect=None):
    c = np.asarray(c, np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    if c[2] <= 0:
        return x64
    return np.where(rect_mask(rect, *x.shape), np.power(np.maximum((x64 - c[0]) / c[1], 0.0), c[2]), x64)


def add_field64(x, f, rect=None):
    return x.astype(np.float64) + f.astype(np.float64) * rect_mask(rect, *x.shape)


def mix64(x, y, lam):
    lam = float(np.float32(lam))
    return x.astype(np.float64) if lam < 0 else x.astype(np.float64) * lam + y.astype(np.float64) * (1.0 - lam)


def check_elementwise(got, ref, x, touched, rtol=2e-5, atol=1e-5, what=''):
    """Whole plane against float64; where the definition leaves a pixel alone (`touched` False) it must keep its bits."""
    keep = ~np.asarray(touched, bool)
    assert (got[keep].view(np.uint32) == x[keep].view(np.uint32)).all(), f'{what}: an untouched pixel changed'
    np.testing.assert_allclose(got.astype(np.float64), ref, rtol=rtol, atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------ Gaussian filters
def gauss_radius(sigma):
    """The kernel's (and scipy's) truncation: int(4 sigma + 0.5), in fp32 like the kernel."""
    return int(np.float32(4.0) * np.float32(sigma) + np.float32(0.5))


def blur64(x, sigma, mode='reflect', extra_radius=0):
    """scipy.ndimage.gaussian_filter of one plane in float64; sigma <= 0 copies.  mode / extra_radius plant mistakes."""
    sg = float(np.float32(sigma))
    if sg <= 0:
        return x.astype(np.float64)
    if extra_radius:
        return scipy.ndimage.gaussian_filter(x.astype(np.float64), sg, mode=mode, truncate=(gauss_radius(sigma) + extra_radius) / sg)
    return scipy.ndimage.gaussian_filter(x.astype(np.float64), sg, mode=mode)


def field64(B, H, W, sigma_alpha, seed, mode='reflect', extra_radius=0):
    """pp_aug_elastic_field in float64: [B][2][H][W], Gaussian-filtered U(-1, 1) Philox noise times alpha, 0 where sigma <= 0."""
    u = AO.uniform_field(B * 2 * H * W, seed).reshape(B, 2, H, W)
    out = np.zeros(u.shape, np.float64)
    for n in range(B):
        sg, al = np.float32(sigma_alpha[n][0]), float(np.float32(sigma_alpha[n][1]))
        if sg > 0:
            for a in range(2):
                out[n, a] = blur64(u[n, a], sg, mode, extra_radius) * al
    return out


def check_blur(got, ref, x, sigma, what=''):
    """5e-4 for unit-variance planes; where the radius is 0 (sigma < 0.125) or sigma <= 0 the input bits come back."""
    if sigma <= 0 or gauss_radius(sigma) == 0:
        assert (got.view(np.uint32) == x.view(np.uint32)).all(), f'{what}: radius 0 must return the input bits'
    d = np.abs(got.astype(np.float64) - ref)
    assert d.max() <= 5e-4, f'{what}: blur off by {d.max()} at {np.unravel_index(d.argmax(), d.shape)}'


def check_field(got, ref, sigma_alpha, what=''):
    """2e-4 for fields with alpha <= 150; a sample with sigma <= 0 is exactly 0."""
    assert np.abs(np.asarray(sigma_alpha)[:, 1]).max() <= 150
    for n, (sg, _) in enumerate(sigma_alpha):
        if sg <= 0:
            assert (got[n] == 0).all(), f'{what}: sample {n} (sigma <= 0) is not exactly 0'
    d = np.abs(got.astype(np.float64) - ref)
    assert d.max() <= 2e-4, f'{what}: field off by {d.max()} at {np.unravel_index(d.argmax(), d.shape)}'


# ------------------------------------------------------------------------------------------ scribble synthesis
ANTIDIAGONAL = np.eye(3)[::-1].astype(bool)
MASK_CONTENTS = ('ones', 'empty', 'pixel', 'block2', 'border_lines', 'cut_ellipse', 'ring')


def mask(kind, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    if kind == 'ones':
        m[:] = 1
    elif kind == 'pixel':
        m[H // 2, W // 3] = 1
    elif kind == 'block2':
        m[H // 2:H // 2 + 2, W // 2:W // 2 + 2] = 1
    elif kind == 'border_lines':                            # a one-pixel line along the top row and along the right column
        m[0, :] = 1
        m[:, W - 1] = 1
    elif kind == 'cut_ellipse':                             # centred near the top-left corner: cut by two borders
        m[((yy - 0.1 * H) / (0.45 * H + 1)) ** 2 + ((xx - 0.15 * W) / (0.3 * W + 1)) ** 2 < 1] = 1
    elif kind == 'ring':
        r2 = ((yy - H / 2) / (0.4 * H + 1)) ** 2 + ((xx - W / 2) / (0.4 * W + 1)) ** 2
        m[(r2 < 1) & (r2 > 0.45)] = 1
    else:
        assert kind == 'empty'
    return m


def skeleton_masks(i, H, W):
    """The M = 5 masks of size case i: five consecutive contents of MASK_CONTENTS starting at 2 i, so that the five sizes cover
    all seven between them (and the 280 x 280 launch has the all-ones image)."""
    kinds = [MASK_CONTENTS[(2 * i + j + (3 if i == 2 else 0)) % 7] for j in range(5)]
    return kinds, np.stack([mask(k, H, W) for k in kinds])


def skeleton_ref(masks):
    from oracle import pacing_oracle as O
    return np.stack([O.skeletonize_zhang(m) for m in masks]).astype(np.uint8)


def dilation_case(H, W):
    """M = 3 (seed, mask) pairs: seeds in the four corners; on a mask edge; outside the mask (it must stay set, as in scipy)."""
    yy, xx = np.mgrid[0:H, 0:W]
    seeds, masks = np.zeros((3, H, W), np.uint8), np.zeros((3, H, W), np.uint8)
    masks[0] = 1
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        seeds[0, y, x] = 1
    masks[1, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1
    seeds[1, H // 4, W // 4 + 2] = 1                        # on the mask's top edge
    seeds[1, 3 * H // 4 - 1, 3 * W // 4 - 1] = 1            # its bottom-right corner
    seeds[1, H // 2, W // 4] = 1                            # its left edge
    masks[2] = ((yy + xx) % 7 != 0) & (xx > W // 3)
    seeds[2, H // 2, W // 2] = 1
    seeds[2, 1, 1] = 1                                      # outside the mask
    seeds[2, H - 2, W // 6] = 1                             # outside the mask
    return seeds, masks


def dilation_ref(seeds, masks, iterations):
    """Exactly `iterations` steps; 0 steps is the identity (scipy reads iterations < 1 as "until nothing changes", which is NOT
    the entry point's contract, so scipy is asked only for iterations >= 1)."""
    if iterations == 0:
        return (seeds != 0).astype(np.uint8)
    return np.stack([scipy.ndimage.binary_dilation(s != 0, structure=ANTIDIAGONAL, iterations=iterations, mask=m != 0)
                     for s, m in zip(seeds, masks)]).astype(np.uint8)


def curves(H, W):
    """M = 3 curve images: curves ending in corners and on edges; an isolated pixel, a T-junction; a closed loop."""
    c = np.zeros((3, H, W), np.uint8)
    for i in range(min(H, W)):                              # a diagonal from the top-left corner, ending inside or at an edge
        c[0, i, i] = 1
    c[0, H - 1, W - 3:] = 1                                 # a short stroke ending in the bottom-right corner
    c[1, H // 2, 0:W - 2] = 1                               # a stroke starting on the left edge ...
    c[1, 0:H // 2, 2] = 1                                   # ... with a stem to the top edge: a T-junction
    c[1, H - 1, W - 1] = 1                                  # an isolated pixel: no end point
    c[2, 1, 1:W - 1] = 1
    c[2, H - 2, 1:W - 1] = 1
    c[2, 1:H - 1, 1] = 1
    c[2, 1:H - 1, W - 2] = 1                                # a closed loop: no end point
    return c


def endpoints_ref(img):
    ring = np.ones((3, 3), np.int64)
    ring[1, 1] = 0
    return np.stack([(m != 0) & (scipy.ndimage.convolve((m != 0).astype(np.int64), ring, mode='constant', cval=0) == 1)
                     for m in img]).astype(np.uint8)


def check_masks(got, ref, what=''):
    """Bit-equal, mask by mask (a mask swapped with its neighbour in the batch fails)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    for n in range(len(ref)):
        bad = np.argwhere(got[n] != ref[n])
        assert len(bad) == 0, f'{what}: mask {n} differs at {len(bad)} pixels, first {bad[0].tolist()}'


# largest image pp_skeletonize / pp_dilate_antidiagonal admit: two zero-bordered byte images in dynamic LDS,
# 2 (H + 2)(W + 2) <= 160 KB - 64, i.e. (H + 2)(W + 2) <= 81888; with the skeleton kernel's 4 static bytes that is at most
# 163780 of the 163840 bytes a workgroup can have.  The largest square: 284 x 284 (286^2 = 81796); 285 x 285 (287^2 = 82369) is out.
LDS_BYTES = 160 * 1024
SK_LARGEST_SQUARE = 284


def scribble_lds(H, W, static=4):
    return 2 * (H + 2) * (W + 2) + static
