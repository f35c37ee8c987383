"""The input-side kernels entry by entry through the C ABI against float64 and scipy: the 13 augmentation entry points of
pacingpseudo_amd/csrc/pp_augment.hip and the scribble-synthesis kernels at the end of pp_spatial.hip (pp_skeletonize,
pp_dilate_antidiagonal, pp_curve_endpoints).  Every comparison is per pixel over the whole output; no share of pixels is left out.
References, case tables and comparators live in tests/_input_reference.py; tests/test_input_kernels.py checks them without a GPU
and hands every comparator a planted mistake.

What is new against test_gpu_augment.py / test_gpu_augment_ref.py / test_gpu_round2.py:
  * every grid-stride loop of pp_augment.hip behind a CAPPED grid makes a second trip (scalar_map, gamma, add_field, mix,
    add_noise, warp, onehot, gaussian_blur, elastic_field with its uniform draw): each loop shape asserts total > cap * 256 with the
    cap and the block size read from the source (_input_reference.grid_caps).  pp_aug_spline_prefilter's grid is not capped, its
    loop never makes a second trip; pp_aug_warp_spline launches the kernel of pp_aug_warp with the same cap;
  * the warp is decided at EVERY pixel: dyadic maps make the source coordinates exact in fp32 and float64, so valid, label and
    scribble must be bit-equal (ties at .5 go up) and the image must satisfy
        |got - ref64| <= 8 * 2^-24 * mag + 2^-24 * |img_pad|,      mag = sum |w_y w_x s| over the taps.
    The 8: the project's own fp32 restatement of the kernel (oracle/augment_oracle.py: warp), which performs the same operations in
    the same order without contraction, stays within 2.460 * 2^-24 * mag (Keys; bilinear 2.428; nearest 0) of the float64 reference
    over the whole case table -- measured, and asserted to stay below 4, by
    test_input_kernels.py::test_keys_ratio_of_the_fp32_restatement_over_the_case_table;
  * plane memory outside a ragged slice holds 1.0e6 / 99 and img_pad is -3, so a tap that reads outside (hs, ws) shows;
  * bilinear and nearest modes, null class-map / valid outputs, coef mode 3, noise with rectangles and a partial last quad, blur and
    field on axes of length 1 and radii beyond twice the axis, the spline path on small ragged slices with NaN in every
    coefficient the prefilter does not write;
  * pp_skeletonize / pp_dilate_antidiagonal above the 64 KB default of dynamic LDS (256 x 256 and 280 x 280 masks), M > 1, H != W,
    structures on the border, degenerate images.  skimage is not installed: the skeleton's yardstick is the oracle's restatement of
    Zhang-Suen thinning (oracle.pacing_oracle.skeletonize_zhang)."""
import numpy as np
import pytest
import torch

from oracle import augment_oracle as AO
from tests import _input_reference as R

pytestmark = pytest.mark.gpu


def _lib():
    from pacingpseudo_amd._lib import lib
    return lib


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ pp_aug_warp
def _warp(L, cubic, clip=None, outputs=True, Ho=R.HO, Wo=R.WO, spline=None):
    """One launch of pp_aug_warp (or, with spline = (coef, use, disp64), pp_aug_warp_spline) over the planes of L.  outputs False:
    the image-only call form of DeviceAugmenter._lowres (null class maps, null valid).  Outputs start as NaN / -7."""
    B, Hp, Wp = L['img'].shape
    img, lab, scb, maps = _dev(L['img']), _dev(L['lab']), _dev(L['scb']), _dev(L['maps'])
    disp, cl = _dev(L.get('disp')), _dev(clip)
    oi = torch.full((B, Ho, Wo), float('nan'), device='cuda')
    ol, os_ = (torch.full((B, Ho, Wo), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    ov = torch.full((B, Ho, Wo), float('nan'), device='cuda')
    if not outputs:
        lab = scb = ol = os_ = ov = None
    head = (img.data_ptr(), _ptr(lab), _ptr(scb), Hp, Wp, oi.data_ptr(), _ptr(ol), _ptr(os_), _ptr(ov), Ho, Wo, B, maps.data_ptr(), _ptr(disp))
    if spline is None:
        _lib().pp_aug_warp(*head, _ptr(cl), R.IMG_PAD, R.K, cubic, _s())
    else:
        coef, use, d64 = spline
        _lib().pp_aug_warp_spline(*head, _ptr(d64), _ptr(cl), R.IMG_PAD, R.K, cubic, coef.data_ptr(), use.data_ptr(), _s())
    torch.cuda.synchronize()
    return dict(img=oi.cpu().numpy(), lab=None if ol is None else ol.cpu().numpy(), scb=None if os_ is None else os_.cpu().numpy(),
                valid=None if ov is None else ov.cpu().numpy())


def _sample(out, n):
    return {k: (None if v is None else v[n]) for k, v in out.items()}


@pytest.mark.parametrize('cubic', [0, 1, 2], ids=['bilinear', 'keys', 'nearest'])
def test_warp_case_table_every_pixel(cubic):
    """8 maps x 4 slice sizes x 4 canvas rectangles (16 launches of B = 8), clip_stats null / never engaging / the slice's own range
    (narrower than the Keys overshoot at the step edge)."""
    engaged = 0
    for s in range(4):
        for r in range(4):
            L = R.warp_launch(s, r)
            plain = _warp(L, cubic)
            for n, ref in enumerate(R.warp_refs(L, cubic)):
                R.check_warp(_sample(plain, n), ref, R.IMG_PAD, f's{s} r{r} sample {n}')
            wide = _warp(L, cubic, R.wide_clip(8))
            assert all(np.array_equal(wide[k].view(np.uint32), plain[k].view(np.uint32)) for k in wide), 'a clamp that never engages changed bits'
            clip = R.slice_clip(L['img'], L['sizes'])
            tight = _warp(L, cubic, clip)
            for n, ref in enumerate(R.warp_refs(L, cubic, clip)):
                R.check_warp(_sample(tight, n), ref, R.IMG_PAD, f's{s} r{r} sample {n} clipped')
            engaged += int((tight['img'] != plain['img']).sum())
    assert cubic != 1 or engaged >= 10, 'the clamp never engaged'


@pytest.mark.parametrize('cubic', [0, 1, 2], ids=['bilinear', 'keys', 'nearest'])
def test_warp_image_only_call_form_gives_the_same_bits(cubic):
    """out_lab, out_scb, out_valid (and lab, scb) null, as _lowres and the Mixup partner path call it."""
    for s, r in ((0, 0), (1, 1), (2, 3)):
        L = R.warp_launch(s, r)
        clip = R.slice_clip(L['img'], L['sizes'])
        full, bare = _warp(L, cubic, clip), _warp(L, cubic, clip, outputs=False)
        assert np.array_equal(full['img'].view(np.uint32), bare['img'].view(np.uint32))
        for n, ref in enumerate(R.warp_refs(L, cubic, clip)):
            R.check_warp(_sample(bare, n), ref, R.IMG_PAD, f's{s} r{r} sample {n} image only')


@pytest.mark.parametrize('cubic', [1, 0, 2], ids=['keys', 'bilinear', 'nearest'])
def test_warp_displacement_clamps_only_points_that_started_inside(cubic):
    """A dyadic field (multiples of 1/4 up to 3 px): a point whose undisplaced position lies inside the slice is clamped to it at
    all four edges, one that lies outside is not (test_input_kernels.py asserts the field produces every one of these)."""
    L = R.disp_launch()
    for clip in (None, R.slice_clip(L['img'], L['sizes'])):
        out = _warp(L, cubic, clip)
        for n, ref in enumerate(R.warp_refs(L, cubic, clip)):
            R.check_warp(_sample(out, n), ref, R.IMG_PAD, f'disp sample {n}')


def test_warp_grid_stride_loop():
    """B = 9 outputs of 512 x 512 from 64 x 64 planes through the 1/8-scale map: 2,359,296 pixels against 8192 x 256 threads; the
    whole of sample 8 is written by the second trip round the loop."""
    B, Hs, Ho = 9, 64, 512
    total = B * Ho * Ho
    assert total > R.loop_threads('pp_aug_warp') and 8 * Ho * Ho >= R.loop_threads('pp_aug_warp')
    sizes = [(64, 64), (40, 50), (64, 33), (17, 64), (64, 64), (5, 7), (33, 64), (64, 64), (40, 50)]
    rects = [(0, 0, Ho, Ho)] * 8 + [(100, 37, 300, 411)]
    img, lab, scb = R.planes(sizes, 900, Hs, Hs)
    maps = np.stack([R.map_row(R.MAPS[7], rects[n], sizes[n]) for n in range(B)])
    L = dict(img=img, lab=lab, scb=scb, maps=maps)
    clip = R.slice_clip(img, sizes)
    out = _warp(L, 1, clip, Ho=Ho, Wo=Ho)
    for n in (0, 4, 8):
        ref = R.warp64(img[n], lab[n], scb[n], maps[n], Ho, Ho, None, clip[n], R.IMG_PAD, R.K, 1)
        R.check_warp(_sample(out, n), ref, R.IMG_PAD, f'loop sample {n}')
    for n in range(B):
        one = _warp({k: v[n:n + 1] for k, v in L.items()}, 1, clip[n:n + 1], Ho=Ho, Wo=Ho)
        for k in one:
            assert np.array_equal(one[k][0].view(np.uint32), out[k][n].view(np.uint32)), f'sample {n}: {k} differs from the B = 1 launch'


# ------------------------------------------------------------------------------------------ spline path
def test_spline_prefilter_and_warp_on_small_ragged_slices():
    """B = 4, use = [1, 0, 1, 1], slices (12, 16), (5, 7), (1, 4), (2, 3) in 12 x 16 planes with the sentinel outside, a float64
    field of up to 3 px through disp64, the coefficient buffer full of NaN before the prefilter.  Against
    scipy.ndimage.map_coordinates(order=3, mode='nearest') on the float64 slice; sample 1 against pp_aug_warp's bits."""
    L = R.spline_launch()
    B, Hp, Wp = L['img'].shape
    img, maps, use = _dev(L['img']), _dev(L['maps']), _dev(L['use'])
    coef = torch.full((B, Hp + 24, Wp + 24), float('nan'), dtype=torch.float64, device='cuda')
    _lib().pp_aug_spline_prefilter(img.data_ptr(), B, Hp, Wp, maps.data_ptr(), use.data_ptr(), coef.data_ptr(), _s())
    torch.cuda.synchronize()
    c = coef.cpu().numpy()
    for n, (hs, ws) in enumerate(L['sizes']):
        written = np.isfinite(c[n])
        if L['use'][n]:
            assert written[:hs + 24, :ws + 24].all() and written.sum() == (hs + 24) * (ws + 24), f'sample {n}: coefficients written'
            np.testing.assert_allclose(c[n, :hs + 24, :ws + 24], AO.spline_coefficients(L['img'][n, :hs, :ws]), rtol=0, atol=1e-9 * 2200)
        else:
            assert not written.any(), 'the prefilter wrote coefficients of a sample that does not use the spline'
    out = _warp(L, 1, L['clip'], Ho=Hp, Wo=Wp, spline=(coef, use, _dev(L['disp64'])))
    for n in range(B):
        if L['use'][n]:
            R.check_spline(_sample(out, n), R.spline_ref(L, n), f'spline sample {n}')
    keys = _warp(dict(L, disp=L['disp64'].astype(np.float32)), 1, L['clip'], Ho=Hp, Wo=Wp)
    for k in keys:
        assert np.array_equal(keys[k][1].view(np.uint32), out[k][1].view(np.uint32)), f'use = 0 sample: {k} differs from pp_aug_warp'


# ------------------------------------------------------------------------------------------ pp_aug_stats, pp_aug_coef
@pytest.mark.parametrize('H,W', [(7, 9), (33, 65)])
def test_stats_planes_and_rectangles(H, W):
    rng = np.random.RandomState(11)
    x = np.stack([rng.normal(size=(H, W)) * 20 + 50, -np.abs(rng.normal(size=(H, W))) - 1, np.abs(rng.normal(size=(H, W))) + 1,
                  np.full((H, W), 0.5), rng.normal(size=(H, W))]).astype(np.float32)
    B = len(x)
    forms = [(0, 0, H, W), (H // 2, W // 3, 1, 1), (H - 1, 0, 1, W), (0, W - 1, H, 1), (2, 1, 0, 4)]     # full, one pixel, last row, last column, empty
    xd = _dev(x)
    st = torch.full((B, 4), float('nan'), dtype=torch.float64, device='cuda')
    for shift in [None] + list(range(5)):
        rect = None if shift is None else np.array([forms[(n + shift) % 5] for n in range(B)], np.int32)
        st.fill_(float('nan'))
        rd = _dev(rect)
        _lib().pp_aug_stats(xd.data_ptr(), B, H, W, _ptr(rd), st.data_ptr(), _s())
        got = st.cpu().numpy()
        want = np.stack([AO.stats(x[n], None if rect is None else rect[n]) for n in range(B)])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9, err_msg=f'rect shift {shift}')
        for n in range(B):
            if rect is not None and rect[n][2] * rect[n][3] == 0:
                assert (got[n] == 0).all(), 'an empty rectangle gives all zeros'
            elif n == 3:
                assert got[n, 1] == 0 and got[n, 2] == got[n, 3] == 0.5, 'a constant plane: std exactly 0, min == max'
            if n == 1 and (rect is None or rect[n][2] * rect[n][3]):
                assert got[n, 3] < 0                                    # all negative: a max that started at 0 would show
            if n == 2 and (rect is None or rect[n][2] * rect[n][3]):
                assert got[n, 2] > 0


def test_coef_all_modes_second_block():
    """All five modes, mode 3 with its stats0, SKIP rows, a std = 0 row, B = 65 (the second block of 64) against AO.coef."""
    B = 65
    rng = np.random.RandomState(12)
    st = np.stack([-rng.uniform(1, 60, B), rng.uniform(0.5, 30, B), rng.uniform(-200, -100, B), rng.uniform(100, 200, B)], 1)
    st0 = np.stack([rng.uniform(1, 60, B), rng.uniform(0.5, 30, B), rng.uniform(-200, -100, B), rng.uniform(100, 200, B)], 1)
    st[[7, 64], 1] = 0.0
    par = rng.uniform(0.5, 1.5, B).astype(np.float32)
    par[[3, 33, 64]] = AO.SKIP
    std, st0d, pd = _dev(st), _dev(st0), _dev(par)
    coef = torch.empty(B, 4, device='cuda')
    for mode in range(5):
        coef.fill_(float('nan'))
        _lib().pp_aug_coef(None if mode == 4 else std.data_ptr(), st0d.data_ptr() if mode == 3 else None, pd.data_ptr() if mode else None,
                           mode, B, coef.data_ptr(), _s())
        want = np.stack([AO.coef(mode, st[n], st0[n], par[n] if mode else None) for n in range(B)])
        np.testing.assert_allclose(coef.cpu().numpy(), want, rtol=1e-6, err_msg=f'mode {mode}')
    with pytest.raises(Exception, match='aug_coef'):
        _lib().pp_aug_coef(std.data_ptr(), None, pd.data_ptr(), 3, B, coef.data_ptr(), _s())          # mode 3 without stats0


# ------------------------------------------------------------------------------------------ elementwise maps
def _elementwise_case(B, H, W, rects, seed):
    rng = np.random.RandomState(seed)
    x = (rng.normal(size=(B, H, W)) * 20 + 50).astype(np.float32)
    lin = np.stack([rng.uniform(0.5, 2, B), rng.uniform(-30, 30, B), np.where(np.arange(B) % 2, 20.0, -3.0e38),
                    np.where(np.arange(B) % 2, 80.0, 3.0e38)], 1).astype(np.float32)
    gam = np.stack([x.reshape(B, -1).min(1), x.reshape(B, -1).max(1) - x.reshape(B, -1).min(1) + 1e-8,
                    np.array([0.7, 1.5, -1.0, 0.4, 2.0, 0.0, 1.0, 0.9])[np.arange(B) % 8], np.zeros(B)], 1).astype(np.float32)
    f = rng.normal(size=(B, H, W)).astype(np.float32)
    xm, ym = (np.abs(rng.normal(size=(B, H, W))) + 0.5).astype(np.float32), (np.abs(rng.normal(size=(B, H, W))) + 0.5).astype(np.float32)
    lam = np.array([0.8, -1.0, 1.0, 0.0, 0.93, -0.5, 0.85, 0.99], np.float32)[np.arange(B) % 8]
    return x, lin, gam, f, xm, ym, lam, np.array(rects, np.int32)


def _check_elementwise_entries(B, H, W, rects, seed):
    x, lin, gam, f, xm, ym, lam, rect = _elementwise_case(B, H, W, rects, seed)
    lib, s = _lib(), _s()
    for use_rect in (True, False):
        rd = _dev(rect) if use_rect else None
        rl = [rect[n] if use_rect else None for n in range(B)]
        inside = np.stack([R.rect_mask(rl[n], H, W) for n in range(B)])
        y, c = _dev(x), _dev(lin)
        lib.pp_aug_scalar_map(y.data_ptr(), B, H, W, c.data_ptr(), _ptr(rd), s)
        R.check_elementwise(y.cpu().numpy(), np.stack([R.scalar_map64(x[n], lin[n], rl[n]) for n in range(B)]), x, inside, what='scalar_map')
        y, c = _dev(x), _dev(gam)
        lib.pp_aug_gamma(y.data_ptr(), B, H, W, c.data_ptr(), _ptr(rd), s)
        R.check_elementwise(y.cpu().numpy(), np.stack([R.gamma_map64(x[n], gam[n], rl[n]) for n in range(B)]), x,
                            inside & (gam[:, 2] > 0)[:, None, None], what='gamma')
        y, fd = _dev(x), _dev(f)
        lib.pp_aug_add_field(y.data_ptr(), fd.data_ptr(), B, H, W, _ptr(rd), s)
        R.check_elementwise(y.cpu().numpy(), np.stack([R.add_field64(x[n], f[n], rl[n]) for n in range(B)]), x, inside, what='add_field')
    y, yd, ld = _dev(xm), _dev(ym), _dev(lam)
    lib.pp_aug_mix(y.data_ptr(), yd.data_ptr(), B, H * W, ld.data_ptr(), s)
    # two products and a sum of positive terms: three fp32 roundings, 1.8e-7, against rtol 2e-6 and nothing else
    R.check_elementwise(y.cpu().numpy(), np.stack([R.mix64(xm[n], ym[n], lam[n]) for n in range(B)]), xm,
                        np.broadcast_to((lam >= 0)[:, None, None], xm.shape), rtol=2e-6, atol=0, what='mix')


def test_scalar_map_gamma_add_field_mix_small_planes_edge_rectangles():
    """7 x 9 planes (fewer elements than one block has threads per sample), rectangles on every edge, one pixel, empty; samples with
    gamma <= 0 and lam < 0 and pixels outside the rectangle keep their bits."""
    rects = [(0, 0, 7, 9), (0, 0, 1, 9), (6, 0, 1, 9), (0, 8, 7, 1), (3, 4, 1, 1), (2, 2, 0, 5), (1, 1, 5, 7), (0, 0, 7, 1)]
    _check_elementwise_entries(8, 7, 9, rects, 21)


def test_scalar_map_gamma_add_field_mix_grid_stride_loop():
    """B = 5 at 512 x 512: 1,310,720 elements against 4096 x 256 threads; sample 4 is written by the second trip round the loop."""
    B, H = 5, 512
    for e in ('pp_aug_scalar_map', 'pp_aug_gamma', 'pp_aug_add_field', 'pp_aug_mix'):
        assert B * H * H > R.loop_threads(e) and 4 * H * H >= R.loop_threads(e)
    _check_elementwise_entries(B, H, H, [(0, 0, H, H), (10, 20, 400, 300), (511, 0, 1, 512), (0, 0, H, H), (100, 50, 300, 411)], 22)


# ------------------------------------------------------------------------------------------ pp_aug_add_noise
def _start_plane(B, H, W, seed):
    return (np.random.RandomState(seed).randint(-16, 17, size=(B, H, W)) / 8.0).astype(np.float32)      # |x| <= 2, multiples of 1/8


def test_add_noise_partial_last_quad_and_rectangles():
    """5 x 7 planes: 35 pixels, the ninth quad of a sample holds three and must not touch the next sample."""
    B, H, W = 6, 5, 7
    x = _start_plane(B, H, W, 31)
    sigma = np.array([0.5, 0.0, 2.0, 0.1, 1.0, 0.25], np.float32)
    rects = np.array([(0, 0, 5, 7), (0, 0, 5, 7), (4, 0, 1, 7), (0, 6, 5, 1), (1, 2, 3, 4), (2, 2, 0, 3)], np.int32)
    for rect in (None, rects):
        y, sd, rd = _dev(x), _dev(sigma), _dev(rect)
        _lib().pp_aug_add_noise(y.data_ptr(), B, H, W, sd.data_ptr(), _ptr(rd), 0xABCDEF0123, _s())
        got = y.cpu().numpy()
        for n in range(B):
            rn = None if rect is None else rect[n]
            keep = ~R.rect_mask(rn, H, W) | (sigma[n] <= 0)
            assert (got[n][keep].view(np.uint32) == x[n][keep].view(np.uint32)).all(), f'sample {n}: a pixel outside the rectangle changed'
            if sigma[n] > 0:
                R.check_noise(got[n], R.noise_ref(x, n, sigma[n], rn, 0xABCDEF0123), float(sigma[n]), f'sample {n}')
                assert (got[n][~keep] != x[n][~keep]).all()


def test_add_noise_grid_stride_loop():
    """B = 17 at 512 x 512: 1,114,112 quads against 4096 x 256 threads; sample 16 is drawn by the second trip round the loop."""
    B, H = 17, 512
    assert B * (H * H // 4) > R.loop_threads('pp_aug_add_noise') and 16 * (H * H // 4) >= R.loop_threads('pp_aug_add_noise')
    x = _start_plane(B, H, H, 32)
    sigma = np.linspace(0.2, 1.8, B).astype(np.float32)
    rect = np.array([(0, 0, H, H)] * 16 + [(3, 100, 500, 411)], np.int32)
    y, sd, rd = _dev(x), _dev(sigma), _dev(rect)
    _lib().pp_aug_add_noise(y.data_ptr(), B, H, H, sd.data_ptr(), rd.data_ptr(), 20240607, _s())
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    for n in range(B):
        inside = R.rect_mask(rect[n], H, H)
        assert (got[n][~inside] == x[n][~inside]).all()
        if n in (0, 8, 16):
            R.check_noise(got[n], R.noise_ref(x, n, sigma[n], rect[n], 20240607), float(sigma[n]), f'sample {n}')
        else:
            assert (got[n][inside] != x[n][inside]).mean() > 0.999, f'sample {n} did not change'
    assert not np.array_equal(got[1] - x[1], got[2] - x[2])


# ------------------------------------------------------------------------------------------ Gaussian blur, elastic field
GAUSS_CASES = [((1, 7), 2.0), ((7, 1), 2.0), ((3, 5), 2.0), ((2, 2), 3.0), ((37, 53), 1.7), ((9, 4), 0.1), ((9, 4), 0.124), ((9, 4), 0.126)]


def _blur(x, sigmas):
    B, H, W = x.shape
    y, scr = _dev(x), torch.full((B, H, W), float('nan'), device='cuda')
    sp = _dev(np.stack([sigmas, np.zeros(B)], 1).astype(np.float32))
    _lib().pp_aug_gaussian_blur(y.data_ptr(), scr.data_ptr(), B, H, W, sp.data_ptr(), _s())
    return y.cpu().numpy()


def _field(B, H, W, sa, seed):
    disp, scr = (torch.full((B, 2, H, W), float('nan'), device='cuda') for _ in range(2))
    sd = _dev(sa)
    _lib().pp_aug_elastic_field(disp.data_ptr(), scr.data_ptr(), B, H, W, sd.data_ptr(), seed, _s())
    return disp.cpu().numpy()


@pytest.mark.parametrize('shape,sigma', GAUSS_CASES)
def test_gaussian_blur_and_elastic_field_small_shapes(shape, sigma):
    """Axes of length 1, radii beyond twice the axis (several reflections), the radius stepping 0 -> 1 between sigma 0.124 and 0.126;
    per-sample sigma mixed with sigma <= 0 (blur: the bits come back; field: exactly 0)."""
    H, W = shape
    x = np.random.RandomState(41).normal(size=(4, H, W)).astype(np.float32)
    sig = np.array([sigma, 0.0, -1.0, sigma], np.float32)
    got = _blur(x, sig)
    for n in range(4):
        R.check_blur(got[n], R.blur64(x[n], sig[n]), x[n], float(sig[n]), f'blur {shape} sample {n}')
    sa = np.array([[sigma, 150.0], [0.0, 0.0], [sigma, 40.0], [-1.0, 10.0]], np.float32)
    R.check_field(_field(4, H, W, sa, 4243), R.field64(4, H, W, sa, 4243), sa, f'field {shape}')


def test_gaussian_blur_mixed_sigma_in_one_launch():
    x = np.random.RandomState(42).normal(size=(6, 37, 53)).astype(np.float32)
    sig = np.array([1.7, 0.0, 2.0, -1.0, 0.124, 0.6], np.float32)
    got = _blur(x, sig)
    for n in range(6):
        R.check_blur(got[n], R.blur64(x[n], sig[n]), x[n], float(sig[n]), f'sample {n}')
    sa = np.stack([sig, [150, 0, 100, 7, 150, 20]], 1).astype(np.float32)
    R.check_field(_field(6, 37, 53, sa, 99), R.field64(6, 37, 53, sa, 99), sa, 'mixed field')


def test_gaussian_blur_and_elastic_field_grid_stride_loops():
    """Blur B = 9 at 512 x 512 (2,359,296 elements), field B = 5 (2,621,440), against 8192 x 256 threads; the field's uniform draw,
    one thread per four elements, loops only from B = 17 on: there sigma 0.1 (radius 0) and alpha 1 return the draw itself."""
    H = 512
    assert 9 * H * H > R.loop_threads('pp_aug_gaussian_blur') and 5 * 2 * H * H > R.loop_threads('pp_aug_elastic_field')
    x = np.random.RandomState(43).normal(size=(9, H, H)).astype(np.float32)
    sig = np.full(9, 1.0, np.float32)
    got = _blur(x, sig)
    for n in range(9):
        R.check_blur(got[n], R.blur64(x[n], 1.0), x[n], 1.0, f'loop blur sample {n}')
    sa = np.array([[2.0, 150.0]] * 4 + [[2.0, 60.0]], np.float32)
    R.check_field(_field(5, H, H, sa, 5150), R.field64(5, H, H, sa, 5150), sa, 'loop field')
    B = 17
    assert (B * 2 * H * H + 3) // 4 > R.loop_threads('pp_aug_elastic_field')
    draw = _field(B, H, H, np.array([[0.1, 1.0]] * B, np.float32), 31337)
    assert np.array_equal(draw.reshape(-1), AO.uniform_field(B * 2 * H * H, 31337)), 'the uniform draw is not the Philox stream'


# ------------------------------------------------------------------------------------------ pp_aug_onehot
@pytest.mark.parametrize('B,K,H,W', [(3, 5, 7, 9), (2, 5, 512, 512)], ids=['odd', 'loop'])
def test_onehot(B, K, H, W):
    """Labels K and -1 set no plane; odd H W; B = 2, K = 5 at 512 x 512 is 2,621,440 elements against 8192 x 256 threads."""
    if H == 512:
        assert B * K * H * W > R.loop_threads('pp_aug_onehot')
    lab = np.random.RandomState(51).randint(-1, K + 1, size=(B, H, W)).astype(np.int32)
    assert (lab == K).any() and (lab == -1).any()
    ld, out = _dev(lab), torch.full((B, K, H, W), float('nan'), device='cuda')
    _lib().pp_aug_onehot(ld.data_ptr(), out.data_ptr(), B, K, H * W, _s())
    got = out.cpu().numpy()
    want = np.stack([AO.to_one_hot(lab[n], K) for n in range(B)])
    assert np.array_equal(got, want)
    assert (got.sum(1)[(lab == K) | (lab == -1)] == 0).all()


# ------------------------------------------------------------------------------------------ scribble synthesis
SKELETON_SIZES = [(37, 53), (256, 256), (280, 280), (1, 9), (9, 1)]


@pytest.mark.parametrize('i', range(5), ids=[f'{h}x{w}' for h, w in SKELETON_SIZES])
def test_skeletonize_five_masks_per_launch(i):
    """One launch of M = 5 different masks (block index -> mask).  256 x 256 needs 133 KB and 280 x 280 (the size the source
    promises) 159 KB of dynamic LDS: above the 64 KB default, the pp_max_lds path."""
    H, W = SKELETON_SIZES[i]
    kinds, masks = R.skeleton_masks(i, H, W)
    if H >= 256:
        assert 64 * 1024 < R.scribble_lds(H, W) <= R.LDS_BYTES
    md = _dev(masks * 255 if i == 0 else masks)                      # any non-zero byte is set
    _lib().pp_skeletonize(md.data_ptr(), 5, H, W, _s())
    R.check_masks(md.cpu().numpy(), R.skeleton_ref(masks), f'skeleton {H}x{W} {kinds}')


def test_skeletonize_refuses_one_size_above_the_largest_without_launching():
    """The argument check against 160 KB of LDS: two zero-bordered byte images, 2 (H + 2)(W + 2) <= 160 KB - 64, plus the kernel's 4
    static bytes.  The largest square admitted is 284 x 284 (2 * 286^2 + 4 = 163596 <= 163840); 285 x 285 must be refused with the
    masks untouched."""
    from pacingpseudo_amd._lib import HipLibraryError
    n = R.SK_LARGEST_SQUARE + 1
    assert R.scribble_lds(n - 1, n - 1) <= R.LDS_BYTES and 2 * (n + 2) ** 2 > R.LDS_BYTES - 64
    masks = np.ones((1, n, n), np.uint8)
    md = _dev(masks)
    with pytest.raises(HipLibraryError, match='skeletonize'):
        _lib().pp_skeletonize(md.data_ptr(), 1, n, n, _s())
    with pytest.raises(HipLibraryError, match='dilate_antidiagonal'):
        _lib().pp_dilate_antidiagonal(md.data_ptr(), md.data_ptr(), 1, n, n, 1, _s())
    torch.cuda.synchronize()
    assert np.array_equal(md.cpu().numpy(), masks)


@pytest.mark.parametrize('iterations', [0, 1, 40])
@pytest.mark.parametrize('H,W', [(37, 53), (256, 256)])
def test_dilate_antidiagonal(H, W, iterations):
    """M = 3: seeds in the four corners, on a mask edge, and outside the mask (they stay set, as in scipy)."""
    seeds, masks = R.dilation_case(H, W)
    sd, md = _dev(seeds * 3), _dev(masks * 200)
    _lib().pp_dilate_antidiagonal(sd.data_ptr(), md.data_ptr(), 3, H, W, iterations, _s())
    R.check_masks(sd.cpu().numpy(), R.dilation_ref(seeds, masks, iterations), f'dilate {H}x{W} x{iterations}')
    assert np.array_equal(md.cpu().numpy(), masks * 200)


@pytest.mark.parametrize('H,W', [(5, 7), (37, 53)])
def test_curve_endpoints(H, W):
    """M = 3: curves ending in corners and on edges, an isolated pixel, a T-junction, a closed loop."""
    img = R.curves(H, W)
    d, out = _dev(img * 9), torch.full((3, H, W), 77, dtype=torch.uint8, device='cuda')
    _lib().pp_curve_endpoints(d.data_ptr(), out.data_ptr(), 3, H, W, _s())
    R.check_masks(out.cpu().numpy(), R.endpoints_ref(img), f'end points {H}x{W}')
