"""CPU companions of tests/test_gpu_input_kernels.py: the float64 references of tests/_input_reference.py checked against scipy
and against the project's own fp32 restatement, the coverage of the warp case table asserted from the reference, the Keys ratio
re-measured over that table, and every comparator handed a reference output with ONE planted mistake, which it must reject --
so the tolerances of the GPU module stay honest without a GPU.

Which planted mistake goes to which comparator:
  a tap shifted by one at a slice border (it reads plane memory outside the slice), a border tap clamped to the slice
  instead of reading the padding, a tie rounded down, one pixel outside a rectangle changed          -> check_warp
  an unwritten (NaN) coefficient, a coordinate moved by 2^-12 px                                     -> check_spline
  radius + 1, 'reflect' replaced by 'mirror'                                                         -> check_field
  'reflect' replaced by 'mirror', a radius of 1 where it must be 0                                   -> check_blur
  one pixel outside a rectangle changed (by one ulp)                                                 -> check_elementwise
  a sample drawn with its neighbour's counter                                                        -> check_noise
  a mask swapped with its neighbour in the batch, one iteration too many, a border end point missed  -> check_masks
radius + 1 is NOT given to check_blur: scipy and the kernel cut the Gaussian at int(4 sigma + 0.5) >= 4 sigma - 0.5, so the first
tap left out weighs at most exp(-8) / (sigma sqrt(2 pi)) of the sum, 1.3e-4 / sigma, times the difference of two samples of a
unit-variance plane: below the project's 5e-4 for every sigma >= 1.  The elastic field multiplies the same filter by alpha up to
150, where the same mistake is far outside 2e-4; that comparator carries it."""
import os

import numpy as np
import pytest
import scipy.ndimage

from oracle import augment_oracle as AO
from tests import _input_reference as R


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ------------------------------------------------------------------------------------------ launch geometry
def test_grid_caps_are_read_from_the_source():
    caps = R.grid_caps()
    small = ('pp_aug_scalar_map', 'pp_aug_gamma', 'pp_aug_add_field', 'pp_aug_mix', 'pp_aug_add_noise')
    large = ('pp_aug_warp', 'pp_aug_warp_spline', 'pp_aug_onehot', 'pp_aug_elastic_field', 'pp_aug_gaussian_blur')
    assert set(caps) == set(small + large)
    assert all(caps[k] == (4096, 256) for k in small) and all(caps[k] == (8192, 256) for k in large)
    # the loop shapes of the GPU module against these numbers
    assert 5 * 512 * 512 > R.loop_threads('pp_aug_scalar_map') and 17 * (512 * 512 // 4) > R.loop_threads('pp_aug_add_noise')
    assert 9 * 512 * 512 > R.loop_threads('pp_aug_warp') and 2 * 5 * 512 * 512 > R.loop_threads('pp_aug_onehot')
    assert 5 * 2 * 512 * 512 > R.loop_threads('pp_aug_elastic_field') and 9 * 512 * 512 > R.loop_threads('pp_aug_gaussian_blur')


# ------------------------------------------------------------------------------------------ warp: ratio, coverage, mistakes
def _case_launches():
    for s in range(4):
        for r in range(4):
            yield f's{s}r{r}', R.warp_launch(s, r)
    yield 'disp', R.disp_launch()


def _fp32_restatement(L, n, cubic, clip):
    return AO.warp(L['img'][n], L['lab'][n], L['scb'][n], L['maps'][n], R.HO, R.WO, None if L.get('disp') is None else L['disp'][n],
                   None if clip is None else clip[n], R.IMG_PAD, R.K, cubic)


def test_keys_ratio_of_the_fp32_restatement_over_the_case_table(capsys):
    """max |AO.warp - warp64| / (2^-24 mag) over every launch, sample, mode and clip form of the case table: the GPU bound of
    8 * 2^-24 * mag rests on this staying below 4 (the kernel does the same operations in the same order, possibly contracted).
    Class maps, valid and the nearest-neighbour image of the restatement equal the reference's bit for bit."""
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    for name, L in _case_launches():
        for cubic in (0, 1, 2):
            for clip in (None, R.slice_clip(L['img'], L['sizes'])):
                for n, ref in enumerate(R.warp_refs(L, cubic, clip)):
                    v, ol, os_, valid = _fp32_restatement(L, n, cubic, clip)
                    assert np.array_equal(ol, ref['lab']) and np.array_equal(os_, ref['scb']) and np.array_equal(valid, ref['valid'])
                    R.check_warp(dict(img=v, lab=ol, scb=os_, valid=valid), ref, R.IMG_PAD, f'{name}[{n}] cubic={cubic}')
                    k = ref['keep']
                    if k.any():
                        worst[cubic] = max(worst[cubic], float((np.abs(v.astype(np.float64) - ref['v'])[k] / (R.F32_EPS * ref['mag'][k])).max()))
    with capsys.disabled():
        print(f'\n  fp32 restatement / float64, in units of 2^-24 mag: bilinear {worst[0]:.3f}, Keys {worst[1]:.3f}, nearest {worst[2]:.3f}')
    assert worst[2] == 0.0
    assert 0 < worst[1] < 4 and 0 < worst[0] < 4, worst


def test_case_table_has_every_pad_read_class_ties_and_clamps():
    launches = dict(_case_launches())
    table = [L for k, L in launches.items() if k != 'disp']
    for cubic in (0, 1, 2):
        c = R.coverage([r for L in table for r in R.warp_refs(L, cubic)])
        assert c['all_in'] > 0 and c['all_pad'] > 0 and c['outside'] > 0, (cubic, c)
        assert cubic == 2 or c['some_pad'] > 0, (cubic, c)
    # every (map, slice size, rectangle) combination occurs
    combos = {(n, L['sizes'][n], L['rects'][n]) for L in table for n in range(8)}
    assert len(combos) == 8 * 4 * 4
    # ties at exactly .5 inside the slice, in both axes (they must go up)
    ties = 0
    for L in table:
        for r in R.warp_refs(L, 2):
            ties += int((r['keep'] & (((r['ys'] + 0.5) % 1 == 0) | ((r['xs'] + 0.5) % 1 == 0))).sum())
    assert ties > 100
    # the slice's own [min, max] is narrower than the bicubic overshoot at the step edge: both clamps engage; the wide range never
    over = under = 0
    for L in table:
        clip = R.slice_clip(L['img'], L['sizes'])
        for n, r in enumerate(R.warp_refs(L, 1, clip)):
            lo, hi = min(clip[n, 2], R.IMG_PAD), max(clip[n, 3], R.IMG_PAD)
            over += int((r['keep'] & (r['pre'] > hi + 1e-3)).sum())
            under += int((r['keep'] & (r['pre'] < lo - 1e-3)).sum())
            assert (np.abs(r['pre'][r['keep']]) < 1.0e5).all()
    assert over >= 5 and under >= 5, (over, under)
    # displacement: points inside pushed past each of the four edges (clamped), points outside pushed in (not clamped)
    L = launches['disp']
    edge = dict(top=0, bottom=0, left=0, right=0, pushed_in=0)
    for n in range(8):
        m = L['maps'][n].astype(np.float64)
        hs, ws = L['sizes'][n]
        yo, xo = np.mgrid[0:R.HO, 0:R.WO].astype(np.float64)
        ys, xs = m[0] * yo + m[1] * xo + m[2] + L['disp'][n, 0], m[3] * yo + m[4] * xo + m[5] + L['disp'][n, 1]
        r = R.warp64(L['img'][n], L['lab'][n], L['scb'][n], L['maps'][n], R.HO, R.WO, L['disp'][n], None, R.IMG_PAD, R.K, 1)
        i, v = r['inside'], r['valid'] > 0
        edge['top'] += int((v & i & (ys < 0)).sum()); edge['bottom'] += int((v & i & (ys > hs - 1)).sum())
        edge['left'] += int((v & i & (xs < 0)).sum()); edge['right'] += int((v & i & (xs > ws - 1)).sum())
        edge['pushed_in'] += int((v & ~i & r['in_src']).sum())
    assert min(edge.values()) > 0, edge


def test_warp64_refuses_an_undecidable_map():
    L = R.warp_launch(0, 0)
    m = L['maps'][0].copy()
    m[0] = 1.0 / 3.0
    with pytest.raises(ValueError):
        R.warp64(L['img'][0], L['lab'][0], L['scb'][0], m, R.HO, R.WO)


def test_warp_comparator_rejects_planted_mistakes():
    hit = dict(replicate1=0, replicate0=0, tie=0, shift1=0, shift0=0)
    for name, L in _case_launches():
        for n in range(8):
            a = (L['img'][n], L['lab'][n], L['scb'][n], L['maps'][n], R.HO, R.WO, None if L.get('disp') is None else L['disp'][n], None,
                 R.IMG_PAD, R.K)
            for cubic in (1, 0):
                ref, bad = R.warp64(*a, cubic), R.warp64(*a, cubic, mistake='replicate')
                got = dict(img=bad['v'].astype(np.float32), lab=bad['lab'], scb=bad['scb'], valid=bad['valid'])
                R.check_warp(dict(got, img=ref['v'].astype(np.float32)), ref, R.IMG_PAD)
                if np.abs(bad['v'] - ref['v']).max() > 1e-2:   # a padding tap of non-zero weight at a kept pixel: the mistake shows
                    _rejects(R.check_warp, got, ref, R.IMG_PAD)
                    hit[f'replicate{cubic}'] += 1
                bad = R.warp64(*a, cubic, mistake='shift')
                if np.abs(bad['v'] - ref['v']).max() > 1e-2:   # a tap of non-zero weight one pixel past the bottom / right border
                    _rejects(R.check_warp, dict(got, img=bad['v'].astype(np.float32)), ref, R.IMG_PAD)
                    hit[f'shift{cubic}'] += 1
            ref, bad = R.warp64(*a, 2), R.warp64(*a, 2, mistake='tie_down')
            if not (np.array_equal(ref['lab'], bad['lab']) and np.array_equal(ref['scb'], bad['scb'])):
                _rejects(R.check_warp, dict(img=bad['v'].astype(np.float32), lab=bad['lab'], scb=bad['scb'], valid=bad['valid']), ref, R.IMG_PAD)
                hit['tie'] += 1
    assert min(hit['replicate1'], hit['replicate0']) >= 30 and min(hit['shift1'], hit['shift0']) >= 10 and hit['tie'] >= 20, hit
    # one pixel outside the canvas rectangle changed by one ulp; one valid-mask pixel flipped
    L = R.warp_launch(0, 1)
    n = 0
    assert L['rects'][n] == R.RECTS[1]
    ref = R.warp_refs(L, 1)[n]
    good = dict(img=ref['v'].astype(np.float32), lab=ref['lab'], scb=ref['scb'], valid=ref['valid'])
    R.check_warp(good, ref, R.IMG_PAD)
    img = good['img'].copy()
    img[0, 0] = np.nextafter(img[0, 0], np.float32(0))
    _rejects(R.check_warp, dict(good, img=img), ref, R.IMG_PAD)
    valid = good['valid'].copy()
    valid[1, 3] = 1
    _rejects(R.check_warp, dict(good, valid=valid), ref, R.IMG_PAD)
    # an image 12 * 2^-24 * mag away at one kept pixel
    y, x = np.argwhere(ref['keep'])[0]
    img = good['img'].copy()
    img[y, x] += np.float32(12 * R.F32_EPS * ref['mag'][y, x])
    _rejects(R.check_warp, dict(good, img=img), ref, R.IMG_PAD)


# ------------------------------------------------------------------------------------------ spline path
def test_spline_reference_is_decidable_covers_every_edge_and_matches_the_restatement():
    L = R.spline_launch()
    for n, (hs, ws) in enumerate(L['sizes']):
        ref = R.spline_ref(L, n)
        for c in ref['coords']:                      # no class-map decision hangs on a float64 contraction
            assert np.abs((c + 0.5) - np.round(c + 0.5)).min() > 1e-9
        yo, xo = np.mgrid[0:R.HP, 0:R.WP]
        ins = (yo < hs) & (xo < ws)
        yu, xu = yo + L['disp64'][n, 0], xo + L['disp64'][n, 1]
        if hs > 1 and ws > 2:
            assert (ins & (yu < 0)).any() and (ins & (yu > hs - 1)).any() and (ins & (xu < 0)).any() and (ins & (xu > ws - 1)).any()
        if n:                                        # a small slice: points outside it pushed in and left outside
            assert (~ins & ref['in_src']).any() and (~ins & ~ref['in_src']).any()
        v, ol, os_, valid = AO.warp(L['img'][n], L['lab'][n], L['scb'][n], L['maps'][n], R.HP, R.WP, L['disp64'][n], L['clip'][n],
                                    R.IMG_PAD, R.K, 1, spline=True)
        got = dict(img=v, lab=ol, scb=os_, valid=valid)
        R.check_spline(got, ref, f'sample {n}')
        # planted: a coefficient never written; the coordinates moved by 2^-12 px
        bad = v.copy()
        bad[hs // 2, ws // 2] = np.nan
        _rejects(R.check_spline, dict(got, img=bad), ref)
        if hs > 1:
            moved = dict(L, disp64=L['disp64'] + 2.0 ** -12)
            _rejects(R.check_spline, dict(got, img=R.spline_ref(moved, n)['v'].astype(np.float32)), ref)
    lab = R.spline_ref(L, 0)['lab'].copy()
    lab[3, 3] += 1
    _rejects(R.check_spline, dict(got, lab=lab), R.spline_ref(L, 3))


# ------------------------------------------------------------------------------------------ Philox
def test_single_sample_normal_field_is_a_row_of_the_batch_field():
    for HW in (35, 64):
        full = AO.normal_field(5, HW, 0x1234567890)
        for n in (0, 3, 4):
            assert np.array_equal(R.normal_sample(n, HW, 0x1234567890), full[n])
    x = np.zeros((3, 5, 7), np.float32)
    ref = R.noise_ref(x, 1, 0.5, (1, 2, 3, 4), 99)
    R.check_noise(ref.astype(np.float32), ref, 0.5)
    assert (ref[R.rect_mask((1, 2, 3, 4), 5, 7)] != 0).all() and (ref[~R.rect_mask((1, 2, 3, 4), 5, 7)] == 0).all()
    _rejects(R.check_noise, R.noise_ref(x, 2, 0.5, (1, 2, 3, 4), 99).astype(np.float32), ref, 0.5)      # the neighbour's counter


# ------------------------------------------------------------------------------------------ elementwise maps
def test_elementwise_references_and_comparator():
    rng = np.random.RandomState(3)
    x = (rng.normal(size=(7, 9)) * 20 + 50).astype(np.float32)
    c, rect = np.array([1.5, -3.0, 10.0, 90.0], np.float32), (1, 1, 5, 7)
    ref = R.scalar_map64(x, c, rect)
    np.testing.assert_allclose(AO.scalar_map(x, c, rect), ref, rtol=1e-6)
    g = np.array([x.min(), x.max() - x.min() + 1e-8, 0.7, 0], np.float32)
    np.testing.assert_allclose(AO.gamma_map(x, g), R.gamma_map64(x, g), rtol=1e-5)
    assert np.array_equal(R.gamma_map64(x, np.array([0, 1, -1, 0], np.float32)), x.astype(np.float64))
    assert np.array_equal(R.mix64(x, x + 1, -1.0), x.astype(np.float64))
    touched = R.rect_mask(rect, 7, 9)
    good = ref.astype(np.float32)
    R.check_elementwise(good, ref, x, touched)
    bad = good.copy()
    bad[0, 8] = np.nextafter(bad[0, 8], np.float32(1e9))                  # one pixel outside the rectangle, one ulp
    _rejects(R.check_elementwise, bad, ref, x, touched)
    bad = good.copy()
    bad[3, 3] *= np.float32(1 + 1e-4)
    _rejects(R.check_elementwise, bad, ref, x, touched)


# ------------------------------------------------------------------------------------------ Gaussian filters
BLUR_CASES = (((1, 7), 2.0), ((7, 1), 2.0), ((3, 5), 2.0), ((2, 2), 3.0), ((37, 53), 1.7), ((9, 4), 0.1), ((9, 4), 0.124),
              ((9, 4), 0.126))


def _gauss_fp32(x, sigma, axis):
    """aug_gauss_pass_kernel in numpy fp32: weights exp(-k^2 / (2 sigma^2)), 'reflect' index, normalised by the weight sum."""
    f = np.float32
    n, rad = x.shape[axis], R.gauss_radius(sigma)
    inv = f(-0.5) / (f(sigma) * f(sigma))
    acc, wsum = np.zeros(x.shape, f), f(0)
    for k in range(-rad, rad + 1):
        w = np.exp(inv * f(k) * f(k)).astype(f)
        i = (np.arange(n) + k) % (2 * n)
        i = np.where(i < n, i, 2 * n - 1 - i)
        acc, wsum = acc + w * np.take(x, i, axis), wsum + w
    return (acc / wsum).astype(f)


def test_gaussian_references_radius_and_planted_mistakes(capsys):
    assert [R.gauss_radius(s) for s in (0.1, 0.124, 0.126, 1.0, 1.7, 2.0, 3.0)] == [0, 0, 1, 4, 7, 8, 12]
    rng = np.random.RandomState(5)
    worst = 0.0
    for (H, W), sg in BLUR_CASES:
        x = rng.normal(size=(H, W)).astype(np.float32)
        ref = R.blur64(x, sg)
        got = _gauss_fp32(_gauss_fp32(x, sg, 0), sg, 1)
        worst = max(worst, float(np.abs(got - ref).max()))
        R.check_blur(got, ref, x, sg, f'{H}x{W} sigma {sg}')
    with capsys.disabled():
        print(f'\n  fp32 restatement of the separable Gaussian against scipy over the blur cases: {worst:.2e}')
    assert worst < 2e-7
    assert any(R.gauss_radius(sg) > 2 * min(s) for s, sg in BLUR_CASES) and any(min(s) == 1 for s, _ in BLUR_CASES)
    # planted on the blur comparator: 'mirror' for 'reflect'; a radius of 1 where 0 is required does not return the input bits
    x = rng.normal(size=(37, 53)).astype(np.float32)
    _rejects(R.check_blur, R.blur64(x, 1.7, mode='mirror').astype(np.float32), R.blur64(x, 1.7), x, 1.7)
    x = rng.normal(size=(9, 4)).astype(np.float32)
    smeared = scipy.ndimage.gaussian_filter(x.astype(np.float64), 0.3).astype(np.float32)
    _rejects(R.check_blur, smeared, R.blur64(x, 0.124), x, 0.124)
    # planted on the field comparator (alpha = 150): radius + 1, 'mirror'
    sa = np.array([[1.7, 150.0], [0.0, 0.0], [2.0, 40.0]], np.float32)
    ref = R.field64(3, 37, 53, sa, 4242)
    R.check_field(ref.astype(np.float32), ref, sa)
    assert np.abs(AO.device_elastic_field(3, 37, 53, sa, 4242) - ref).max() < 1e-4
    _rejects(R.check_field, R.field64(3, 37, 53, sa, 4242, extra_radius=1).astype(np.float32), ref, sa)
    _rejects(R.check_field, R.field64(3, 37, 53, sa, 4242, mode='mirror').astype(np.float32), ref, sa)
    notzero = ref.astype(np.float32)
    notzero[1, 0, 5, 5] = 1e-30
    _rejects(R.check_field, notzero, ref, sa)


# ------------------------------------------------------------------------------------------ scribble synthesis
def test_scribble_references_and_planted_mistakes():
    # the five skeleton launches cover the seven contents between them; 280 x 280 has the all-ones image
    kinds = [R.skeleton_masks(i, 9, 9)[0] for i in range(5)]
    assert {k for ks in kinds for k in ks} == set(R.MASK_CONTENTS) and 'ones' in kinds[2] and all(len(set(ks)) == 5 for ks in kinds)
    _, masks = R.skeleton_masks(0, 37, 53)
    sk = R.skeleton_ref(masks)
    assert sk.dtype == np.uint8 and (sk <= masks).all() and sk[0].sum() > 0 and sk[1].sum() == 0 and sk[2].sum() == 1
    R.check_masks(sk, sk)
    _rejects(R.check_masks, sk[[1, 0, 2, 3, 4]], sk)                       # a mask swapped with its neighbour in the batch
    for H, W in ((1, 9), (9, 1)):                                          # degenerate images: a line is its own skeleton
        line = R.skeleton_ref(np.ones((1, H, W), np.uint8))
        assert line.sum() == 9
    # dilation: a seed outside the mask stays; one step too many fails
    seeds, dm = R.dilation_case(37, 53)
    assert (seeds[2][dm[2] == 0]).sum() == 2 and (seeds[0].sum(), seeds[1].sum()) == (4, 3)
    for it in (0, 1, 40):
        ref = R.dilation_ref(seeds, dm, it)
        assert (ref[seeds != 0] == 1).all() and (ref[(dm == 0) & (seeds == 0)] == 0).all()
    assert np.array_equal(R.dilation_ref(seeds, dm, 0), seeds)
    one = R.dilation_ref(seeds, dm, 1)
    assert one[0, 1, 51] == 1 and one[0, 35, 1] == 1 and one[0].sum() == 6          # corners: only the anti-diagonal neighbours join
    _rejects(R.check_masks, R.dilation_ref(seeds, dm, 2), one)
    big = [a[:1] for a in R.dilation_case(256, 256)]                        # 40 steps have not converged on the real slice size
    _rejects(R.check_masks, R.dilation_ref(*big, 41), R.dilation_ref(*big, 40))
    # end points: by hand on the 5 x 7 curves
    c = R.curves(5, 7)
    ep = R.endpoints_ref(c)
    assert ep[2].sum() == 0                                                # a closed loop has none
    assert ep[1, 4, 6] == 0 and ep[1, 2, 0] == 1 and ep[1, 0, 2] == 1 and ep[1, 2, 4] == 1 and ep[1].sum() == 3
    assert ep[0, 0, 0] == 1 and ep[0, 4, 6] == 1
    missed = ep.copy()
    missed[0, 0, 0] = 0                                                    # the end point in the corner missed
    _rejects(R.check_masks, missed, ep)


def test_scribble_lds_budget_and_argument_checks():
    """The size pp_skeletonize promises (280 x 280) and the largest it admits fit 160 KB with the kernel's 4 static bytes; one size
    above is refused by the argument check, before any launch -- so this runs without a GPU, with a pointer that is never read."""
    import ctypes
    from pacingpseudo_amd import _lib
    assert R.scribble_lds(256, 256) > 64 * 1024                            # the real slices are on the large-LDS path
    assert R.scribble_lds(280, 280) == 159052 <= R.LDS_BYTES
    big = R.SK_LARGEST_SQUARE
    assert 2 * (big + 2) ** 2 <= R.LDS_BYTES - 64 < 2 * (big + 3) ** 2 and R.scribble_lds(big, big) <= R.LDS_BYTES
    assert os.path.exists(_lib.LIB_PATH), 'library not built (run __graft_entry__.build()): the argument checks cannot be tested'
    # The wrap cases are safe only because the check refuses them before any HIP call: the 64-byte host buffer is never read.  If
    # the check regressed, pp_skeletonize(65534, 65534) would launch with 0 bytes of LDS -- without a GPU that is a launch error,
    # on a GPU machine a memory fault, not an assertion; do not widen this list without reading the check.
    buf = ctypes.create_string_buffer(b'\x01' * 64)
    p = ctypes.addressof(buf)
    # 65534 + 2 = 2^16: a 32-bit (H + 2)(W + 2) wraps round to 0 and would pass
    for H, W in ((big + 1, big + 1), (1, 27295), (0, 5), (5, 0), (65534, 65534), (46340, 46340)):
        with pytest.raises(_lib.HipLibraryError, match='skeletonize'):
            _lib.lib.pp_skeletonize(p, 1, H, W, None)
        with pytest.raises(_lib.HipLibraryError, match='dilate_antidiagonal'):
            _lib.lib.pp_dilate_antidiagonal(p, p, 1, H, W, 1, None)
    assert buf.raw[:64] == b'\x01' * 64
