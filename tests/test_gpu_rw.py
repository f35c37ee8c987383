"""Random-walker expansion of scribbles on the MI355X (libpacingpseudo_prep.so, utils/random_walker.py, --rw_scribbles) against the
float64 sparse direct solve of tests/_rw_reference.py.

PROB_TOL bounds max |prob - oracle|.  The solver stops at a relative residual of 1e-6 in fp32, so the deviation is set by the
conditioning of the slice's Laplacian, not by the number format alone; it was therefore MEASURED once on the MI355X on the three
cases of test_against_the_oracle and set to twice the largest deviation seen, rounded up to one significant digit (the figures stand
beside the constant and in DESIGN.md section 7).  test_padding_and_odd_shapes holds its slices to the same constant.

The degenerate slices and the class counts (tests 4 and 5) are cases of this file's own making, and PROB_TOL says nothing about them:
  * on some of them the definition's stopping rule itself -- the same iteration carried out in float64 on the CPU,
    tests/_rw_reference.truncation_error -- stops further from the direct solve than PROB_TOL: 16 x 16 with seeds on all four
    borders, class 2: 1.71e-3 in float64 (the MI355X gave 1.61e-3 there); K = 32 with one seed per class: 1.75e-3;
  * one of them is far worse conditioned than the phantoms: K = 1 has a single seed for 255 unknowns, the smallest eigenvalue of its
    Laplacian is 4.8e-6 (phantoms: 4.7e-5 .. 9.3e-5), and fp32 rounding, amplified by its inverse, moved the MI355X 9.6e-4 from the
    direct solve where the float64 iteration stops 2.6e-6 from it (a float32 numpy emulation of the iteration: 3.9e-4).
Their bound is therefore that truncation error, a float64 property of the slice that no kernel enters, plus DEVICE_CEILING = 1e-3:
the most the device may add before the solver counts as defective, whatever the case.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _rw_reference as R
from tests._guard import BandSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured on the MI355X, 32 x 32 K = 5 phantoms, default parameters: max |prob - oracle| = 2.776e-4 (seed 0), 2.589e-4 (seed 1),
# 9.469e-5 (seed 2); twice the largest = 5.55e-4, rounded up to one significant digit
PROB_TOL = 6e-4
DEVICE_CEILING = 1e-3
DEV = 'cuda'


def _dev(img, scb, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(scb)).to(DEV).to(dtype)


@pytest.fixture(scope='module')
def phantoms():
    """The three 32 x 32 K = 5 phantoms with their oracle probabilities, computed once."""
    cases = []
    for seed in (0, 1, 2):
        img, lab, scb = R.phantom(seed, 32, 5)
        cases.append(dict(img=img, lab=lab, scb=scb, prob=R.rw_prob(img, scb, 5)))
    img, scb = _dev(np.stack([c['img'] for c in cases]), np.stack([c['scb'] for c in cases]))
    return cases, img, scb


def _image(seed, h, w):
    """An h x w window of a phantom image (K = 3 structures on noise)."""
    return R.phantom(seed, max(h, w, 16), 3)[0][:h, :w].copy()


def _random_case(h, w, K, seed, classes=None):
    rng = np.random.default_rng(seed)
    img = _image(seed, h, w)
    scb = np.full((h, w), K, np.int64)
    flat = rng.permutation(h * w)
    for j, k in enumerate(range(K) if classes is None else classes):
        scb.flat[flat[2 * j]] = k
        scb.flat[flat[2 * j + 1]] = k
    return img, scb


def _planes(cases, H, W, K):
    """Slices of different sizes in the top-left corners of one (N, H, W) plane pair: image padding 0, scribble padding K."""
    img = np.zeros((len(cases), H, W), np.float32)
    scb = np.full((len(cases), H, W), K, np.int64)
    for n, (i, s) in enumerate(cases):
        h, w = s.shape
        img[n, :h, :w], scb[n, :h, :w] = i, s
    return img, scb, [s.shape for _, s in cases]


def _check_against_oracle(prob, labels, stats, cases, K, tau, truncation=False):
    """`truncation`: the bound per class is DEVICE_CEILING plus what the stopping rule leaves in float64 (the module docstring says
    why); else PROB_TOL."""
    prob, labels = prob.cpu().numpy(), labels.cpu().numpy()
    for n, (img, scb) in enumerate(cases):
        h, w = scb.shape
        ref = R.rw_prob(img, scb, K)
        dev = np.abs(prob[n, :, :h, :w] - ref).reshape(K, -1).max(1)
        bound = DEVICE_CEILING + R.truncation_error(img, scb, K) if truncation else np.full(K, PROB_TOL)
        print(f'slice {n} ({h} x {w}, K = {K}): max |prob - oracle| = {dev.max():.3e}' + (f', largest float64 truncation {bound.max() - DEVICE_CEILING:.3e}' if truncation else ''))
        assert (dev <= bound).all(), (n, dev.tolist(), bound.tolist())
        assert not prob[n, :, h:, :].any() and not prob[n, :, :, w:].any()
        assert (labels[n, h:, :] == K).all() and (labels[n, :, w:] == K).all()
        # a label may differ where the oracle is within 1e-3 of a tie or of the threshold (twice the bound where that is larger:
        # two classes may each move by it)
        keep = ~R.undecided(ref, tau, max(1e-3, 2 * float(bound.max())) if truncation else 1e-3)
        assert np.array_equal(labels[n, :h, :w][keep], R.rw_labels(ref, scb, K, tau)[keep]), n
        assert np.array_equal(labels[n, :h, :w][scb < K], scb[scb < K])
        for k in range(K):
            if not (scb == k).any():
                assert not prob[n, k].any() and stats[n, k].tolist() == [0.0, 0.0, 1.0], (n, k)
            else:
                assert stats[n, k, 2] == 1.0, (n, k, stats[n, k].tolist())


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_oracle(phantoms):
    from pacingpseudo_amd.utils import random_walker
    cases, img, scb = phantoms
    prob, stats = random_walker(img, scb, 5, return_stats=True)
    assert prob.shape == (3, 5, 32, 32) and prob.dtype == torch.float32 and stats.shape == (3, 5, 3)
    prob4 = random_walker(img[:, None], scb, 5)                              # (N, 1, H, W) images are the same call
    assert torch.equal(prob, prob4)
    prob, stats = prob.cpu().numpy(), stats.cpu().numpy()
    for n, c in enumerate(cases):
        dev = float(np.abs(prob[n] - c['prob']).max())
        print(f'phantom seed {n}: max |prob - oracle| = {dev:.3e}, iterations {stats[n, :, 0].tolist()}, true residual {stats[n, :, 1].tolist()}')
        assert dev <= PROB_TOL, (n, dev)
    seeded = np.array([[(c['scb'] == k).any() for k in range(5)] for c in cases])
    assert (stats[:, :, 2] == 1).all() and (stats[:, :, 0][seeded] >= 1).all() and (stats[:, :, 0][~seeded] == 0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', [0.5, 0.9])
def test_labels_equal_the_oracles(phantoms, tau):
    from pacingpseudo_amd.utils import expand_scribbles
    cases, img, scb = phantoms
    labels = expand_scribbles(img, scb, 5, None, tau)
    assert labels.dtype == scb.dtype and labels.shape == scb.shape
    assert expand_scribbles(img, scb.to(torch.uint8), 5, None, tau).dtype == torch.uint8
    labels = labels.cpu().numpy()
    for n, c in enumerate(cases):
        out = R.undecided(c['prob'], tau) & (c['scb'] == 5)
        print(f'phantom seed {n}, threshold {tau}: {100 * out.mean():.2f} % of the pixels left out')
        assert out.mean() <= 0.02
        assert np.array_equal(labels[n][~out], R.rw_labels(c['prob'], c['scb'], 5, tau)[~out]), n


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_padding_and_odd_shapes():
    from pacingpseudo_amd.utils import expand_scribbles
    K, H, W = 3, 40, 48
    cases = []
    for seed, (h, w) in zip((3, 4, 5), ((33, 17), (20, 41), (40, 48))):
        img, _, scb = R.phantom(seed, 48, K)
        ys, xs = np.nonzero(scb < K)                                         # a window of the phantom that keeps its strokes
        y0, x0 = min(max(int(ys.min()) - 2, 0), 48 - h), min(max(int(xs.min()) - 2, 0), 48 - w)
        cases.append((img[y0:y0 + h, x0:x0 + w].copy(), scb[y0:y0 + h, x0:x0 + w].copy()))
        assert len(np.unique(cases[-1][1])) >= 3                             # two seeded classes and unknowns
    img, scb, sizes = _planes(cases, H, W, K)
    a = expand_scribbles(*_dev(img, scb), K, sizes, 0.9, return_stats=True, return_prob=True)
    _check_against_oracle(a[2], a[0], a[1].cpu().numpy(), cases, K, 0.9)
    # what lies outside h x w is never read: NaN in the image padding, seeds in the scribble padding, the same bits
    img2, scb2 = np.full_like(img, np.nan), np.zeros_like(scb)
    for n, (h, w) in enumerate(sizes):
        img2[n, :h, :w], scb2[n, :h, :w] = img[n, :h, :w], scb[n, :h, :w]
    b = expand_scribbles(*_dev(img2, scb2), K, sizes, 0.9, return_stats=True, return_prob=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_slices_beside_a_normal_one():
    from pacingpseudo_amd.utils import expand_scribbles
    K, S = 3, 16
    rng = np.random.default_rng(11)
    normal = _random_case(S, S, K, 20)
    no_class2 = _random_case(S, S, K, 21, classes=(0, 1))
    no_seed = (_image(22, S, S), np.full((S, S), K, np.int64))
    all_seeded = (_image(23, S, S), rng.integers(0, K, (S, S)))
    one_unknown = (_image(24, S, S), rng.integers(0, K, (S, S)))
    one_unknown[1][5, 7] = K
    row = (np.full((1, 7), 2.0, np.float32), np.array([[0, K, K, K, K, K, 1]]))
    col = (_image(25, 7, 1), np.array([[2, K, K, K, K, K, 0]]).T.copy())
    tiny = (_image(26, 2, 2), np.array([[0, K], [K, 1]]))
    border = (_image(27, S, S), np.full((S, S), K, np.int64))
    border[1][0, :], border[1][-1, :], border[1][1:-1, 0], border[1][1:-1, -1] = 0, 1, 2, 0
    cases = [normal, no_class2, no_seed, all_seeded, one_unknown, row, col, tiny, border]
    img, scb, sizes = _planes(cases, S, S, K)
    labels, stats, prob = expand_scribbles(*_dev(img, scb), K, sizes, 0.9, return_stats=True, return_prob=True)
    stats = stats.cpu().numpy()
    _check_against_oracle(prob, labels, stats, cases, K, 0.9, truncation=True)
    p, lab = prob.cpu().numpy(), labels.cpu().numpy()
    assert not p[1, 2].any() and stats[1, 2].tolist() == [0, 0, 1] and stats[1, 0, 0] >= 1          # a class without seeds
    assert not p[2].any() and (lab[2] == K).all() and (stats[2] == [0, 0, 1]).all()                 # no seeds at all
    assert np.array_equal(lab[3], all_seeded[1]) and (stats[3, :, 0] == 0).all() and (stats[3, :, 2] == 1).all()
    for k in range(K):
        assert np.array_equal(p[3, k], (all_seeded[1] == k).astype(np.float32))                     # output = input, no iteration
    assert stats[4, :, 0].max() <= 1                                                                # one unknown: one step at most
    assert np.abs(p[5, 1, 0, :7] - np.arange(7) / 6.0).max() <= PROB_TOL                            # the chain's linear ramp


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 32])
def test_class_counts(K):
    from pacingpseudo_amd.utils import expand_scribbles
    rng = np.random.default_rng(K)
    img = _image(30 + K, 16, 16)
    scb = np.full((16, 16), K, np.int64)
    scb.flat[rng.permutation(256)[:K]] = np.arange(K)                        # one seed per class
    labels, stats, prob = expand_scribbles(*_dev(img[None], scb[None]), K, None, 0.5, return_stats=True, return_prob=True)
    _check_against_oracle(prob, labels, stats.cpu().numpy(), [(img, scb)], K, 0.5, truncation=True)
    if K == 1:                                                               # the direct solve is 1 everywhere
        assert (labels == 0).all()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_reproducible_alone_in_a_batch_and_on_a_side_stream(phantoms):
    from pacingpseudo_amd.utils import expand_scribbles
    _, img, scb = phantoms
    kw = dict(return_stats=True, return_prob=True)
    a = expand_scribbles(img, scb, 5, **kw)
    b = expand_scribbles(img, scb, 5, **kw)
    alone = expand_scribbles(img[1:2].contiguous(), scb[1:2].contiguous(), 5, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = expand_scribbles(img, scb, 5, **kw)
    side.synchronize()
    for x, y, z, one in zip(a, b, c, alone):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x[1:2], one)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_iteration_cap_and_the_reported_residual(phantoms):
    from pacingpseudo_amd.utils import random_walker
    cases, img, scb = phantoms
    prob, stats = random_walker(img[:1].contiguous(), scb[:1].contiguous(), 5, max_iters=3, return_stats=True)
    prob, stats = prob.cpu().numpy()[0], stats.cpu().numpy()[0]
    c = cases[0]
    for k in range(5):
        if not (c['scb'] == k).any():
            assert stats[k].tolist() == [0, 0, 1]
            continue
        assert stats[k, 0] == 3 and stats[k, 2] == 0 and stats[k, 1] > 1e-6, stats[k].tolist()
        ref = R.relres(c['img'], c['scb'], 5, k, prob[k])
        print(f'class {k}: reported true residual {stats[k, 1]:.6e}, recomputed in float64 {ref:.6e}')
        assert abs(stats[k, 1] - ref) <= 1e-3 * ref, (k, stats[k, 1], ref)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_sentinel_bands(phantoms):
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._prep import prep
    from pacingpseudo_amd.utils import expand_scribbles
    _, img, scb = phantoms
    N, K, H, W = 3, 5, 32, 32
    sizes = [(32, 32), (29, 31), (32, 17)]
    import ctypes
    host = np.ascontiguousarray(np.asarray(sizes, np.int32))
    hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    want = expand_scribbles(img, scb, K, sizes, return_stats=True, return_prob=True)
    got = []
    for pattern in (0xFF, 0xA5):
        bs = BandSet(pattern, DEV)
        g_img, g_scb = bs.tensor(img, label='img'), bs.tensor(scb.to(torch.int32), label='scb')
        prob, stats = bs.banded((N, K, H, W), torch.float32, 'prob'), bs.banded((N, K, 3), torch.float32, 'stats')
        out = bs.banded((N, H, W), torch.int32, 'labels')
        ws = bs.ws(prep.pprep_rw_workspace_bytes(N, K, H, W), 'workspace')
        prep.pprep_rw_solve(g_img.data_ptr(), g_scb.data_ptr(), hp, N, K, H, W, 13.0, 1e-4, 1e-6, 10000, prob.ptr(), stats.ptr(), ws.ptr(),
                            stream_ptr())
        prep.pprep_rw_labels(prob.ptr(), g_scb.data_ptr(), hp, N, K, H, W, 0.9, out.ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert bs.damaged() == []
        got.append((out.t.clone(), stats.t.clone(), prob.t.clone()))
    for x, y, w_ in zip(got[0], got[1], want):
        assert torch.equal(x, y) and torch.equal(x.to(w_.dtype), w_)        # nothing stale read, nothing left unwritten
    assert bool(torch.isfinite(got[0][2]).all())


# 9 ---------------------------------------------------------------------------------------------------------------------------
DRIVER = ['--synthetic', '8', '--image_size', '32', '--epoch', '2', '--batch_size', '4', '--num_workers', '0', '--init_ch', '8',
          '--max_ch', '64']


def test_driver_expands_once_and_resumes_bit_for_bit(tmp_path):
    from tests.test_gpu_resume import _load, _resume_case, _run, _scalars
    full, resumed, _ = _resume_case(tmp_path, 'train_chaos.py', DRIVER + ['--rw_scribbles'], 0, 1, session='Control')
    log = open(os.path.join(full, 'log.txt')).read()
    line = [ln for ln in log.splitlines() if 'random-walker scribbles: 8 slices' in ln]
    assert len(line) == 1 and 'coverage' in line[0] and 'agreement' in line[0] and '0 unconverged systems' in line[0], log[-2000:]
    z = np.load(os.path.join(full, 'rw_scribbles.npz'))
    assert z['iterations'].shape == (8, 5) and z['converged'].all() and (z['coverage_after'] > z['coverage_before']).all()
    z2 = np.load(os.path.join(resumed, 'rw_scribbles.npz'))                  # recomputed by the resumed process: the same bits
    assert all(np.array_equal(z[k], z2[k], equal_nan=True) for k in z.files)
    sc = _scalars(full)
    assert sc[('RW/coverage', 0)] == pytest.approx(float(z['coverage_after'].mean())) and ('RW/agreement', 0) in sc
    # without the flag: the parent's path -- no expansion, no file, no scalar -- and another training run
    plain = _run('train_chaos.py', DRIVER, tmp_path / 'plain', 'p', session='Control')
    assert not os.path.exists(os.path.join(plain, 'rw_scribbles.npz')) and 'random-walker' not in open(os.path.join(plain, 'log.txt')).read()
    assert not any(tag.startswith('RW/') for tag, _ in _scalars(plain))
    a, b = _load(os.path.join(full, 'ckps', 'ckp_1.pth')), _load(os.path.join(plain, 'ckps', 'ckp_1.pth'))
    assert any(not torch.equal(a[k], b[k]) for k in a)


def test_expanded_planes_reach_the_model():
    """The data set the driver builds, with the override the driver computes: the scribble planes of the batches it hands to the
    model label more pixels than without the flag, on the GPU-augmentation path and on the --cpu_input path."""
    from pacingpseudo_amd.augment import AugConfig, DeviceAugmenter, collate_raw
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import check_rw_params
    from pacingpseudo_amd.utils.random_walker import expand_dataset
    K, S = 5, 32
    counts = {}
    for raw in (True, False):
        ds = SyntheticPhantoms(8, K, size=S, raw=raw, seed=1)
        maps, rep = expand_dataset(ds, K, torch.device(DEV), check_rw_params(K=K))
        assert all(m.dtype == np.uint8 and m.shape == (S, S) for m in maps) and (rep['coverage_after'] > rep['coverage_before']).all()
        for on in (False, True):
            ds.scribble_override = maps if on else None
            items = [ds[i] for i in range(8)]
            if raw:
                batch = collate_raw(items)
                aug = DeviceAugmenter(AugConfig(num_classes=K, crop_size=(S, S)), device=DEV, seed=3)
                scribble = aug(batch['img'], batch['lab'], batch['scb'], batch['sizes'])['scribble']
            else:
                scribble = torch.stack([it['scribble'] for it in items])
            assert scribble.shape == (8, K + 1, S, S)
            counts[raw, on] = float(scribble[:, :K].sum())
    assert counts[True, True] > 2 * counts[True, False] > 0 and counts[False, True] > 2 * counts[False, False] > 0, counts


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_tool_writes_what_expand_scribbles_returns(tmp_path):
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import expand_scribbles
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'expand_scribbles.py'), '--synthetic', '4', '--image_size', '32',
                        '--out', str(tmp_path / 'rw')], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'random-walker scribbles: 4 slices' in r.stdout
    files = sorted(glob.glob(str(tmp_path / 'rw' / '*.npz')))
    assert len(files) == 4
    ds = SyntheticPhantoms(4, 5, size=32, raw=True)
    raw = [ds.raw_arrays(i) for i in range(4)]
    labels, prob = expand_scribbles(*_dev(np.stack([x[0] for x in raw]), np.stack([x[2] for x in raw])), 5, return_prob=True)
    for i, f in enumerate(files):
        z = np.load(f)
        assert set(z.files) == {'uid', 'img', 'lab', 'scb', 'scb_orig', 'rw_maxprob'}
        assert np.array_equal(z['scb'], labels[i].cpu().numpy()) and np.array_equal(z['scb_orig'], raw[i][2])
        assert np.array_equal(z['img'], raw[i][0]) and np.array_equal(z['lab'], raw[i][1])
        assert z['rw_maxprob'].dtype == np.float16 and np.array_equal(z['rw_maxprob'], prob[i].amax(0).to(torch.float16).cpu().numpy())
