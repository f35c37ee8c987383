"""Random walker with priors on the MI355X (libpacingpseudo_rwp.so, utils.random_walker_prior / refresh_scribbles / refresh_dataset,
train_chaos.py --rw_refresh) against the float64 sparse direct solve of tests/_rw_prior_reference.py.

PROB_TOL bounds max |prob - oracle| on the three 32 x 32 K = 5 phantoms with their test prior at gamma = 0.01, 0.1 and 1.0.  As in
tests/test_gpu_rw.py it was MEASURED once on the MI355X and set to twice the largest deviation seen, rounded up to one significant
digit (the figures stand beside the constant and in DESIGN.md section 7); test 1 also checks that it is never above the float64
truncation error of the stopping rule for the case plus DEVICE_CEILING = 1e-3.

The slices of this file's own making (classes without seeds, odd shapes, K = 1 / 2 / 32) are held to that truncation error -- the
same iteration carried out in float64, tests/_rw_prior_reference.truncation_error, a property of the slice that no kernel enters --
plus DEVICE_CEILING, as tests/test_gpu_rw.py holds its own: PROB_TOL was measured on the phantoms and says nothing about them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _rw_prior_reference as P
from tests import _rw_reference as R
from tests._guard import BandSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMAS = (0.01, 0.1, 1.0)
# measured on the MI355X, 32 x 32 K = 5 phantoms with the test prior, default parameters: max |prob - oracle| for seeds 0 / 1 / 2 at
# gamma 0.01: 6.490e-6 / 3.900e-6 / 4.783e-6 (91 - 119 iterations); gamma 0.1: 1.330e-6 / 1.093e-6 / 1.004e-6 (39 - 44); gamma 1.0:
# 9.478e-7 / 2.153e-6 / 9.302e-7 (15 - 16).  Twice the largest = 1.30e-5, rounded up to one significant digit.  Most of it is the
# stopping rule: the same iteration in float64 stops 6.90e-6 from the direct solve on seed 0 at gamma 0.01.
PROB_TOL = 2e-5
DEVICE_CEILING = 1e-3
DEV = 'cuda'


def _dev(img, scb, z, dtype=torch.int64):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t(np.asarray(img, dtype=np.float32)), t(scb).to(dtype), t(np.asarray(z, dtype=np.float32))


@pytest.fixture(scope='module')
def phantoms():
    """The three 32 x 32 K = 5 phantoms with their test prior and the oracle's probabilities per gamma, computed once."""
    cases = []
    for seed in (0, 1, 2):
        img, lab, scb = R.phantom(seed, 32, 5)
        z = P.prior_logits(seed, lab, 5)
        cases.append(dict(img=img, lab=lab, scb=scb, z=z, prob={g: P.rw_prob(img, scb, z, 5, g) for g in GAMMAS}))
    return (cases,) + _dev(np.stack([c['img'] for c in cases]), np.stack([c['scb'] for c in cases]), np.stack([c['z'] for c in cases]))


def _image(seed, h, w):
    """An h x w window of a phantom image (K = 3 structures on noise)."""
    return R.phantom(seed, max(h, w, 16), 3)[0][:h, :w].copy()


def _planes(cases, H, W, K):
    """Slices of different sizes in the top-left corners of one (N, H, W) plane set: image and logits padding 0, scribble padding K."""
    img = np.zeros((len(cases), H, W), np.float32)
    scb = np.full((len(cases), H, W), K, np.int64)
    z = np.zeros((len(cases), K, H, W), np.float32)
    for n, (i, s, l) in enumerate(cases):
        h, w = s.shape
        img[n, :h, :w], scb[n, :h, :w], z[n, :, :h, :w] = i, s, l
    return img, scb, z, [s.shape for _, s, _ in cases]


def _check_own_cases(prob, labels, stats, cases, K, gamma, tau):
    """Slices of this file's own making: per class within DEVICE_CEILING + the float64 truncation error of the stopping rule."""
    prob, labels, stats = prob.cpu().numpy(), labels.cpu().numpy(), stats.cpu().numpy()
    for n, (img, scb, z) in enumerate(cases):
        h, w = scb.shape
        ref = P.rw_prob(img, scb, z, K, gamma)
        dev = np.abs(prob[n, :, :h, :w] - ref).reshape(K, -1).max(1)
        trunc = P.truncation_error(img, scb, z, K, gamma)
        print(f'slice {n} ({h} x {w}, K = {K}, gamma = {gamma}): max |prob - oracle| = {dev.max():.3e}, largest float64 truncation {trunc.max():.3e}, '
              f'iterations up to {int(stats[n, :, 0].max())}')
        assert (dev <= DEVICE_CEILING + trunc).all(), (n, dev.tolist(), trunc.tolist())
        assert not prob[n, :, h:, :].any() and not prob[n, :, :, w:].any()
        assert (labels[n, h:, :] == K).all() and (labels[n, :, w:] == K).all()
        keep = ~R.undecided(ref, tau, max(1e-3, 2 * float((DEVICE_CEILING + trunc).max())))
        assert np.array_equal(labels[n, :h, :w][keep], R.rw_labels(ref, scb, K, tau)[keep]), n
        assert np.array_equal(labels[n, :h, :w][scb < K], scb[scb < K])
        assert (stats[n, :, 2] == 1.0).all(), (n, stats[n].tolist())
        if gamma > 0:
            assert np.abs(prob[n, :, :h, :w].sum(0) - 1.0).max() <= K * (DEVICE_CEILING + float(trunc.max()))


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_oracle(phantoms):
    from pacingpseudo_amd.utils import random_walker_prior
    cases, img, scb, z = phantoms
    worst = 0.0
    for g in GAMMAS:
        prob, stats = random_walker_prior(img, scb, z, 5, gamma=g, return_stats=True)
        assert prob.shape == (3, 5, 32, 32) and prob.dtype == torch.float32 and stats.shape == (3, 5, 3)
        assert torch.equal(prob, random_walker_prior(img[:, None], scb, z, 5, gamma=g))          # (N, 1, H, W) images are the same call
        prob, stats = prob.cpu().numpy(), stats.cpu().numpy()
        for n, c in enumerate(cases):
            dev = float(np.abs(prob[n] - c['prob'][g]).max())
            trunc = float(P.truncation_error(c['img'], c['scb'], c['z'], 5, g).max())
            print(f'phantom seed {n}, gamma {g}: max |prob - oracle| = {dev:.3e}, float64 truncation {trunc:.3e}, iterations '
                  f'{stats[n, :, 0].tolist()}, true residual {stats[n, :, 1].tolist()}')
            worst = max(worst, dev)
            assert PROB_TOL <= trunc + DEVICE_CEILING
            assert dev <= PROB_TOL, (n, g, dev)
        assert (stats[:, :, 2] == 1).all() and (stats[:, :, 0] >= 1).all()                        # every class is a system
    print(f'largest deviation {worst:.3e}')


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', [0.5, 0.9])
def test_labels_equal_the_oracles(phantoms, tau):
    from pacingpseudo_amd.utils import refresh_scribbles
    cases, img, scb, z = phantoms
    for g in GAMMAS:
        labels = refresh_scribbles(img, scb, z, 5, None, tau, gamma=g)
        assert labels.dtype == scb.dtype and labels.shape == scb.shape
        assert refresh_scribbles(img, scb.to(torch.uint8), z, 5, None, tau, gamma=g).dtype == torch.uint8
        labels = labels.cpu().numpy()
        for n, c in enumerate(cases):
            out = R.undecided(c['prob'][g], tau) & (c['scb'] == 5)
            print(f'phantom seed {n}, gamma {g}, threshold {tau}: {100 * out.sum() / (c["scb"] == 5).sum():.2f} % of the unlabelled pixels left out')
            assert out.sum() <= 0.02 * (c['scb'] == 5).sum()
            assert np.array_equal(labels[n][~out], R.rw_labels(c['prob'][g], c['scb'], 5, tau)[~out]), (n, g)
            assert np.array_equal(labels[n][c['scb'] < 5], c['scb'][c['scb'] < 5])              # seeds keep their class


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_is_the_plain_walker(phantoms):
    from pacingpseudo_amd.utils import random_walker, random_walker_prior
    cases, img, scb, z = phantoms
    scb = scb.clone()
    scb[1][scb[1] == 2] = 5                                                  # slice 1 without seeds of class 2
    assert bool((scb[1] == 3).any())
    prob, stats = random_walker_prior(img, scb, z, 5, gamma=0.0, return_stats=True)
    plain, plain_stats = random_walker(img, scb, 5, return_stats=True)
    dev = float((prob - plain).abs().max())
    print(f'gamma = 0 against utils.random_walker: max difference {dev:.3e}')
    assert dev <= PROB_TOL
    assert not bool(prob[1, 2].any()) and stats[1, 2].tolist() == [0.0, 0.0, 1.0]
    assert torch.equal(stats[:, :, 2], plain_stats[:, :, 2]) and bool((stats[0, :, 0] >= 1).all())


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_unseeded_systems(phantoms):
    from pacingpseudo_amd.utils import refresh_scribbles
    cases, _, _, _ = phantoms
    c = cases[0]
    scb = np.where(c['scb'] == 2, 5, c['scb'])
    labels, stats, prob = refresh_scribbles(*_dev(c['img'][None], scb[None], c['z'][None]), 5, None, 0.9, gamma=0.1, return_stats=True,
                                            return_prob=True)
    assert float(prob[0, 2].max()) > 0.5 and float(stats[0, 2, 0]) >= 1                            # an ordinary system
    _check_own_cases(prob, labels, stats, [(c['img'], scb, c['z'])], 5, 0.1, 0.9)
    # no seed at all, a constant image and constant per-class logits: L const = 0, so prob = softmax of the constants
    K, S = 4, 16
    const = np.array([0.3, -1.0, 2.0, 0.5], np.float32)
    z = np.broadcast_to(const[:, None, None], (K, S, S)).copy()
    none = np.full((S, S), K, np.int64)
    labels, stats, prob = refresh_scribbles(*_dev(np.full((1, S, S), 4.0, np.float32), none[None], z[None]), K, None, 0.5, gamma=0.1,
                                            return_stats=True, return_prob=True)
    want = P.softmax(const[:, None, None])[:, 0, 0]
    dev = float(np.abs(prob[0].cpu().numpy() - want[:, None, None]).max())
    print(f'no seed, constant prior: max |prob - softmax| = {dev:.3e}, iterations {stats[0, :, 0].tolist()}')
    assert dev <= 1e-5 and bool((stats[0, :, 2] == 1).all())
    assert bool((labels[0] == 2).all())                                      # softmax(2.0 among these) = 0.64 >= 0.5


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_padding_and_odd_shapes():
    from pacingpseudo_amd.utils import refresh_scribbles
    K, H, W, g = 3, 24, 24, 0.1
    rng = np.random.default_rng(5)
    cases = []
    for seed, (h, w) in zip((3, 4, 5, 6), ((7, 1), (1, 9), (1, 1), (17, 23))):
        img = _image(seed, h, w)
        scb = np.full((h, w), K, np.int64)
        flat = rng.permutation(h * w)
        if h * w > 1:
            scb.flat[flat[0]], scb.flat[flat[1]] = 0, 1                      # class 2 has no seed; the 1 x 1 slice has none at all
        cases.append((img, scb, rng.normal(0, 2, (K, h, w)).astype(np.float32)))
    img, scb, z, sizes = _planes(cases, H, W, K)
    a = refresh_scribbles(*_dev(img, scb, z), K, sizes, 0.9, gamma=g, return_stats=True, return_prob=True)
    _check_own_cases(a[2], a[0], a[1], cases, K, g, 0.9)
    # what lies outside h x w is never read: NaN in the image and logits padding, seeds in the scribble padding, the same bits.
    # (the Python surface refuses non-finite logits as a whole, so this goes to the library directly)
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._prep import prep
    from pacingpseudo_amd._rwp import rwp
    import ctypes
    img2, scb2, z2 = np.full_like(img, np.nan), np.zeros_like(scb), np.full_like(z, np.nan)
    for n, (h, w) in enumerate(sizes):
        img2[n, :h, :w], scb2[n, :h, :w], z2[n, :, :h, :w] = img[n, :h, :w], scb[n, :h, :w], z[n, :, :h, :w]
    d_img, d_scb, d_z = _dev(img2, scb2, z2, torch.int32)
    N = len(cases)
    host = np.ascontiguousarray(np.asarray(sizes, np.int32))
    hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    prob, stats = torch.empty((N, K, H, W), device=DEV), torch.empty((N, K, 3), device=DEV)
    out = torch.empty((N, H, W), device=DEV, dtype=torch.int32)
    ws = torch.empty(rwp.prwp_workspace_bytes(N, K, H, W), device=DEV, dtype=torch.uint8)
    rwp.prwp_solve(d_img.data_ptr(), d_scb.data_ptr(), d_z.data_ptr(), hp, N, K, H, W, 13.0, 1e-4, g, 1e-6, 10000, prob.data_ptr(),
                   stats.data_ptr(), ws.data_ptr(), stream_ptr())
    prep.pprep_rw_labels(prob.data_ptr(), d_scb.data_ptr(), hp, N, K, H, W, 0.9, out.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(prob, a[2]) and torch.equal(stats, a[1]) and torch.equal(out.to(a[0].dtype), a[0])


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 32])
def test_class_counts(K):
    from pacingpseudo_amd.utils import refresh_scribbles
    rng = np.random.default_rng(K)
    img = _image(30 + K, 16, 16)
    scb = np.full((16, 16), K, np.int64)
    scb.flat[rng.permutation(256)[:K]] = np.arange(K)                        # one seed per class
    z = rng.normal(0, 2, (K, 16, 16)).astype(np.float32)
    labels, stats, prob = refresh_scribbles(*_dev(img[None], scb[None], z[None]), K, None, 0.5, gamma=0.1, return_stats=True,
                                            return_prob=True)
    _check_own_cases(prob, labels, stats, [(img, scb, z)], K, 0.1, 0.5)
    if K == 1:                                                               # softmax of one class is 1: the solution is 1 everywhere
        assert (labels == 0).all()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_reproducible_alone_in_a_batch_and_on_a_side_stream(phantoms):
    from pacingpseudo_amd.utils import refresh_scribbles
    _, img, scb, z = phantoms
    kw = dict(gamma=0.1, return_stats=True, return_prob=True)
    a = refresh_scribbles(img, scb, z, 5, **kw)
    b = refresh_scribbles(img, scb, z, 5, **kw)
    alone = refresh_scribbles(img[1:2].contiguous(), scb[1:2].contiguous(), z[1:2].contiguous(), 5, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = refresh_scribbles(img, scb, z, 5, **kw)
    side.synchronize()
    for x, y, w_, one in zip(a, b, c, alone):
        assert torch.equal(x, y) and torch.equal(x, w_) and torch.equal(x[1:2], one)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_probabilities_sum_to_one(phantoms):
    from pacingpseudo_amd.utils import random_walker_prior
    _, img, scb, z = phantoms
    for g in GAMMAS:
        dev = float((random_walker_prior(img, scb, z, 5, gamma=g).sum(1) - 1.0).abs().max())
        print(f'gamma {g}: max |sum_k prob - 1| = {dev:.3e}')
        assert dev <= 5 * PROB_TOL


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_iteration_cap_and_the_reported_residual(phantoms):
    from pacingpseudo_amd.utils import random_walker_prior
    cases, img, scb, z = phantoms
    c = cases[0]
    prob, stats = random_walker_prior(img[:1].contiguous(), scb[:1].contiguous(), z[:1].contiguous(), 5, gamma=0.1, max_iters=3,
                                      return_stats=True)
    prob, stats = prob.cpu().numpy()[0], stats.cpu().numpy()[0]
    for k in range(5):
        assert stats[k, 0] == 3 and stats[k, 2] == 0 and stats[k, 1] > 1e-6, stats[k].tolist()
        ref = P.relres(c['img'], c['scb'], c['z'], 5, 0.1, k, prob[k])
        print(f'class {k}: reported true residual {stats[k, 1]:.6e}, recomputed in float64 {ref:.6e}')
        assert abs(stats[k, 1] - ref) <= 1e-3 * ref, (k, stats[k, 1], ref)


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_sentinel_bands(phantoms):
    import ctypes
    from pacingpseudo_amd._lib import stream_ptr
    from pacingpseudo_amd._rwp import rwp
    from pacingpseudo_amd.utils import random_walker_prior
    _, img, scb, z = phantoms
    N, K, H, W = 3, 5, 32, 32
    sizes = [(32, 32), (29, 31), (32, 17)]
    host = np.ascontiguousarray(np.asarray(sizes, np.int32))
    hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    want = random_walker_prior(img, scb, z, K, sizes, gamma=0.1, return_stats=True)
    got = []
    for pattern in (0xFF, 0xA5):
        bs = BandSet(pattern, DEV)
        g_img, g_scb, g_z = bs.tensor(img, label='img'), bs.tensor(scb.to(torch.int32), label='scb'), bs.tensor(z, label='logits')
        prob, stats = bs.banded((N, K, H, W), torch.float32, 'prob'), bs.banded((N, K, 3), torch.float32, 'stats')
        ws = bs.ws(rwp.prwp_workspace_bytes(N, K, H, W), 'workspace')
        rwp.prwp_solve(g_img.data_ptr(), g_scb.data_ptr(), g_z.data_ptr(), hp, N, K, H, W, 13.0, 1e-4, 0.1, 1e-6, 10000, prob.ptr(),
                       stats.ptr(), ws.ptr(), stream_ptr())
        torch.cuda.synchronize()
        assert bs.damaged() == []
        got.append((prob.t.clone(), stats.t.clone()))
    for x, y, w_ in zip(got[0], got[1], want):
        assert torch.equal(x, y) and torch.equal(x, w_)                      # nothing stale read, nothing left unwritten
    assert bool(torch.isfinite(got[0][0]).all())


def test_non_finite_logits_and_wrong_shapes_are_refused(phantoms):
    from pacingpseudo_amd.utils import random_walker_prior
    _, img, scb, z = phantoms
    bad = z.clone()
    bad[2, 4, 31, 31] = float('inf')
    with pytest.raises(ValueError, match='non-finite'):
        random_walker_prior(img, scb, bad, 5)
    with pytest.raises(ValueError, match='logits must be'):
        random_walker_prior(img, scb, z[:, :4].contiguous(), 5)
    with pytest.raises(TypeError, match='float32'):
        random_walker_prior(img, scb, z.double(), 5)


# 11 --------------------------------------------------------------------------------------------------------------------------
DRIVER = ['--synthetic', '8', '--image_size', '32', '--epoch', '3', '--batch_size', '4', '--num_workers', '2', '--init_ch', '8',
          '--max_ch', '64', '--rw_refresh', '1', '--rw_refresh_start', '1']
# the driver in a child process with the augmenter's entry wrapped: every raw batch the loader's workers deliver is kept
RECORDER = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from pacingpseudo_amd import augment, train
seen = []
inner = augment.DeviceAugmenter.ahead
def ahead(self, stream, image, label, scribble, *rest):
    seen.append((image.numpy().copy(), scribble.numpy().copy()))
    return inner(self, stream, image, label, scribble, *rest)
augment.DeviceAugmenter.ahead = ahead
train.train_main({argv!r})
np.savez({out!r}, img=np.stack([s[0] for s in seen]), scb=np.stack([s[1] for s in seen]))
"""


def test_driver_refreshes_and_resumes_bit_for_bit(tmp_path):
    from pacingpseudo_amd import resume
    from pacingpseudo_amd.data import SyntheticPhantoms
    from tests.test_gpu_resume import RUN_TIMEOUT, _assert_same_run, _driver, _scalars, _trimmed_copy
    import glob
    argv = DRIVER + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'full')]
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE')}
    r = subprocess.run([sys.executable, '-c', RECORDER.format(root=ROOT, argv=argv, out=str(tmp_path / 'seen.npz'))], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=RUN_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    (full,) = glob.glob(os.path.join(str(tmp_path / 'full'), 't1', 'Control', 'Control-*-fold1-r'))
    assert sorted(os.listdir(os.path.join(full, 'rw_refresh'))) == ['maps_1.npz', 'maps_2.npz']
    ds = SyntheticPhantoms(8, 5, size=32, raw=True, seed=1)                  # the driver's training set
    raw = [ds.raw_arrays(i) for i in range(8)]
    maps = {0: [np.asarray(x[2]) for x in raw]}
    for t in (1, 2):
        maps[t] = resume.read_refresh_maps(resume.refresh_maps_path(full, t))
        z = np.load(resume.refresh_maps_path(full, t))
        assert z['report_changed'].shape == (8,) and not z['report_skipped'].any() and z['report_converged'].all() and z['param_gamma'] == 0.1
        assert all(m.dtype == np.uint8 and m.shape == (32, 32) for m in maps[t])
        for i in range(8):                                                   # S is the scribble on disk, at every refresh
            seeds = raw[i][2] < 5
            assert np.array_equal(maps[t][i][seeds], raw[i][2][seeds])
    # seeds keep their class, so coverage never falls below the scribbles'; the first refresh labelled something new
    assert any(not np.array_equal(a, b) for a, b in zip(maps[1], maps[0])) and (z['report_coverage_after'] >= z['report_coverage_before']).all()
    # two batches of four per epoch, in the order the model saw them: every slice once per epoch, with that epoch's maps
    seen = np.load(tmp_path / 'seen.npz')
    assert seen['img'].shape == (6, 4, 32, 32)
    for e in range(3):
        ids = []
        for b in (2 * e, 2 * e + 1):
            for j in range(4):
                (i,) = [i for i in range(8) if np.array_equal(seen['img'][b, j], raw[i][0].astype(np.float32))]
                ids.append(i)
                assert np.array_equal(seen['scb'][b, j], maps[e][i]), (e, b, j, i)
        assert sorted(ids) == list(range(8))
    log = open(os.path.join(full, 'log.txt')).read()
    lines = [ln for ln in log.splitlines() if 'random-walker refresh at epoch' in ln]
    assert len(lines) == 2 and 'epoch 001: 8 slices (0 skipped)' in lines[0] and '0 unconverged systems' in lines[1], log[-2000:]
    sc = _scalars(full)
    for t in (1, 2):
        z = np.load(resume.refresh_maps_path(full, t))
        assert sc[('RW/refresh_coverage', t)] == pytest.approx(float(z['report_coverage_after'].mean()))
        assert sc[('RW/refresh_changed', t)] == pytest.approx(float(z['report_changed'].mean())) and ('RW/refresh_agreement', t) in sc
    assert not any(tag.startswith('RW/refresh') and step == 0 for tag, step in sc)
    # resumed from state_1: the maps of maps_1 are loaded, the refresh due at epoch 2 is recomputed -- the same run bit for bit
    copy = _trimmed_copy(full, tmp_path / 'full', tmp_path / 'resumed', 1, 2)
    os.remove(resume.refresh_maps_path(copy, 2))
    resume_argv = DRIVER + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'resumed'), '--resume',
                            os.path.join(copy, 'ckps', 'state_1.pth')]
    r = _driver('train_chaos.py', resume_argv)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    _assert_same_run(full, copy, 2)
    a, b = np.load(resume.refresh_maps_path(full, 2)), np.load(resume.refresh_maps_path(copy, 2))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a.files)
    # without maps_1.npz the run cannot be continued, and says which file it misses
    broken = _trimmed_copy(full, tmp_path / 'full', tmp_path / 'broken', 1, 2)
    os.remove(resume.refresh_maps_path(broken, 1))
    r = _driver('train_chaos.py', DRIVER + ['--state_interval', '1', '--tag', 'r', '--root', str(tmp_path / 'broken'), '--resume',
                                            os.path.join(broken, 'ckps', 'state_1.pth')])
    assert r.returncode != 0 and 'ResumeError' in r.stderr and 'maps_1.npz' in r.stderr, r.stderr[-3000:]


# 12 --------------------------------------------------------------------------------------------------------------------------
def _tree_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(_tree_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_tree_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_refresh_leaves_the_training_state_alone():
    import copy
    import random
    from pacingpseudo_amd.augment import AugConfig, DeviceAugmenter, collate_raw
    from pacingpseudo_amd.data import SyntheticPhantoms, full_flags
    from pacingpseudo_amd.models import ConsistencyRegulr
    from pacingpseudo_amd.optim import FusedAdam
    from pacingpseudo_amd.utils import SharedMaps, check_rw_params, refresh_dataset
    from pacingpseudo_amd.utils.random_walker import refresh_forward
    K, S = 5, 32
    args = full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64], aux_drop_prob=0.5)
    torch.manual_seed(3)
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=K, output_stride=8, is_stride_conv=False,
                         is_trans_conv=False, elab_end_points=True),
        kwargs_aux_path=dict(num_classes=K, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=args.hid_ch, aux_drop_prob=0.5,
                             do_memory=True, max_step=args.epoch, update_momentum=0.9, ensemble_mode='cosine_similarity'),
        args_parser=args).cuda()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=args.wd)
    ds = SyntheticPhantoms(6, K, size=S, raw=True, seed=1)
    ds.scribble_override = SharedMaps([np.asarray(ds.raw_arrays(i)[2]).astype(np.uint8) for i in range(6)])
    aug = DeviceAugmenter(AugConfig(num_classes=K, crop_size=(S, S), do_strong=True), device=DEV, seed=3)
    batch = collate_raw([ds[i] for i in range(4)])
    inputs = {k: v for k, v in aug(batch['img'], batch['lab'], batch['scb'], batch['sizes']).items() if k not in ('label', 'label_strong')}
    out = model(inputs, mode='train', step=0)                                # one step: every state is live
    opt.zero_grad()
    (out['loss_pce'] + out['loss_cr'] + out['loss_aux_cls'] + out['loss_memory']).backward()
    opt.step()
    torch.cuda.synchronize()

    def snapshot():
        return dict(model={k: v.detach().clone() for k, v in model.state_dict().items()}, opt=copy.deepcopy(opt.state_dict()),
                    python=random.getstate(), numpy=np.random.get_state(), torch=torch.get_rng_state(), cuda=torch.cuda.get_rng_state(),
                    aug=aug.rng.get_state(), modes=[m.training for m in model.modules()])

    prm = dict(check_rw_params(K=K), gamma=0.1)
    for training in (True, False):
        model.train(training)
        before = snapshot()
        held = [ds.scribble_override[i].copy() for i in range(6)]
        maps, rep = refresh_dataset(ds, refresh_forward(model, K), K, torch.device(DEV), prm, 8)
        torch.cuda.synchronize()
        after = snapshot()
        assert model.training is training
        for key in before:
            assert _tree_equal(before[key], after[key]), (training, key)
        assert all(np.array_equal(ds.scribble_override[i], held[i]) for i in range(6))            # the caller installs the maps
        assert len(maps) == 6 and all(m.dtype == np.uint8 and m.shape == (S, S) for m in maps)
        assert not rep['skipped'].any() and rep['converged'].all() and (rep['coverage_after'] >= rep['coverage_before']).all()
        assert np.allclose(rep['changed'], [(m != h).mean() for m, h in zip(maps, held)])
    # a stride the slices are no multiple of: every slice keeps its map and is counted
    maps, rep = refresh_dataset(ds, refresh_forward(model, K), K, torch.device(DEV), prm, 5)
    assert rep['skipped'].all() and not rep['changed'].any() and all(np.array_equal(m, h) for m, h in zip(maps, held))


def test_refresh_dataset_is_what_refresh_scribbles_returns():
    """refresh_dataset = the host normalisation of evaluation items, `forward`, refresh_scribbles on the raw image and the scribble
    on disk -- also when an earlier refresh is in force."""
    from pacingpseudo_amd.data import SyntheticPhantoms
    from pacingpseudo_amd.utils import check_rw_params, refresh_dataset, refresh_scribbles
    K, S, n = 5, 32, 3
    ds = SyntheticPhantoms(n, K, size=S, raw=True, seed=1)
    ev = SyntheticPhantoms(n, K, size=S, train=False, native=True, compact=True, seed=1)
    ev.base_seed = ds.base_seed                                              # the same slices as evaluation items
    raw = [ds.raw_arrays(i) for i in range(n)]
    got_inputs = []

    def forward(x):
        got_inputs.append(x.clone())
        return torch.cat([3.0 * x, -x, x * x, 0.5 * x, 1.0 - x], 1)

    prm = dict(check_rw_params(K=K, threshold=0.5), gamma=1.0)
    ds.scribble_override = [np.zeros((S, S), np.uint8)] * n                  # an earlier map in force: it must not become the seeds
    maps, rep = refresh_dataset(ds, forward, K, torch.device(DEV), prm, 8)
    assert len(got_inputs) == 1 and all(torch.equal(got_inputs[0][i].cpu(), ev[i]['image']) for i in range(n))
    img = torch.from_numpy(np.stack([r[0] for r in raw]).astype(np.float32)).to(DEV)
    scb = torch.from_numpy(np.stack([r[2] for r in raw])).to(DEV)
    want = refresh_scribbles(img, scb, forward(got_inputs[0]), K, None, 0.5, gamma=1.0).cpu().numpy()
    assert all(np.array_equal(maps[i], want[i]) for i in range(n))
    assert np.allclose(rep['changed'], [(want[i] != 0).mean() for i in range(n)])
    assert np.allclose(rep['coverage_before'], [(r[2] != K).mean() for r in raw])
