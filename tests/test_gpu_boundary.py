"""Boundary loss on the device (libpacingpseudo_dist.so): the exact Euclidean distance transform against scipy, the signed level-set
maps and the loss against the float64 reference of tests/_boundary_reference.py, determinism and extents under sentinel bands, and
the fully supervised driver with and without --do_loss_boundary.

Bounds.  Unit spacing: every candidate (g sy)^2 + (dx sx)^2 is an integer below 2^24, so the squared field is exact and the distance
is one correctly rounded fp32 root away from it: 1 ulp.  Inside a class phi = -(d - 1); d - 1 is exact in fp32 for 1 <= d < 2^24 and
has at least half of d's ulp, so the root's half ulp stays within 1 ulp of phi.  Anisotropic spacing: the fp32 chain (two rounded
products, their squares, one sum, one root) is bounded by about 3 * 2^-24 relative; REL = 2^-21 leaves a factor of about 2.6, and
the minimum over candidates cannot err by more than its candidates do.  The loss keeps the bounds of
test_gpu_round2.py::test_dice_loss_kernels_against_torch."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _boundary_reference as R  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests._guard import PATTERNS, BandSet  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 2.0 ** -21


def dev():
    return torch.device('cuda', 0)


def _ulp_ok(got32, ref64):
    """|got - ref| <= one fp32 ulp of the reference's magnitude (0 must be met exactly, +inf by +inf)."""
    got = np.asarray(got32, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    inf = np.isinf(ref)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    ok = np.where(inf, got == ref, np.abs(got - np.where(inf, 0.0, ref)) <= np.where(inf, 0.0, ulp))
    return bool(ok.all())


# ---------------------------------------------------------------- EDT, unit spacing
def _edt_planes():
    rng = np.random.RandomState(11)
    cases = {}
    cases['1x1'] = np.array([[[0]], [[1]]], dtype=np.uint8)                               # zero; non-zero (no zero pixel: +inf)
    cases['1x40'] = (rng.rand(3, 1, 40) < np.array([0.5, 0.8, 0.95])[:, None, None]).astype(np.uint8)
    cases['40x1'] = (rng.rand(3, 40, 1) < np.array([0.5, 0.8, 0.95])[:, None, None]).astype(np.uint8)
    big = (rng.rand(4, 67, 129) < 0.8).astype(np.uint8)
    big[2, :, :60] = 1                                                                    # a wide block without a zero
    big[3] = 7                                                                            # a plane with no zero at all
    cases['67x129'] = big
    cases['3x300'] = (rng.rand(2, 3, 300) < np.array([0.8, 0.97])[:, None, None]).astype(np.uint8)
    cases['2048x3'] = (rng.rand(2, 2048, 3) < np.array([0.9, 0.999])[:, None, None]).astype(np.uint8)      # the limits of H and of W:
    cases['3x2048'] = (rng.rand(2, 3, 2048) < np.array([0.9, 0.999])[:, None, None]).astype(np.uint8)      # 16 column segments; the whole LDS row
    yy, xx = np.indices((16, 16))
    cases['checkerboard'] = np.stack([(yy + xx) % 2, (yy + xx + 1) % 2]).astype(np.uint8)
    corners = np.ones((4, 64, 64), dtype=np.uint8)
    for p, (y, x) in enumerate([(0, 0), (0, 63), (63, 0), (63, 63)]):
        corners[p, y, x] = 0
    cases['corners'] = corners
    far = np.ones((1, 512, 512), dtype=np.uint8)
    far[0, 511, 0] = 0
    cases['512x512'] = far
    for v in cases.values():
        v.setflags(write=False)
    return cases


_EDT = {}


def _edt_case(name):
    """(mask, scipy's squared distances as integers (-1: none)); made once and never modified."""
    if not _EDT:
        for k, m in _edt_planes().items():
            _EDT[k] = (m, R.edt_squared_int(m))
    return _EDT[name]


@pytest.mark.parametrize('name', ['1x1', '1x40', '40x1', '67x129', '3x300', '2048x3', '3x2048', 'checkerboard', 'corners', '512x512'])
def test_edt_unit_spacing_against_scipy(name):
    from pacingpseudo_amd.utils import distance_transform_edt
    mask, ref2 = _edt_case(name)
    assert mask.shape[0] > 1 or name == '512x512'
    m = torch.from_numpy(mask.copy()).to(dev())
    sq = distance_transform_edt(m, squared=True).cpu().numpy()
    d = distance_transform_edt(m).cpu().numpy()
    assert sq.dtype == np.float32 and sq.shape == mask.shape
    none = ref2 < 0
    want2 = np.where(none, np.inf, ref2.astype(np.float64))
    bad = int((sq.astype(np.float64) != want2).sum())
    print(f'edt {name}: {mask.shape}, {bad} squared distances differ from scipy, max {np.where(none, 0, ref2).max()}')
    assert bad == 0                                                   # bit for bit: integers
    root32 = np.sqrt(want2).astype(np.float32)
    assert _ulp_ok(d, root32.astype(np.float64))
    assert (d[mask == 0] == 0).all() and (sq[mask == 0] == 0).all()
    if name == '67x129':
        assert np.isinf(d[3]).all() and np.isinf(sq[3]).all() and np.isfinite(d[:3]).all()
    if name == '1x1':
        assert d[0, 0, 0] == 0 and np.isinf(d[1, 0, 0])
    # a single (H, W) plane is a batch of one
    one = distance_transform_edt(m[0].bool()).cpu().numpy()
    assert one.shape == mask.shape[1:] and np.array_equal(one, d[0])


@pytest.mark.parametrize('shape', [(33, 9), (67, 129)])
def test_edt_anisotropic_spacing_against_float64(shape):
    from pacingpseudo_amd.utils import distance_transform_edt
    rng = np.random.RandomState(shape[0])
    mask = (rng.rand(3, *shape) < np.array([0.6, 0.8, 0.97])[:, None, None]).astype(np.uint8)
    ref = R.edt(mask, (1.5, 0.75))
    assert np.isfinite(ref).all()
    got = distance_transform_edt(torch.from_numpy(mask).to(dev()), spacing=(1.5, 0.75)).double().cpu().numpy()
    err = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    print(f'edt (1.5, 0.75) {shape}: max relative error {err.max():.3e} (bound {REL:.3e})')
    assert (np.abs(got - ref) <= REL * ref).all()
    got2 = distance_transform_edt(torch.from_numpy(mask).to(dev()), spacing=(1.5, 0.75), squared=True).double().cpu().numpy()
    assert (np.abs(got2 - ref * ref) <= 2 * REL * ref * ref).all()


# ---------------------------------------------------------------- signed maps
def _blobs(N, K, H, W, seed):
    rng = np.random.RandomState(seed)
    cm = np.zeros((N, H, W), dtype=np.int64)
    yy, xx = np.indices((H, W))
    for n in range(N):
        for _ in range(3 * K):
            k = rng.randint(1, K) if K > 1 else 0
            cy, cx, ry, rx = rng.randint(H), rng.randint(W), rng.randint(1, max(H // 3, 2)), rng.randint(1, max(W // 3, 2))
            cm[n][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return cm


_MAPS = {}


def _maps_case(name):
    """(class map, K, {spacing: float64 phi}); made once and never modified."""
    if not _MAPS:
        main = _blobs(3, 5, 37, 70, 3)
        main[0][main[0] == 3] = 0                     # image 0 lacks class 3
        main[1] = 2                                   # image 1 is entirely class 2
        main[2, 5:9, 60:66] = 5                       # image 2 holds the value K: ignored pixels, outside every class
        main[2, 30, 2] = -1
        assert all((main[2] == k).any() for k in range(5)) and not (main[0] == 3).any()
        one = (np.random.RandomState(5).rand(2, 9, 11) < 0.3).astype(np.int64)          # K = 1: the value 1 is outside the class
        many = np.random.RandomState(6).randint(0, 32, size=(2, 16, 16)).astype(np.int64)
        for name_, cm, K in (('main', main, 5), ('k1', one, 1), ('k32', many, 32)):
            cm.setflags(write=False)
            _MAPS[name_] = (cm, K, {sp: R.signed_maps(cm, K, sp) for sp in ((1.0, 1.0), (2.0, 1.0))})
    return _MAPS[name]


@pytest.mark.parametrize('name', ['main', 'k1', 'k32'])
def test_signed_maps_against_the_reference(name):
    from pacingpseudo_amd.utils import signed_distance_maps
    cm, K, refs = _maps_case(name)
    c = torch.from_numpy(cm.copy()).to(dev())
    got = signed_distance_maps(c, K).cpu().numpy()
    ref = refs[(1.0, 1.0)]
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(np.sign(got), np.sign(ref))                 # the sign is exact
    assert _ulp_ok(got, ref)
    if name == 'main':
        assert not got[0, 3].any()                                    # absent class
        assert not got[1, 2].any() and (got[1, [0, 1, 3, 4]] == 0).all()      # the whole image: 0; the others are absent there
        assert (got[2, :, 5:9, 60:66] > 0).all() and (got[2, :, 30, 2] > 0).all()      # ignored pixels are outside every class
        assert (got[0, 1] < 0).any() and (got[0, 1] > 0).any()
    got2 = signed_distance_maps(c, K, spacing=(2.0, 1.0)).double().cpu().numpy()
    ref2 = refs[(2.0, 1.0)]
    err = np.abs(got2 - ref2)
    print(f'signed maps {name} spacing (2, 1): max relative error {(err / np.where(ref2 != 0, np.abs(ref2), 1.0)).max():.3e}')
    assert (err <= REL * np.abs(ref2)).all() and np.array_equal(np.sign(got2), np.sign(ref2))
    # (H, W) input, and a narrower integer dtype
    single = signed_distance_maps(c[0].to(torch.int32), K).cpu().numpy()
    assert single.shape == (K,) + cm.shape[1:] and np.array_equal(single, got[0])


# ---------------------------------------------------------------- loss
def _loss_inputs():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(3, 5, 20, 24, generator=g) * 3
    cls = torch.randint(0, 5, (3, 20, 24), generator=g)
    cls[1][cls[1] == 2] = 0                                           # a class absent from one sample
    return z, cls


def _check_loss(z, phi_ref64, run):
    """run(zd) -> device loss; both bounds of the dice_loss_fn test, upstream factor 1.7."""
    ref, gref = R.loss_and_grad(z.numpy(), phi_ref64, 1.7)
    zd = z.to(dev()).requires_grad_(True)
    got = run(zd)
    (got * 1.7).backward()
    err = abs(float(got.detach()) - ref)
    rel = G.rel_err(zd.grad.double().cpu().numpy(), gref)
    print(f'boundary loss {tuple(z.shape)}: ref {ref:.9f}, |dev - ref| = {err:.3e}, gradient rel_err {rel:.3e}')
    assert got.dtype == torch.float32 and got.dim() == 0
    assert err < 1e-6 * max(1.0, abs(ref))
    assert rel < 1e-5
    return float(got.detach())


def test_loss_arithmetic_with_the_devices_own_maps():
    from pacingpseudo_amd.losses.losses import boundary_loss
    from pacingpseudo_amd.utils import signed_distance_maps
    z, cls = _loss_inputs()
    phi = signed_distance_maps(cls.to(dev()), 5)
    a = _check_loss(z, phi.double().cpu().numpy(), lambda zd: boundary_loss(zd, None, dist_maps=phi))
    assert a != 0.0
    assert not phi.requires_grad


def test_loss_end_to_end_from_the_label():
    from pacingpseudo_amd.losses.losses import boundary_loss
    z, cls = _loss_inputs()
    phi = R.signed_maps(cls.numpy(), 5)
    onehot = torch.nn.functional.one_hot(cls, 5).permute(0, 3, 1, 2).float().contiguous().to(dev())
    a = _check_loss(z, phi, lambda zd: boundary_loss(zd, onehot))
    b = _check_loss(z, phi, lambda zd: boundary_loss(zd, cls.to(dev())))
    assert a == b                                                     # one-hot label and class map: the same maps, the same bits
    phi2 = R.signed_maps(cls.numpy(), 5, (2.0, 1.0))
    _check_loss(z, phi2, lambda zd: boundary_loss(zd, cls.to(dev()), spacing=(2.0, 1.0)))


def test_loss_with_one_class_and_at_one_pixel():
    from pacingpseudo_amd.losses.losses import boundary_loss
    cm, K, refs = _maps_case('k1')
    g = torch.Generator().manual_seed(8)
    z1 = torch.randn(2, 1, 9, 11, generator=g) * 3
    v = _check_loss(z1, refs[(1.0, 1.0)], lambda zd: boundary_loss(zd, torch.from_numpy(cm.copy()).to(dev())))
    assert abs(v - refs[(1.0, 1.0)].mean()) < 1e-5                    # soft-max over one class is 1: the mean of phi, gradient 0
    z2 = torch.randn(2, 2, 1, 1, generator=g) * 3
    cls = torch.tensor([[[0]], [[1]]])
    assert _check_loss(z2, R.signed_maps(cls.numpy(), 2), lambda zd: boundary_loss(zd, cls.to(dev()))) == 0.0      # no boundary at 1x1
    phi = torch.randn(2, 2, 1, 1, generator=g) * 4
    _check_loss(z2, phi.double().numpy(), lambda zd: boundary_loss(zd, None, dist_maps=phi.to(dev())))


def test_loss_at_17_and_32_classes():
    """The class bounds 16 and 32 of the loss kernels (K <= 8 is the case above)."""
    from pacingpseudo_amd.losses.losses import boundary_loss
    g = torch.Generator().manual_seed(9)
    for K in (9, 17, 32):
        z = torch.randn(2, K, 5, 7, generator=g) * 3
        phi = torch.randn(2, K, 5, 7, generator=g) * 4
        _check_loss(z, phi.double().numpy(), lambda zd: boundary_loss(zd, None, dist_maps=phi.to(dev())))


# ---------------------------------------------------------------- determinism and extents
def _guarded_run(pattern):
    """The four launches between sentinel bands, workspaces of exactly the queried size and stale: (results, damaged bands)."""
    from pacingpseudo_amd._dist import dist
    from pacingpseudo_amd._lib import stream_ptr
    P, N, K, H, W = 2, 2, 5, 13, 37
    rng = np.random.RandomState(21)
    mask = torch.from_numpy((rng.rand(P, H, W) < 0.8).astype(np.uint8))
    cm = torch.from_numpy(_blobs(N, K, H, W, 4))
    g = torch.Generator().manual_seed(4)
    z = torch.randn(N, K, H, W, generator=g) * 3
    bs = BandSet(pattern, dev())
    st = stream_ptr()
    mask_d, cm_d, z_d = bs.tensor(mask.to(dev()), label='mask'), bs.tensor(cm.to(dev()), label='class map'), bs.tensor(z.to(dev()), label='z')
    up = bs.tensor(torch.tensor([1.7], device=dev()), label='upstream')
    edt, phi = bs.tensor((P, H, W), torch.float32, 'edt'), bs.tensor((N, K, H, W), torch.float32, 'phi')
    loss, dz = bs.tensor((1,), torch.float32, 'loss'), bs.tensor((N, K, H, W), torch.float32, 'dz')
    w1 = bs.ws(dist.pdist_edt_workspace(P, H, W), 'edt workspace')
    w2 = bs.ws(dist.pdist_signed_maps_workspace(N, K, H, W), 'maps workspace')
    w3 = bs.ws(dist.pdist_boundary_loss_workspace(N, K, H, W), 'loss workspace')
    assert (w1.n, w2.n, w3.n) == ((P * H * W * 2 + 7) // 8 * 8, (N * K * H * W * 2 + 7) // 8 * 8, 4 * 8)
    dist.pdist_edt(mask_d.data_ptr(), P, H, W, 1.0, 1.0, 0, edt.data_ptr(), w1.data_ptr(), w1.n, st)
    dist.pdist_signed_maps(cm_d.data_ptr(), N, K, H, W, 1.0, 1.0, phi.data_ptr(), w2.data_ptr(), w2.n, st)
    dist.pdist_boundary_loss_fwd(z_d.data_ptr(), phi.data_ptr(), N, K, H, W, loss.data_ptr(), w3.data_ptr(), w3.n, st)
    dist.pdist_boundary_loss_bwd(z_d.data_ptr(), phi.data_ptr(), N, K, H, W, up.data_ptr(), dz.data_ptr(), st)
    damaged = bs.damaged()
    return [t.clone() for t in (edt, phi, loss, dz)], damaged, (mask, cm, z)


def test_same_bits_under_both_band_patterns_and_bands_intact():
    from pacingpseudo_amd.losses.losses import boundary_loss
    from pacingpseudo_amd.utils import distance_transform_edt, signed_distance_maps
    runs = []
    for pattern in PATTERNS:
        res, damaged, inputs = _guarded_run(pattern)
        assert damaged == [], damaged
        assert all(bool(torch.isfinite(t).all()) for t in res)        # nothing stale or out of extent reached a result
        runs.append(res)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # two plain runs through the Python surface: the same bits again
    mask, cm, z = inputs
    for _ in range(2):
        zd = z.to(dev()).requires_grad_(True)
        e, p = distance_transform_edt(mask.to(dev())), signed_distance_maps(cm.to(dev()), 5)
        v = boundary_loss(zd, cm.to(dev()))
        (v * 1.7).backward()
        for a, b in zip(runs[0], (e, p, v.detach().view(1), zd.grad)):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- driver
_DRIVER = ['--synthetic', '8', '--image_size', '64', '--init_ch', '8', '--max_ch', '64', '--batch_size', '4', '--epoch', '2', '--num_workers', '0']


def _run_dir(root, tag):
    runs = glob.glob(os.path.join(root, 't1', 'Upperbound', f'Upperbound-*-fold1-{tag}'))
    assert len(runs) == 1, runs
    return runs[0]


def _fields(line):
    """The field names of an `epoch:` / `val:` log line."""
    return [f.split(':')[0].strip() for f in line.split('] ')[-1].split(', ')]


def test_driver_with_the_flag(tmp_path, monkeypatch, capsys):
    """Four steps (two epochs of two) with --do_loss_boundary: the log and the scalars carry the term, the first step's value is the
    reference's for that step's logits and label, and the state file refuses a resume without the flag."""
    from pacingpseudo_amd.losses import losses as L
    from pacingpseudo_amd.upper_bound import train_main
    real, calls = L.boundary_loss, []

    def spy(logits, target, *a, **kw):
        v = real(logits, target, *a, **kw)
        calls.append((torch.is_grad_enabled(), logits.detach().cpu(), target.cpu(), float(v.detach())))
        return v
    monkeypatch.setattr(L, 'boundary_loss', spy)
    root = str(tmp_path / 'on')
    train_main(['--tag', 'bl', '--root', root, '--do_loss_boundary', '--state_interval', '1'] + _DRIVER)
    run = _run_dir(root, 'bl')
    train = [c for c in calls if c[0]]
    assert len(train) == 4 and len(calls) > 4                          # four steps, and the validation passes
    _, logits, target, value = train[0]
    assert target.dtype == torch.int64 and tuple(logits.shape) == (4, 5, 64, 64)
    ref = float(R.loss(logits.double(), torch.from_numpy(R.signed_maps(target.numpy(), 5))))
    print(f'first step: loss_boundary {value:.9f}, reference {ref:.9f}')
    assert abs(value - ref) < 1e-6 * max(1.0, abs(ref)) and value != 0.0
    log = open(os.path.join(run, 'log.txt')).read().splitlines()
    for e in (0, 1):
        ep = next(ln for ln in log if f'epoch: {e:03d},' in ln)
        va = next(ln for ln in log if f'val: {e:03d},' in ln)
        assert _fields(ep)[:5] == ['epoch', 'lr', 'loss_ce', 'loss_dice', 'loss_boundary'] and _fields(va)[:4] == ['val', 'loss_ce', 'loss_dice', 'loss_boundary']
        logged = float(ep.split('loss_boundary: ')[1].split(',')[0])
        assert abs(logged - (train[2 * e][3] + train[2 * e + 1][3]) / 2) < 2e-6
    sc = {}
    for line in open(os.path.join(run, 'tb_summary', 'scalars.jsonl')):
        r = json.loads(line)
        sc[(r['tag'], r['step'])] = r['value']
    for e in (0, 1):
        assert abs(sc[('losses/loss_boundary_train', e)] - (train[2 * e][3] + train[2 * e + 1][3]) / 2) < 1e-6
        assert np.isfinite(sc[('losses/loss_boundary_val', e)]) and sc[('losses/boundary_weight', e)] == 0.01
    # resume: the same command line is accepted by the check, the one without the flag is a usage error
    from pacingpseudo_amd import resume, upper_bound
    state = os.path.join(run, 'ckps', 'state_1.pth')
    saved = resume.load(state)['args']
    assert saved['do_loss_boundary'] is True
    argv = ['--tag', 'bl', '--root', root, '--state_interval', '1', '--resume', state] + _DRIVER
    from pacingpseudo_amd.train import apply_dataset_preset
    resume.check_compatible(saved, resume.flag_dict(apply_dataset_preset(upper_bound.parser.parse_args(argv + ['--do_loss_boundary']))), 1, 1)
    capsys.readouterr()
    with pytest.raises(SystemExit) as ex:
        train_main(argv)
    assert ex.value.code == 2 and '--do_loss_boundary' in capsys.readouterr().err


def test_driver_without_the_flag_is_the_parents(tmp_path):
    """The flag off, in a process of its own: the parent's log fields and scalar tags, and the distance library is never loaded."""
    root = str(tmp_path / 'off')
    code = ('import sys\n'
            'from pacingpseudo_amd.upper_bound import train_main\n'
            f'train_main({["--tag", "off", "--root", root] + _DRIVER!r})\n'
            'm = sys.modules.get("pacingpseudo_amd._dist")\n'
            'assert m is None or m.dist._dll is None, "libpacingpseudo_dist.so was loaded"\n'
            'print("DIST_NOT_LOADED", m is None)\n')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE')}
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert 'DIST_NOT_LOADED' in r.stdout
    run = _run_dir(root, 'off')
    log = open(os.path.join(run, 'log.txt')).read()
    assert 'do_loss_boundary=False' in log                             # (the flag dump names the flag)
    for e in (0, 1):
        ep = next(ln for ln in log.splitlines() if f'epoch: {e:03d},' in ln)
        va = next(ln for ln in log.splitlines() if f'val: {e:03d},' in ln)
        assert _fields(ep) == ['epoch', 'lr', 'loss_ce', 'loss_dice', _fields(ep)[-1]] and _fields(ep)[-1].endswith('s/epoch')
        assert _fields(va) == ['val', 'loss_ce', 'loss_dice', _fields(va)[-1]] and _fields(va)[-1].endswith('s/epoch')
        assert 'loss_boundary' not in ep and 'loss_boundary' not in va
    tags = {json.loads(ln)['tag'] for ln in open(os.path.join(run, 'tb_summary', 'scalars.jsonl'))}
    assert tags and not [t for t in tags if 'boundary' in t]
    assert {'losses/loss_ce_train', 'losses/loss_dice_train', 'losses/loss_ce_val', 'losses/loss_dice_val', 'lr/current_lr'} <= tags
