"""Mean-field CRF refinement without a GPU: properties of the float64 definition (tests/_crf_refine_reference.py), the parameter
check, the C ABI of the two entry points with their refusals before any launch, and the inference flags."""
import ctypes
import importlib
import os
import re

import pytest
import torch

from tests import _crf_refine_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pp_crf_refine_workspace', 'pp_crf_refine')
SMALL = [c for c in R.CASES if c[2] * c[3] <= 2000]            # the reference properties need no large shape


# ---- the reference itself ----
@pytest.mark.parametrize('case', SMALL, ids=R.case_id)
def test_reference_rows_sum_to_one_and_zero_weights_give_the_softmax(case):
    z, x = R.inputs(case)
    r, d = case[5], case[6]
    for q in R.refine_steps(z, x, 3, r, d, **R.DEFAULTS):
        assert q.dtype == torch.float64 and q.shape == z.shape
        assert float((q.sum(1) - 1.0).abs().max()) <= 1e-14
        assert float(q.min()) >= 0.0
    off = R.refine(z, x, 3, radius=r, dilation=d, w_bilateral=0.0, w_smooth=0.0)
    assert float((off - torch.softmax(z.double(), 1)).abs().max()) <= 1e-15


def test_reference_leaves_a_single_pixel_and_a_single_class_unchanged():
    z, x = R.inputs((1, 3, 1, 1, 1, 2, 1))
    assert float((R.refine(z, x, 5, radius=2, **R.DEFAULTS) - torch.softmax(z.double(), 1)).abs().max()) <= 1e-15
    z, x = R.inputs((2, 1, 9, 9, 1, 1, 1))
    assert torch.equal(R.refine(z, x, 5, radius=1, **R.DEFAULTS), torch.ones(2, 1, 9, 9, dtype=torch.float64))


def test_reference_commutes_with_flips():
    z, x = R.inputs((2, 5, 37, 53, 1, 5, 1))
    z, x = z[:1, :, :12, :17].contiguous(), x[:1, :, :12, :17].contiguous()
    want = R.refine(z, x, 3, radius=3, dilation=2, **R.DEFAULTS)
    for dims in ((-1,), (-2,), (-1, -2)):
        got = R.refine(z.flip(dims), x.flip(dims), 3, radius=3, dilation=2, **R.DEFAULTS)
        assert float((got.flip(dims) - want).abs().max()) <= 1e-14, dims


def test_reference_constant_image_and_constant_logits_leave_nothing_spatial():
    """Every neighbour holds the same distribution q, so both normalised messages are q S / (S + 1e-6) with S > 0 at every pixel of
    a 6 x 7 image; the factor differs from pixel to pixel only through the 1e-6 (S >= 3 neighbours' weight), so Q^1 is constant up
    to ~1e-6 and Q^2 = Q^1 to the same order: the update has nothing spatial left to do."""
    z = torch.tensor([0.3, -1.0, 2.0, 0.0]).view(1, 4, 1, 1).expand(1, 4, 6, 7).contiguous()
    x = torch.full((1, 2, 6, 7), 0.25)
    q1, q2, q3 = R.refine_steps(z, x, 3, 2, 1, **R.DEFAULTS)
    q0 = torch.softmax(z.double(), 1)
    assert float((q1 - q1[:, :, :1, :1]).abs().max()) <= 1e-5            # spatially constant
    # the step is the same map at every pixel: Q^{t+1} = softmax(u + (wb + ws) Q^t); Q^1 is that map applied to Q^0
    want = torch.softmax(torch.log_softmax(z.double(), 1) + 5.0 * q0, 1)
    assert float((q1 - want).abs().max()) <= 1e-5
    assert float((q2 - torch.softmax(torch.log_softmax(z.double(), 1) + 5.0 * q1, 1)).abs().max()) <= 1e-5
    assert float((q1 - q0).abs().max()) > 1e-2                           # and it moves: the test sees a step that does nothing
    assert float((q3 - torch.softmax(torch.log_softmax(z.double(), 1) + 5.0 * q2, 1)).abs().max()) <= 1e-5
    # logits that are also constant over the classes: every class receives the same message, Q^1 = Q^0 = 1 / K
    flat = R.refine_steps(torch.full((1, 4, 6, 7), 0.7), x, 2, 2, 1, **R.DEFAULTS)
    assert all(float((q - 0.25).abs().max()) <= 1e-15 for q in flat)


def test_reference_changes_classes_on_the_test_inputs():
    """What makes a kernel that does nothing visible: at the default weights the refinement moves a share of the arg-max."""
    case = (2, 5, 37, 53, 1, 5, 1)
    z, x = R.inputs(case)
    steps, err32 = R.oracle(case)
    for t in (1, 5):
        changed = float((steps[t - 1].argmax(1) != z.argmax(1)).double().mean())
        assert 0.05 <= changed <= 0.40, (t, changed)
    assert err32 <= 1e-6, err32
    gap = R.top_two_gap(steps[4])
    assert float((gap < 1e-3).double().mean()) <= 0.01


# ---- the parameter check ----
def test_parameter_check():
    from pacingpseudo_amd import utils
    mod = importlib.import_module('pacingpseudo_amd.utils.crf_refine')
    assert utils.crf_refine is mod.crf_refine and utils.check_crf_refine_params is mod.check_crf_refine_params
    chk = mod.check_crf_refine_params
    assert chk() == dict(iterations=5, radius=5, dilation=1, sigma_xy=6.0, sigma_rgb=0.1, sigma_smooth=1.5, w_bilateral=4.0, w_smooth=1.0)
    got = chk(64, 8, 2, 1, 1, 0.5, 0, 0, K=32, C=4)
    assert got['iterations'] == 64 and got['radius'] == 8 and got['w_bilateral'] == 0.0 and isinstance(got['sigma_smooth'], float)
    assert chk(1.0, 4, 4)['iterations'] == 1
    value = [dict(iterations=0), dict(iterations=-1), dict(iterations=2.5), dict(iterations=True), dict(radius=0), dict(dilation=0),
             dict(radius=1.5), dict(sigma_xy=0.0), dict(sigma_rgb=-1.0), dict(sigma_smooth=0.0), dict(sigma_smooth=float('nan')),
             dict(sigma_smooth=float('inf')), dict(sigma_xy=float('nan')), dict(w_bilateral=-0.1), dict(w_smooth=-1.0),
             dict(w_bilateral=float('inf')), dict(w_smooth=float('nan'))]
    for kw in value:
        with pytest.raises(ValueError):
            chk(**kw)
    size = [dict(iterations=65), dict(radius=9), dict(dilation=5), dict(radius=5, dilation=4), dict(K=33), dict(K=0), dict(C=5), dict(C=0)]
    for kw in size:
        with pytest.raises(NotImplementedError):
            chk(**kw)


def test_wrapper_raises_before_touching_the_library(monkeypatch):
    from pacingpseudo_amd import _lib
    mod = importlib.import_module('pacingpseudo_amd.utils.crf_refine')

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'the library was touched ({name})')
    monkeypatch.setattr(mod, 'lib', Untouchable())
    monkeypatch.setattr(_lib, 'lib', Untouchable())
    z, x = torch.zeros(2, 5, 4, 6), torch.zeros(2, 1, 4, 6)
    with pytest.raises(ValueError, match='CUDA'):
        mod.crf_refine(z, x)
    with pytest.raises(ValueError, match='float32'):
        mod.crf_refine(z.double(), x)
    with pytest.raises(ValueError, match='float32'):
        mod.crf_refine(z, x.to(torch.int64))
    with pytest.raises(ValueError, match=r'\(N, C, H, W\)'):
        mod.crf_refine(z[0], x)
    with pytest.raises(ValueError, match='empty'):
        mod.crf_refine(torch.zeros(2, 5, 0, 6), x)
    with pytest.raises(ValueError, match='tensor'):
        mod.crf_refine(z.numpy(), x)
    with pytest.raises(ValueError, match=r'2\^31'):
        mod.crf_refine(torch.zeros(1).expand(2, 1, 1 << 15, 1 << 15), x)


# ---- the C ABI ----
def test_abi_names_the_entry_points():
    from pacingpseudo_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    want = {'pp_crf_refine_workspace': ('size_t', 4), 'pp_crf_refine': ('int', 20)}
    for name in NAMES:
        assert name in _lib._PROTOS and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\b' + want[name][0] + ' ' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, f'{name} is not declared in the header'
        assert len(m.group(1).split(',')) == len(_lib._PROTOS[name][1]) == want[name][1], name
        assert name not in _lib.H16_ENTRIES                        # logits and image are fp32 in every storage mode: one symbol
    assert _lib._PROTOS['pp_crf_refine_workspace'][0] is ctypes.c_size_t and _lib._PROTOS['pp_crf_refine'][0] is ctypes.c_int
    # the five floats sit where the header has them: after iterations, radius, dilation
    assert _lib._PROTOS['pp_crf_refine'][1][10:15] == [ctypes.c_float] * 5
    for h in ('pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h'):
        assert 'pp_crf_refine' not in open(os.path.join(ROOT, 'include', h)).read()
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', src).group(1)) == _lib.MIN_LIB_VERSION


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """No GPU is needed: every call below must return an error from its argument checks.  The pointers are made up and never
    dereferenced by the host side."""
    from pacingpseudo_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'library not built (run __graft_entry__.build())'
    lib = _lib.lib
    dll = lib.load()
    N, K, C, H, W = 2, 5, 1, 37, 53
    need = dll.pp_crf_refine_workspace(N, K, H, W)
    assert need == 4 * N * K * H * W
    for bad in ((0, K, H, W), (N, 0, H, W), (N, K, 0, W), (N, K, H, -1)):
        assert dll.pp_crf_refine_workspace(*bad) == 0
    gap = 1 << 40
    zp, xp, pp, cp, wp = (0x10000 + i * gap for i in range(5))          # five "device pointers" far apart
    vp = ctypes.c_void_p

    def call(z=zp, x=xp, n=N, k=K, c=C, h=H, w=W, it=5, r=5, d=1, sxy=6.0, srgb=0.1, ssm=1.5, wb=4.0, ws=1.0, prob=pp, cls=cp, work=wp,
             nbytes=need):
        return dll.pp_crf_refine(vp(z), vp(x), n, k, c, h, w, it, r, d, sxy, srgb, ssm, wb, ws, vp(prob), vp(cls), vp(work), nbytes, None)
    nan, inf = float('nan'), float('inf')
    cases = [dict(z=None), dict(x=None), dict(prob=None), dict(work=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=0), dict(k=0),
             dict(k=33), dict(c=0), dict(c=5), dict(it=0), dict(it=65), dict(it=-1), dict(r=0), dict(r=9), dict(d=0), dict(d=5),
             dict(r=5, d=4), dict(r=6, d=3), dict(sxy=0.0), dict(sxy=nan), dict(sxy=inf), dict(srgb=-1.0), dict(srgb=nan), dict(ssm=0.0),
             dict(ssm=nan), dict(ssm=inf), dict(wb=-1.0), dict(wb=nan), dict(wb=inf), dict(ws=-0.5), dict(ws=nan), dict(ws=inf),
             dict(nbytes=need - 1), dict(nbytes=0), dict(k=1, h=1 << 16, w=1 << 15, nbytes=1 << 62), dict(prob=zp), dict(prob=xp),
             dict(prob=wp), dict(work=zp), dict(work=wp + 2), dict(cls=pp), dict(prob=zp + need - 4)]
    for kw in cases:
        rc = call(**kw)
        assert rc < 0, (kw, rc)
        assert lib.pp_last_error(), kw
    assert call(nbytes=need - 1) == -3 and b'workspace too small' in lib.pp_last_error()
    assert b'iterations=0' in (call(it=0) and lib.pp_last_error())
    assert b'K=33' in (call(k=33) and lib.pp_last_error())
    assert b'C=5' in (call(c=5) and lib.pp_last_error())
    assert b'radius * dilation' in (call(r=6, d=3) and lib.pp_last_error())
    assert b'sigma_smooth' in (call(ssm=nan) and lib.pp_last_error())
    assert b'w_bilateral' in (call(wb=-1.0) and lib.pp_last_error())
    assert b'overlap' in (call(prob=zp) and lib.pp_last_error())
    assert b'null' in (call(z=None) and lib.pp_last_error())


# ---- inference.py ----
BASE = ['--fold', '0', '--checkpoint_file', 'run-fold0']


def test_inference_flags_parse_and_are_checked_before_anything_is_built(capsys):
    from pacingpseudo_amd import inference as I
    a = I.parse_args(BASE)
    assert a.crf_refine == 0 and I.crf_settings(a) is None
    assert (a.crf_radius, a.crf_dilation, a.crf_sigma_xy, a.crf_sigma_rgb) == (5, 1, 6.0, 0.1)               # the training driver's
    assert (a.crf_sigma_smooth, a.crf_w_bilateral, a.crf_w_smooth) == (1.5, 4.0, 1.0)
    from pacingpseudo_amd.train import parse_args as train_args
    t = train_args(['--tag', 'x'])
    assert (t.crf_radius, t.crf_dilation, t.crf_sigma_xy, t.crf_sigma_rgb) == (a.crf_radius, a.crf_dilation, a.crf_sigma_xy, a.crf_sigma_rgb)
    on = I.parse_args(BASE + ['--crf_refine', '7', '--crf_radius', '4', '--crf_dilation', '4', '--crf_sigma_xy', '3', '--crf_sigma_rgb', '0.2',
                              '--crf_sigma_smooth', '2', '--crf_w_bilateral', '0', '--crf_w_smooth', '0.5'])
    assert I.crf_settings(on) == dict(iterations=7, radius=4, dilation=4, sigma_xy=3.0, sigma_rgb=0.2, sigma_smooth=2.0, w_bilateral=0.0,
                                      w_smooth=0.5)
    for bad in (['--crf_refine', '-1'], ['--crf_refine', '65'], ['--crf_refine', 'x'], ['--crf_radius', '0'], ['--crf_radius', '9'],
                ['--crf_dilation', '5'], ['--crf_radius', '5', '--crf_dilation', '4'], ['--crf_sigma_xy', '0'], ['--crf_sigma_rgb', 'nan'],
                ['--crf_sigma_smooth', '0'], ['--crf_sigma_smooth', 'inf'], ['--crf_w_bilateral', '-1'], ['--crf_w_smooth', 'nan']):
        with pytest.raises(SystemExit) as e:
            I.parse_args(BASE + ['--crf_refine', '3'] + bad if bad[0] != '--crf_refine' else BASE + bad)
        assert e.value.code == 2, bad
        assert '--crf_' in capsys.readouterr().err, bad


def test_evaluate_refuses_bad_settings_before_anything_runs():
    from pacingpseudo_amd import inference as I

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'touched ({name})')
    with pytest.raises(ValueError, match='iterations'):
        I.evaluate(Untouchable(), Untouchable(), 4, (1.0, 1.0), 'cpu', crf=dict(iterations=0))
    with pytest.raises(NotImplementedError, match='radius'):
        I.evaluate(Untouchable(), Untouchable(), 4, (1.0, 1.0), 'cpu', crf=dict(iterations=2, radius=9))
