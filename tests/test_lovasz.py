"""Lovasz-softmax loss (upper_bound_chaos.py --do_loss_lovasz; libpacingpseudo_lov.so), the parts that need no GPU: the float64
reference of tests/_lovasz_reference.py against the Jaccard set function by brute force, the tie rule, every ValueError path of the two
Python functions, the parser's flags, the resume tables, header / binding / library agreeing symbol for symbol, and the host half of
the library under AddressSanitizer."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _lovasz_reference as R  # noqa: E402

FLAGS = ('do_loss_lovasz', 'loss_lovasz_weight', 'ramp_up_loss_lovasz', 'lovasz_per_image')
DEFAULTS = dict(do_loss_lovasz=False, loss_lovasz_weight=1.0, ramp_up_loss_lovasz=0, lovasz_per_image=False)


# ---------------------------------------------------------------- the reference itself
def test_increments_are_differences_of_the_jaccard_set_function():
    rng = np.random.RandomState(3)
    for n in range(1, 9):
        for _ in range(12):
            fg = (rng.rand(n) < rng.choice([0.2, 0.5, 0.8])).astype(np.int64)
            g = R.jaccard_increments(fg)
            assert np.abs(g - R.brute_force_increments(fg)).max() < 1e-15
            if fg.sum() > 0:
                assert abs(g.sum() - 1.0) < 1e-14 and (g >= 0).all()
    assert np.array_equal(R.jaccard_increments(np.zeros(4)), [1.0, 0.0, 0.0, 0.0])          # G = 0: J_i = 1, the loss is max e
    assert R.jaccard_increments(np.zeros(0)).shape == (0,)


def test_value_is_the_same_under_any_tie_order_and_the_gradient_is_not():
    e = torch.tensor([.5, .5, .5, .2, .2, 1, 0, 0], dtype=torch.float64)
    fg = np.array([1, 0, 1, 0, 1, 1, 0, 1])
    values, weights = [], []
    for order in R.all_tie_orders(e.numpy()):
        val, g = R.segment_loss(e, fg, order)
        values.append(float(val))
        weights.append(g.numpy())
    assert len(values) == 6 * 2 * 2
    assert max(abs(v - 0.4714285714285714) for v in values) < 1e-15
    # the stable order (ties in ascending index) against the one that takes pixel 1 (fg = 0) before pixel 0 (fg = 1)
    _, g_stable = R.segment_loss(e, fg, R.stable_order(e))
    _, g_other = R.segment_loss(e, fg, [5, 1, 0, 2, 3, 4, 6, 7])
    assert list(R.stable_order(e)) == [5, 0, 1, 2, 3, 4, 6, 7]
    assert abs(abs(g_stable[0] - g_other[0]) - 1.0 / 30.0) < 1e-15
    assert max(np.abs(w - weights[0]).max() for w in weights) > 0.03          # which is why the tie rule is part of the contract


def test_reference_loss_small_cases():
    # one pixel, two classes: class 1 present with e = 1 - p_1; class 0 absent
    z = torch.tensor([[[[0.3]], [[-0.2]]]], dtype=torch.float64)
    t = torch.tensor([[[1]]])
    p = torch.softmax(z, 1).reshape(-1)
    val, g, perms = R.loss(z, t)
    assert abs(float(val) - float(1 - p[1])) < 1e-15 and [p_.tolist() for p_ in perms] == [[0], [0]]
    val_all, _, _ = R.loss(z, t, classes='all')
    assert abs(float(val_all) - float(((1 - p[1]) + p[0]) / 2)) < 1e-15          # class 0: G = 0, the loss is max e = p_0
    # everything ignored: 0, and an out-of-range value is ignored, not indexed
    assert float(R.loss(z, torch.tensor([[[5]]]), ignore_index=None)[0]) == 0.0
    assert float(R.loss(z, torch.tensor([[[-1]]]))[0]) == 0.0
    assert float(R.loss(z, t, ignore_index=1)[0]) == 0.0
    # per image: the mean over ALL images, an image without a present class counts 0
    z2 = torch.cat([z, z])
    t2 = torch.tensor([[[1]], [[7]]])
    assert abs(float(R.loss(z2, t2, per_image=True)[0]) - float(1 - p[1]) / 2) < 1e-15
    # the loss is differentiable through the errors and the sub-gradient is sign(p - fg) g
    g_ = torch.Generator().manual_seed(0)
    z3 = torch.randn(2, 3, 4, 5, generator=g_, dtype=torch.float64, requires_grad=True)
    t3 = torch.randint(0, 3, (2, 4, 5), generator=g_)
    val, g, _ = R.loss(z3, t3)
    _, fg, _ = R.errors(z3, t3)
    (dz,) = torch.autograd.grad(val, z3)
    p = torch.softmax(z3.detach(), 1)
    dp = (torch.sign(p.permute(1, 0, 2, 3).reshape(3, -1) - fg.double()) * g / 3).reshape(3, 2, 4, 5).permute(1, 0, 2, 3)
    assert torch.allclose(dz, p * (dp - (p * dp).sum(1, keepdim=True)), atol=1e-15)


# ---------------------------------------------------------------- argument validation, before anything is loaded
def test_loss_arguments_are_refused_before_the_library_is_touched():
    from pacingpseudo_amd import _lov
    from pacingpseudo_amd.losses.losses import lovasz_softmax_loss
    z = torch.zeros(2, 3, 4, 5)
    t = torch.zeros(2, 4, 5, dtype=torch.int64)
    bad = [
        (dict(input=z.double(), target=t), 'float32'), (dict(input=z[0], target=t), '4-D'), (dict(input=None, target=t), '4-D'),
        (dict(input=torch.zeros(2, 1, 4, 5), target=t), '2 <= K <= 32'), (dict(input=torch.zeros(2, 33, 4, 5), target=t), '2 <= K <= 32'),
        (dict(input=torch.zeros(2, 3, 0, 5), target=t), 'empty axis'),
        (dict(input=torch.zeros(1, 2, 1, 1).expand(1 << 10, 2, 1 << 10, 1 << 10), target=t), '2\\^31'),
        (dict(input=z, target=t, classes='some'), 'classes'), (dict(input=z, target=t, ignore_index=1.5), 'ignore_index'),
        (dict(input=z, target=t, ignore_index=True), 'ignore_index'), (dict(input=z, target=t, per_image=2), 'per_image'),
        (dict(input=z, target=t, return_parts='yes'), 'return_parts'),
        (dict(input=z, target=None), 'torch tensor'), (dict(input=z, target=t.int()), 'int64'), (dict(input=z, target=t[:, :3]), 'int64'),
        (dict(input=z, target=torch.zeros(2, 4, 4, 5)), 'one-hot'), (dict(input=z, target=torch.zeros(5)), 'one-hot'),
        (dict(input=z, target=t), 'CUDA'),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            lovasz_softmax_loss(**kw)
    assert _lov.lov._dll is None


def test_sort_arguments_are_refused_before_the_library_is_touched():
    from pacingpseudo_amd import _lov
    from pacingpseudo_amd.utils import sort_descending
    for v, match in ((None, 'torch tensor'), (torch.zeros(3, 4).double(), 'float32'), (torch.zeros(4), 'float32'),
                     (torch.zeros(0, 4), 'S >= 1'), (torch.zeros(3, 0), 'n >= 1'), (torch.zeros(1, 1).expand(1 << 16, 1 << 15), '2\\^31'),
                     (torch.zeros(3, 4), 'CUDA')):
        with pytest.raises(ValueError, match=match):
            sort_descending(v)
    assert _lov.lov._dll is None


# ---------------------------------------------------------------- parser and resume tables
def test_parser_flags_and_defaults():
    from pacingpseudo_amd import upper_bound
    a = upper_bound.parser.parse_args(['--tag', 'x'])
    assert {k: getattr(a, k) for k in FLAGS} == DEFAULTS
    a = upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_lovasz', '--loss_lovasz_weight', '0.5', '--ramp_up_loss_lovasz', '40',
                                       '--lovasz_per_image'])
    assert (a.do_loss_lovasz, a.loss_lovasz_weight, a.ramp_up_loss_lovasz, a.lovasz_per_image) == (True, 0.5, 40, True)
    helps = {act.dest: act.help for act in upper_bound.parser._actions}
    assert 'untuned first value' in helps['loss_lovasz_weight'] and 'gaussian_ramp_up' in helps['ramp_up_loss_lovasz']
    for argv in (['--ramp_up_loss_lovasz', '-1'], ['--loss_lovasz_weight', 'nan']):
        with pytest.raises(SystemExit) as e:
            upper_bound.train_main(['--tag', 'x', '--do_loss_lovasz'] + argv)
        assert e.value.code == 2


def test_the_scribble_driver_has_none_of_the_flags():
    from pacingpseudo_amd import train
    assert not [a.dest for a in train.parser._actions if 'lovasz' in a.dest]


def test_resume_tables_and_older_state_files():
    from pacingpseudo_amd import resume, upper_bound
    for k, v in DEFAULTS.items():
        assert resume.ABSENT_DEFAULTS[k] == v and type(resume.ABSENT_DEFAULTS[k]) is type(v) and k not in resume.MAY_DIFFER
        assert upper_bound.parser.get_default(k) == v
    new = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x']))
    old = {k: v for k, v in new.items() if k not in FLAGS}          # a state file written before the flags existed
    resume.check_compatible(old, new, 1, 1)
    on = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_lovasz']))
    with pytest.raises(resume.ResumeError, match='--do_loss_lovasz'):
        resume.check_compatible(old, on, 1, 1)
    with pytest.raises(resume.ResumeError, match='--do_loss_lovasz'):
        resume.check_compatible(on, new, 1, 1)
    for extra, name in ((['--loss_lovasz_weight', '0.1'], '--loss_lovasz_weight'), (['--ramp_up_loss_lovasz', '10'], '--ramp_up_loss_lovasz'),
                        (['--lovasz_per_image'], '--lovasz_per_image')):
        other = resume.flag_dict(upper_bound.parser.parse_args(['--tag', 'x', '--do_loss_lovasz'] + extra))
        with pytest.raises(resume.ResumeError, match=name):
            resume.check_compatible(on, other, 1, 1)


# ---------------------------------------------------------------- header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_lov.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(plov_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _lib, _lov
    decls = _header_decls()
    assert len(decls) == 8
    assert list(decls) == list(_lov.EXPORTED_SYMBOLS) == list(_lov._PROTOS)
    for name, (_, argtypes) in _lov._PROTOS.items():
        assert decls[name] == len(argtypes), name
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'lovasz', 'pp_lovasz.hip')).read()
    assert int(re.search(r'#define PLOV_VERSION (\d+)', src).group(1)) == _lov.MIN_LOV_VERSION == 100
    defined = {}
    for m in re.finditer(r'extern "C"[^\n(]*?\b(plov_\w+)\s*\(([^{;]*)\)\s*\{', src):
        params = m.group(2).strip()
        defined[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    assert defined == decls          # symbol for symbol, parameter count for parameter count
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src and '#include "pp_' not in src          # self-contained
    # the only atomics are integer adds on an LDS histogram: no floating-point atomics, same bits in every run
    assert re.findall(r'\batomic\w+\(&(\w+)', code) == ['hist'] and '__shared__ unsigned hist[' in code
    for banned in ('hipDeviceSynchronize', 'hipStreamSynchronize', 'hipEventSynchronize', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset',
                   'malloc(', 'new '):
        assert banned not in code, banned
    assert len(re.findall(r'& \(PLOV_RADIX - 1\)', code)) == 3          # every digit is masked: any key stays inside its histogram
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('plov_')]          # the per-step library is as it was
    if os.path.exists(_lov.LOV_LIB_PATH):
        import ctypes
        dll = ctypes.CDLL(_lov.LOV_LIB_PATH)
        for name in decls:
            assert hasattr(dll, name), name


def test_build_loads_and_checks_the_library():
    from tests._wiring import wired
    wired('lov', 'pacingpseudo_amd/csrc/lovasz/pp_lovasz.hip')


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _lov
    from pacingpseudo_amd._lib import HipLibraryError
    if not os.path.exists(_lov.LOV_LIB_PATH):
        pytest.skip('libpacingpseudo_lov.so is not built')
    lov = _lov._LovLib()
    assert lov.plov_version() >= 100 and _lov.TILE == lov.plov_tile() and _lov.TILE % 64 == 0
    assert lov.plov_sort_workspace(0, 4) == 0 and lov.plov_loss_workspace(2, 1, 4, 4, 0) == 0 and lov.plov_loss_workspace(2, 33, 4, 4, 1) == 0
    assert lov.plov_loss_workspace(1 << 10, 2, 1 << 10, 1 << 10, 0) == 0
    assert lov.plov_sort_workspace(3, 5) >= 4 * 3 * 5 * 4 and lov.plov_loss_workspace(2, 3, 4, 5, 0) >= 16 * 2 * 3 * 4 * 5
    with pytest.raises(HipLibraryError, match='null pointer'):
        lov.plov_sort_descending(None, 3, 5, None, None, None, 0, None)
    with pytest.raises(HipLibraryError, match='K = 40'):
        lov.plov_loss_bwd(8, 8, 2, 40, 4, 4, 0, 0, 0, 8, 8, 8, 8, None)
    with pytest.raises(HipLibraryError, match='is missing'):
        _lov._LovLib(os.path.join(ROOT, 'no_such_dir', 'libpacingpseudo_lov.so')).load()


# ---------------------------------------------------------------- the host half under AddressSanitizer
def test_lov_host_side_under_address_sanitizer():
    """`make asan-lov` instruments the host half of pp_lovasz.hip and runs tests/native/asan_lov_args.cpp, a program of its own that
    feeds every plov_* entry point the arguments it must refuse before any launch.  Nothing is loaded into Python."""
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-lov'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
