"""Fused AdamW (``--optimizer adamw [--wd_exempt_1d]``; libpacingpseudo_opt.so), the parts that need no GPU: the parsers' flags, the
resume tables, every refusal of ``FusedAdamW``, the exemption mask on the small model's slab, header / binding / library agreeing
symbol for symbol, and the host half of the library under AddressSanitizer."""
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------- 1. parsers
def _parsers():
    from pacingpseudo_amd import train, upper_bound
    return ((train, train.parse_args, ['--tag', 'x']), (upper_bound, upper_bound.parse_args, ['--tag', 'x']))


def test_parser_flags_and_defaults():
    for mod, parse, base in _parsers():
        a = parse(base)
        assert a.optimizer == 'adam' and a.wd_exempt_1d is False and a.wd == 0.0003, mod.__name__
        a = parse(base + ['--optimizer', 'adamw'])
        assert a.optimizer == 'adamw' and a.wd_exempt_1d is False
        a = parse(base + ['--optimizer', 'adamw', '--wd_exempt_1d', '--wd', '0.01'])
        assert a.optimizer == 'adamw' and a.wd_exempt_1d is True and a.wd == 0.01          # --wd is used as given
        helps = {act.dest: act.help for act in mod.parser._actions}
        assert 'untuned first value' in helps['wd'] and 'not comparable' in helps['wd'], mod.__name__
        assert 'adamw' in helps['wd_exempt_1d']
    from pacingpseudo_amd import train, upper_bound
    assert train.parse_args(['--tag', 'x', '--optimizer', 'momentum']).optimizer == 'momentum'
    with pytest.raises(SystemExit) as e:          # the supervised driver has no momentum optimizer, as before
        upper_bound.parse_args(['--tag', 'x', '--optimizer', 'momentum'])
    assert e.value.code == 2


def test_exemption_with_adam_or_momentum_is_a_parser_error(capsys):
    from pacingpseudo_amd import train, upper_bound
    for parse, argv in ((train.parse_args, ['--wd_exempt_1d']), (train.parse_args, ['--wd_exempt_1d', '--optimizer', 'adam']),
                        (train.parse_args, ['--wd_exempt_1d', '--optimizer', 'momentum']),
                        (upper_bound.parse_args, ['--wd_exempt_1d']), (upper_bound.parse_args, ['--wd_exempt_1d', '--optimizer', 'adam'])):
        with pytest.raises(SystemExit) as e:
            parse(['--tag', 'x'] + argv)
        assert e.value.code == 2, argv
        assert '--wd_exempt_1d needs --optimizer adamw' in capsys.readouterr().err


# ---------------------------------------------------------------- 2. resume
def test_resume_tables_and_older_state_files():
    from pacingpseudo_amd import resume, train, upper_bound
    assert resume.ABSENT_DEFAULTS['wd_exempt_1d'] is False
    assert 'wd_exempt_1d' not in resume.MAY_DIFFER and 'optimizer' not in resume.MAY_DIFFER and 'wd' not in resume.MAY_DIFFER
    assert train.parser.get_default('wd_exempt_1d') is False and upper_bound.parser.get_default('wd_exempt_1d') is False
    for parse in (train.parse_args, upper_bound.parse_args):
        new = resume.flag_dict(parse(['--tag', 'x']))
        old = {k: v for k, v in new.items() if k != 'wd_exempt_1d'}          # a state file written before the flag existed
        resume.check_compatible(old, new, 1, 1)
        w = resume.flag_dict(parse(['--tag', 'x', '--optimizer', 'adamw']))
        on = resume.flag_dict(parse(['--tag', 'x', '--optimizer', 'adamw', '--wd_exempt_1d']))
        resume.check_compatible(w, dict(w), 1, 1)
        resume.check_compatible(on, dict(on), 1, 1)
        for saved, now in ((old, w), (new, w), (w, new)):
            with pytest.raises(resume.ResumeError, match='--optimizer ') as e:
                resume.check_compatible(saved, now, 1, 1)
            assert '--wd_exempt_1d' not in str(e.value)
        for saved, now in ((w, on), (on, w)):
            with pytest.raises(resume.ResumeError, match='--wd_exempt_1d') as e:
                resume.check_compatible(saved, now, 1, 1)
            assert '--optimizer ' not in str(e.value)
        with pytest.raises(resume.ResumeError, match='--optimizer .*--wd_exempt_1d'):          # an old file resumed with both
            resume.check_compatible(old, on, 1, 1)


# ---------------------------------------------------------------- 3. FusedAdamW validation
def _param():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_fused_adamw_validation_and_param_groups():
    from pacingpseudo_amd.optim import FusedAdam, FusedAdamW, FusedSGD, _SlabOptimizer
    assert issubclass(FusedAdamW, _SlabOptimizer) and FusedAdamW.STATE_KEYS == ('m', 'v')
    opt = FusedAdamW(_param())
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], g['exempt_1d'], g['max_grad_norm'], g['ema_decay']) == \
        (1e-3, (0.9, 0.999), 1e-8, 1e-2, False, None, None)
    for kw in (dict(lr=-1e-3), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(lr=math.nan), dict(eps=math.nan),
               dict(weight_decay=math.nan), dict(lr=math.inf), dict(weight_decay=math.inf), dict(betas=(1.0, 0.999)),
               dict(betas=(0.9, -0.1)), dict(betas=(0.9, math.nan)), dict(betas=(0.9,))):
        with pytest.raises(ValueError):
            FusedAdamW(_param(), **kw)
    # max_grad_norm / ema_decay: the checks of the other two classes
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=math.nan), dict(ema_decay=0.0), dict(ema_decay=1.0),
               dict(ema_decay=-0.5), dict(ema_decay=math.nan)):
        for cls in (FusedAdamW, FusedAdam, FusedSGD):
            with pytest.raises(ValueError):
                cls(_param(), **kw)
    ok = FusedAdamW(_param(), max_grad_norm=math.inf, ema_decay=0.9, exempt_1d=1)
    assert ok.param_groups[0]['max_grad_norm'] == math.inf and ok.param_groups[0]['ema_decay'] == 0.9
    assert ok.param_groups[0]['exempt_1d'] is True
    with pytest.raises(NotImplementedError):
        ok.step(closure=lambda: 0.0)


def test_exempt_1d_travels_with_the_state_dict():
    from pacingpseudo_amd.optim import FusedAdamW
    on = FusedAdamW(_param(), lr=2e-3, weight_decay=0.05, exempt_1d=True)
    sd = on.state_dict()
    assert sd['param_groups'][0]['exempt_1d'] is True and sd['param_groups'][0]['weight_decay'] == 0.05 and sd['slabs'] == []
    off = FusedAdamW(_param())
    off.load_state_dict(sd)
    assert off.param_groups[0]['exempt_1d'] is True and off.param_groups[0]['weight_decay'] == 0.05 and off.param_groups[0]['lr'] == 2e-3
    older = dict(sd, param_groups=[{k: v for k, v in sd['param_groups'][0].items() if k != 'exempt_1d'}])
    was_on = FusedAdamW(_param(), exempt_1d=True)
    was_on.load_state_dict(older)          # a state dict older than the key: off
    assert was_on.param_groups[0]['exempt_1d'] is False
    assert was_on.param_groups[0]['max_grad_norm'] is None and was_on.param_groups[0]['ema_decay'] is None


def test_graph_key_names_the_exemption():
    src = open(os.path.join(ROOT, 'pacingpseudo_amd', 'graph.py')).read()
    key = src[src.index('def _key'):src.index('def _capture')]
    assert "g.get('exempt_1d'" in key and "g.get('weight_decay'" in key


# ---------------------------------------------------------------- 4. the mask
def _small_slab():
    """The slab of smoke()'s small model, on the host: the segments ConsistencyRegulr flattens on the device."""
    from oracle import pacing_oracle as O
    from pacingpseudo_amd.flat import FlatSlab
    from pacingpseudo_amd.models import ConsistencyRegulr
    args = O.full_flags(init_ch=8, max_ch=64, hid_ch=16, feat_ch=[64, 64])
    torch.manual_seed(1)
    model = ConsistencyRegulr(
        kwargs_unet=dict(input_ch=1, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=5, output_stride=8,
                         is_stride_conv=False, is_trans_conv=False, elab_end_points=True),
        kwargs_aux_path=dict(num_classes=5, feat_stage=args.feat_stage, feat_ch=args.feat_ch, hid_ch=args.hid_ch,
                             aux_drop_prob=0.0, do_memory=True, max_step=args.epoch, update_momentum=0.9,
                             ensemble_mode='cosine_similarity'),
        args_parser=args)
    flat = FlatSlab([('backbone', [p for p in model.backbone.parameters() if p.requires_grad]),
                     ('aux_path', [p for p in model.aux_path.parameters() if p.requires_grad])])
    return model, flat


def test_decay_exempt_mask_on_the_small_model():
    from pacingpseudo_amd.optim import decay_exempt_mask
    model, flat = _small_slab()
    mask = decay_exempt_mask(flat)
    assert mask.dtype == torch.uint8 and mask.shape == (flat.numel,) and not mask.is_cuda
    assert set(mask.unique().tolist()) == {0, 1}
    covered = torch.zeros(flat.numel, dtype=torch.bool)
    one_d = four_d = n_one_d = n_four_d = 0
    unaligned = []
    for p, off in flat.offsets.items():
        sl = slice(off, off + p.numel())
        covered[sl] = True
        if p.ndim <= 1:
            assert bool(mask[sl].all()), (tuple(p.shape), off)          # every element of every ndim <= 1 parameter
            one_d += 1
            n_one_d += p.numel()
            if off % 4:
                unaligned.append(off)
        else:
            assert p.ndim == 4 and not bool(mask[sl].any()), (tuple(p.shape), off)          # no element of a 4-D one
            four_d += 1
            n_four_d += p.numel()
    # (the model has a 26th 4-D parameter of 80 elements, the memory bank: it takes no gradient and is not in the slab)
    assert (one_d, n_one_d) == (70, 2645) and (four_d, n_four_d) == (25, 508800)
    assert int(mask.sum()) == 2645          # exactly: nothing else is marked ...
    assert not bool(mask[~covered].any())          # ... no padding element in particular
    assert flat.numel >= n_one_d + n_four_d and int((~covered).sum()) == flat.numel - n_one_d - n_four_d
    # The point of a per-element decision: a boundary between marked and unmarked elements inside a 16-byte lane.  On this model
    # every channel count but the 5 classes is a multiple of 8, so every marked run STARTS on a lane (`unaligned` is empty: measured,
    # not assumed) and the boundary inside a lane is the END of final_conv.bias, one marked element and three of padding in one
    # lane.  Asserted, so that the test cannot lose its point if the model changes; a run that starts inside a lane is the next test.
    change = ((mask[1:] != mask[:-1]).nonzero().flatten() + 1).tolist()
    inside = [c for c in change if c % 4]
    assert inside, 'no marked run begins or ends inside a 16-byte lane: the model changed and this test lost its point'
    names = {id(p): k for k, p in model.named_parameters()}
    ends = {off + p.numel(): names[id(p)] for p, off in flat.offsets.items() if p.ndim <= 1}
    assert unaligned == [] and [ends.get(c) for c in inside] == ['backbone.final_conv.bias']
    for a, b in flat.segments.values():
        assert a % 4 == 0 and b % 4 == 0          # what keeps `exempt + a` 4-byte aligned


def test_decay_exempt_mask_with_runs_that_start_inside_a_lane():
    """Channel counts that are no multiple of 4 (three classes, seven channels): marked runs start and end at every residue."""
    from pacingpseudo_amd.flat import FlatSlab
    from pacingpseudo_amd.optim import decay_exempt_mask
    shapes = {'a': [(7, 1, 3, 3), (7,), (7,), (7,), (3, 7, 1, 1), (3,)], 'b': [(), (5, 3, 1, 1), (5,), (2, 5)]}
    segs = [(name, [torch.nn.Parameter(torch.randn(s)) for s in ss]) for name, ss in shapes.items()]
    flat = FlatSlab(segs)
    mask = decay_exempt_mask(flat)
    want = torch.zeros(flat.numel, dtype=torch.uint8)
    starts = []
    for _, ps in segs:
        for p in ps:
            if p.ndim <= 1:
                o = flat.offsets[p]
                want[o:o + p.numel()] = 1
                starts.append(o)
    assert torch.equal(mask, want) and int(mask.sum()) == 7 * 3 + 3 + 1 + 5
    runs = [i for i in range(flat.numel) if mask[i] and (i == 0 or not mask[i - 1])]
    assert runs == [63, 105, 124] and {s % 4 for s in runs} == {3, 1, 0}          # 63: behind 7 * 9 weights; 105: bias and the 0-d one
    assert flat.segments == {'a': (0, 108), 'b': (108, 140)} and flat.numel == 140
    assert mask[108] == 1 and mask[109] == 0          # the 0-d parameter is exempt, the weight behind it is not
    assert not bool(mask[129:].any())          # the 2-D parameter and the element of padding behind it


# ---------------------------------------------------------------- 5. header / binding / library
def _header_decls():
    header = open(os.path.join(ROOT, 'include', 'pacingpseudo_opt.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(popt_\w+)\s*\(([^;{]*)\)\s*;', header):
        params = m.group(2).strip()
        decls[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    return decls


def test_header_binding_and_library_agree():
    from pacingpseudo_amd import _lib, _opt
    decls = _header_decls()
    assert len(decls) == 6
    assert list(decls) == list(_opt.EXPORTED_SYMBOLS) == list(_opt._PROTOS)
    for name, (_, argtypes) in _opt._PROTOS.items():
        assert decls[name] == len(argtypes), name
    assert (decls['popt_adamw_step'], decls['popt_adamw_step_clip'], decls['popt_adamw_step_ema']) == (16, 17, 19)
    path = os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'optim', 'pp_adamw.hip')
    src = open(path).read()
    assert int(re.search(r'#define POPT_VERSION (\d+)', src).group(1)) == _opt.MIN_OPT_VERSION == 100
    defined = {}
    for m in re.finditer(r'extern "C"[^\n(]*?\b(popt_\w+)\s*\(([^{;]*)\)\s*\{', src):
        params = m.group(2).strip()
        defined[m.group(1)] = 0 if params in ('', 'void') else len(params.split(','))
    assert defined == decls          # symbol for symbol, parameter count for parameter count
    code = re.sub(r'//.*', '', src)
    assert 'asm' not in code and 'getenv' not in src and '#include "pp_' not in src          # self-contained
    assert not re.findall(r'\batomic\w+', code)
    for banned in ('hipDeviceSynchronize', 'hipStreamSynchronize', 'hipEventSynchronize', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset',
                   'malloc(', 'new '):
        assert banned not in code, banned
    assert 'fp contract(off)' in src
    assert 'float4' in code and 'const unsigned int*' in code          # 16-byte lanes, one 4-byte load of the mask per lane
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith('popt_')]          # the per-step library is as it was
    runtime = open(os.path.join(ROOT, 'pacingpseudo_amd', 'csrc', 'pp_runtime.cpp')).read()
    assert int(re.search(r'#define PP_VERSION (\d+)', runtime).group(1)) == 606
    if os.path.exists(_opt.OPT_LIB_PATH):
        import ctypes
        dll = ctypes.CDLL(_opt.OPT_LIB_PATH)
        for name in decls:
            assert hasattr(dll, name), name
        out = subprocess.run(['nm', '-D', '--defined-only', _opt.OPT_LIB_PATH], capture_output=True, text=True)
        if out.returncode == 0:
            exported = sorted(s for s in (ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()) if s.startswith('popt_'))
            assert exported == sorted(decls)


def test_build_loads_and_checks_the_library():
    from tests._wiring import wired
    wired('opt', 'pacingpseudo_amd/csrc/optim/pp_adamw.hip')


def test_library_loads_without_a_gpu_and_refuses_bad_arguments():
    from pacingpseudo_amd import _opt
    from pacingpseudo_amd._lib import HipLibraryError
    if not os.path.exists(_opt.OPT_LIB_PATH):
        pytest.skip('libpacingpseudo_opt.so is not built')
    lib = _opt._OptLib()
    assert lib.popt_version() >= _opt.MIN_OPT_VERSION
    assert lib.popt_trip_elements() > 0 and lib.popt_trip_elements() % (4 * 256) == 0
    nan, inf = math.nan, math.inf
    P = 4096          # an aligned address that is never dereferenced: every call below is refused before any launch

    def plain(p=P, g=P, m=P, v=P, n=64, lr=1e-3, lr_dev=None, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, step=P, skip=None, ex=None):
        return (p, g, m, v, n, lr, lr_dev, b1, b2, eps, wd, step, skip, 1, ex)

    forms = (lambda **kw: lib.popt_adamw_step(*plain(**kw), None),
             lambda **kw: lib.popt_adamw_step_clip(*plain(**kw), P, None),
             lambda **kw: lib.popt_adamw_step_ema(*plain(**kw), P, 0.9, None, None),
             lambda **kw: lib.popt_adamw_step_ema(*plain(**kw), P, 0.9, P, None))
    cases = {
        'null pointer': [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=None)],
        'need n >= 1': [dict(n=0), dict(n=-4)],
        'slabs must be 16-byte aligned': [dict(p=P + 4), dict(g=P + 8), dict(m=P + 12), dict(v=P + 4)],
        'exempt must be 4-byte aligned': [dict(ex=P + 1), dict(ex=P + 2), dict(ex=P + 3)],
        'must be 4-byte aligned': [dict(lr_dev=P + 2), dict(step=P + 1), dict(skip=P + 2)],
        'lr must be finite and >= 0': [dict(lr=-1e-3), dict(lr=nan), dict(lr=inf)],
        'eps must be finite and >= 0': [dict(eps=-1e-8), dict(eps=nan), dict(eps=inf)],
        'weight_decay must be finite and >= 0': [dict(wd=-0.1), dict(wd=nan), dict(wd=inf)],
        r'betas must lie in \[0, 1\)': [dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-0.5), dict(b2=nan)],
    }
    for msg, kws in cases.items():
        for kw in kws:
            for i, form in enumerate(forms):
                with pytest.raises(HipLibraryError, match=r'rc=-1\).*' + msg):
                    form(**kw)
                    pytest.fail(f'form {i} accepted {kw}')
    own = {
        'clip_dev is required': [lambda: lib.popt_adamw_step_clip(*plain(), None, None)],
        'must be 4-byte aligned': [lambda: lib.popt_adamw_step_clip(*plain(), P + 2, None),
                                   lambda: lib.popt_adamw_step_ema(*plain(), P, 0.9, P + 1, None)],
        'ema is required': [lambda: lib.popt_adamw_step_ema(*plain(), None, 0.9, None, None)],
        'slabs must be 16-byte aligned': [lambda: lib.popt_adamw_step_ema(*plain(), P + 4, 0.9, None, None)],
        r'ema_decay must lie in \(0, 1\)': [lambda d=d: lib.popt_adamw_step_ema(*plain(), P, d, None, None) for d in (0.0, 1.0, -0.5, 1.5, nan)],
    }
    for msg, fs in own.items():
        for f in fs:
            with pytest.raises(HipLibraryError, match=r'rc=-1\).*' + msg):
                f()


def test_missing_or_stale_library_raises(tmp_path):
    from pacingpseudo_amd import _opt
    from pacingpseudo_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match='is missing.*make opt'):
        _opt._OptLib(str(tmp_path / 'nope.so')).popt_version()
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler for the stale-library stand-ins')
    for tag, body, msg in (('old', 'int popt_version(void) { return 99; }', 'popt_version\\(\\) = 99.*make opt'),
                           ('part', 'int popt_version(void) { return 100; } const char* popt_last_error(void) { return ""; }',
                            'lacks 4 entry.*make opt')):
        c = tmp_path / f'{tag}.c'
        c.write_text(body)
        so = tmp_path / f'lib{tag}.so'
        subprocess.run([cc, '-shared', '-fPIC', str(c), '-o', str(so)], check=True)
        with pytest.raises(HipLibraryError, match=msg):
            _opt._OptLib(str(so)).load()


def test_the_binding_is_not_loaded_at_import():
    code = ('import pacingpseudo_amd, pacingpseudo_amd.utils, pacingpseudo_amd.train, pacingpseudo_amd.upper_bound, pacingpseudo_amd.optim, sys\n'
            'from pacingpseudo_amd import _opt\n'
            'assert _opt.opt._dll is None\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---------------------------------------------------------------- 6. the host half under AddressSanitizer
def test_opt_host_side_under_address_sanitizer():
    """`make asan-opt` instruments the host half of pp_adamw.hip and runs tests/native/asan_opt_args.cpp, a program of its own that
    feeds every popt_* entry point the arguments it must refuse before any launch.  Nothing is loaded into Python."""
    if shutil.which('hipcc') is None or not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'):
        pytest.skip('hipcc / the ROCm clang++ are not installed: the sanitizer build cannot be made here')
    r = subprocess.run(['make', '-C', ROOT, '-j', '4', 'asan-opt'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'all argument checks rejected their input' in r.stdout
