"""Cross-stream ordering of a training step, proven from a recorded launch log (host code only: no GPU is needed to import this).

Three parts.

Recorder -- `Recording` generalises the `_Recorder` of tests/_launch_census.py: every binding of the entry-point table a training
step reaches (engine.lib_for, engine.lib, optim.lib, losses.losses.lib, convop.lib, and _lib.lib for the call-time imports of
models/aux_path_memory.py) is a logging proxy for the duration of a recording, and so are torch's ordering calls (Event.record /
wait / synchronize, Stream.wait_event / wait_stream / record_event / synchronize, torch.cuda.synchronize), all through a
pytest MonkeyPatch.  The log is one host-ordered list of plain tuples (picklable):
    ('L', entry point, [argument values], stream)     a launch; pointers as integers (None: null), a pp_lazy_in as
                                                      ('lazy', coef, ld, groups), a host item table as ('items', [{field: value}]),
                                                      an array of device pointers as ('ptrs', [...]), other host memory as ('host',)
    ('R', event, stream)                              event recorded on stream
    ('W', event, stream, site)                        stream waits for event; site = name of the function that asked
    ('WS', waiting stream, awaited stream)            Stream.wait_stream
    ('B',) / ('SS', stream) / ('ES', event)           host barriers: device, stream, event
Streams are their hipStream_t handles (0: the null stream), events small integers (`Recording.event_names` labels the plan's).

Access table -- `TABLE`: one row per entry point a step launches; per pointer parameter the mode ('r', 'w', 'rw', or
'w+<flag>': written, and read as well when the call's accumulate flag <flag> is non-zero) and the extent as a strided box
(base, rows, row_bytes, stride_bytes) computed from the call's own arguments.  Parameter names come from
include/pacingpseudo_hip.h (parsed as tests/test_abi.py parses it), element sizes from the prototype that was really called
(pp_h16_t / pp_bf16_t in the _h16 / _bf16 headers: 2 bytes).  NHWC operands are P rows of C elements with stride ld, workspaces
are workspace_bytes, parameter gradients / coefficient rows / sums have the sizes the header states.  The WRITE extents are the
columns tests/test_gpu_conv_census.py and tests/test_gpu_stream_census.py already hold to canaries (a launch that wrote outside
them fails there), so an extent here is not this file's own claim about the kernels.

Checker -- `check(log)`: vector clocks over the log.  Streams execute in order; a wait binds to the latest record of its event
that precedes it in host order (none: it orders nothing); a host barrier orders everything before it against everything after
it.  Reported is every pair of launches on different streams whose extents overlap, of which at least one writes, and which
the clocks leave unordered.  Two boxes with the same stride and disjoint column ranges do not overlap; any other two boxes
whose hulls intersect do.
"""
import ctypes
import functools
import os
import re
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, 'include', n) for n in ('pacingpseudo_hip.h', 'pacingpseudo_hip_h16.h', 'pacingpseudo_hip_bf16.h')]

# ------------------------------------------------------------------------------------------------------------ header
Param = namedtuple('Param', 'name ctype pointer size')       # size: bytes per element a pointer parameter points at (void: 1)
_ELEM = {'float': 4, 'double': 8, 'int': 4, 'int64_t': 8, 'int32_t': 4, 'pp_h16_t': 2, 'pp_bf16_t': 2, 'void': 1, 'char': 1,
         'unsigned char': 1, 'unsigned long long': 8, 'long long': 8, 'size_t': 8}


@functools.lru_cache(maxsize=None)
def header_params():
    """{entry point: [Param, ...]} from the three headers (comments stripped, the declarations as tests/test_abi.py finds them)."""
    out = {}
    for path in HEADERS:
        txt = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
        for m in re.finditer(r'\b(?:int|size_t|const char\*)\s+(pp_\w+)\s*\(([^;]*?)\)\s*;', txt, flags=re.S):
            args = m.group(2).strip()
            params = []
            if args not in ('', 'void'):
                for a in args.split(','):
                    a = ' '.join(a.split())
                    mm = re.match(r'^(.*?)(\w+)$', a)
                    ctype, name = mm.group(1).strip(), mm.group(2)
                    base = ctype.replace('const', '').replace('*', '').strip()
                    params.append(Param(name, ctype, '*' in ctype, _ELEM.get(base, 0)))
            out[m.group(1)] = params
    return out


# ------------------------------------------------------------------------------------------------------------ recorder
def _decode(t, a):
    from pacingpseudo_amd import _lib
    if t is _lib.lazy_p:
        if a is None:
            return None
        o = a._obj
        return ('lazy', o.coef, o.ld, o.groups)
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return None if a is None else ('host',)                      # int* rows_out and the like: host memory
    if t is ctypes.c_void_p:
        if a is None:
            return None
        if isinstance(a, ctypes.Array):
            if issubclass(a._type_, ctypes.Structure):
                return ('items', [{f: getattr(it, f) for f, _ in it._fields_} for it in a])
            if a._type_ is ctypes.c_void_p:
                return ('ptrs', [v for v in a])
            return ('host',)
        if isinstance(a, ctypes.c_void_p):
            return a.value
        return int(a)
    if t is ctypes.c_char_p:
        return ('host',)
    return float(a) if isinstance(a, float) else int(a)


class _Proxy:
    """Stands in for an entry-point table (a _Lib, an _H16Lib or another _Proxy): launches are logged and forwarded unchanged."""

    def __init__(self, inner, suffix, rec):
        self._inner, self._suffix, self._rec = inner, suffix, rec

    def __getattr__(self, name):
        from pacingpseudo_amd import _lib
        from tests._launch_census import is_launch
        fn = getattr(self._inner, name)
        if not is_launch(name):
            return fn
        rec = self._rec
        real = name + self._suffix if (self._suffix and name in _lib._H16_SET) else name

        def call(*a):
            if not rec.active or rec.depth:          # (a proxy behind a proxy: the outer one has logged this launch)
                return fn(*a)
            types = _lib._PROTOS[name][1]
            vals = [_decode(t, v) for t, v in zip(types, a)]
            stream = vals[-1] or 0
            if rec.before_launch is not None:
                rec.before_launch(real, stream)
            rec.log.append(('L', real, vals[:-1], stream))
            rec.depth += 1
            try:
                return fn(*a)
            finally:
                rec.depth -= 1
        call._pp_hazard_proxy = True
        return call


class Recording:
    """with Recording(monkeypatch) as rec: ... -> rec.log.  `before_launch(entry, stream)`, when set, runs in front of every
    launch (the held-back runs enqueue their delay there)."""

    def __init__(self, monkeypatch, before_launch=None):
        self.mp = monkeypatch
        self.log = []
        self.active = False
        self.depth = 0
        self.sync_depth = 0
        self.before_launch = before_launch
        self._events = {}            # id(event) -> index
        self._keep = []              # the event objects, so that no id is handed out twice
        self.event_names = {}

    def ev(self, e):
        i = self._events.get(id(e))
        if i is None:
            i = self._events[id(e)] = len(self._keep)
            self._keep.append(e)
        return i

    def name_events(self, plan, extra=None):
        """Label the plan's events: 'dz_ready', 'wg_done', 'bucket_ev', 'aux_fork', 'aux_join' (+ extra {name: event})."""
        for kind in ('dz_ready', 'wg_done'):
            for e in getattr(plan, kind, None) or []:
                self.event_names[self.ev(e)] = kind
        for kind in ('bucket_ev', 'aux_fork', 'aux_join'):
            e = getattr(plan, kind, None)
            if e is not None:
                self.event_names[self.ev(e)] = kind
        for k, e in (extra or {}).items():
            self.event_names[self.ev(e)] = k

    # ---- patches
    def _sync_patch(self, owner, attr, entry):
        real = getattr(owner, attr)
        rec = self

        def patched(*a, **k):
            if rec.active and rec.sync_depth == 0:
                site = sys._getframe(1).f_code.co_name
                rec.log.append(entry(site, *a, **k))
            rec.sync_depth += 1
            try:
                return real(*a, **k)
            finally:
                rec.sync_depth -= 1
        self.mp.setattr(owner, attr, patched)

    def __enter__(self):
        import torch
        from pacingpseudo_amd import _lib, convop, engine, optim
        from pacingpseudo_amd.losses import losses
        cur = lambda: torch.cuda.current_stream().cuda_stream       # noqa: E731
        sid = lambda s: cur() if s is None else s.cuda_stream      # noqa: E731
        Ev, St = torch.cuda.Event, torch.cuda.Stream
        self._sync_patch(Ev, 'record', lambda site, e, stream=None: ('R', self.ev(e), sid(stream)))
        self._sync_patch(Ev, 'wait', lambda site, e, stream=None: ('W', self.ev(e), sid(stream), site))
        self._sync_patch(Ev, 'synchronize', lambda site, e: ('ES', self.ev(e)))
        self._sync_patch(St, 'wait_event', lambda site, s, e: ('W', self.ev(e), s.cuda_stream, site))
        self._sync_patch(St, 'wait_stream', lambda site, s, other: ('WS', s.cuda_stream, other.cuda_stream))
        self._sync_patch(St, 'synchronize', lambda site, s: ('SS', s.cuda_stream))
        self._sync_patch(torch.cuda, 'synchronize', lambda site, *a, **k: ('B',))
        # Stream.record_event: an event given by the caller is recorded on the stream; a fresh one comes back from the real call
        real_re = St.record_event
        rec = self

        def record_event(s, event=None):
            rec.sync_depth += 1
            try:
                e = real_re(s, event)
            finally:
                rec.sync_depth -= 1
            if rec.active and rec.sync_depth == 0:
                rec.log.append(('R', rec.ev(e), s.cuda_stream))
            return e
        self.mp.setattr(St, 'record_event', record_event)

        real_for = engine.lib_for

        def lib_for(storage):
            s = {4: 'fp32', 2: 'fp16'}.get(storage, storage)
            return _Proxy(real_for(storage), {'fp32': '', 'fp16': '_h16', 'bf16': '_bf16'}[s], self)
        self.mp.setattr(engine, 'lib_for', lib_for)
        base = _Proxy(_lib.lib, '', self)
        for mod in (engine, optim, losses, convop, _lib):
            self.mp.setattr(mod, 'lib', base)
        self.active = True
        return self

    def __exit__(self, *exc):
        from pacingpseudo_amd import _lib
        self.active = False
        self.before_launch = None
        for table in (_lib.lib_h16, _lib.lib_bf16):      # an _H16Lib caches what it resolved: drop the proxies' closures
            for k, v in list(vars(table).items()):
                if getattr(v, '_pp_hazard_proxy', False):
                    delattr(table, k)
        return False


# ------------------------------------------------------------------------------------------------------------ access table
# A row: {parameter: (mode, kind, *expressions)}.  Expressions are evaluated over the call's arguments by name (plus `es`, the
# element size of THIS parameter, and the host queries below).  Kinds:
#   ('nhwc', P, C, ld)   P rows of C elements with stride ld elements
#   ('n', count)         `count` contiguous elements (bytes for a void*)
#   ('bytes', count)     `count` contiguous bytes, whatever the pointer's type (workspaces)
#   ('lazy', C)          the coefficient rows of a pp_lazy_in: groups * 3 rows of C floats with stride ld
#   ('coefrows', C, ld, groups)   the same for a bare pointer (pp_bn_train_finalize_lazy)
#   ('items', {field: (mode, count)})   a host item table: one access per item and device-pointer field
#   ('ptrs', count)      an array of device pointers, `count` elements behind each
#   ('host',)            host memory: no device access
def _lib_query(name, *a):
    from pacingpseudo_amd._lib import lib
    return int(getattr(lib, name)(*a))


@functools.lru_cache(maxsize=None)
def _planes(H, W, dil):
    return (_lib_query('pp_conv3x3_wino_tile', H, W, dil) + 2) ** 2


@functools.lru_cache(maxsize=None)
def _vkeep(C, B, H, W, dil):
    return _lib_query('pp_conv3x3_wino_vkeep_elems', C, B, H, W, dil)


@functools.lru_cache(maxsize=None)
def _sumsq_rows(n):
    return _lib_query('pp_grad_sumsq_rows', n)


_QUERIES = dict(planes=_planes, vkeep=_vkeep, sumsq_rows=_sumsq_rows, max=max, min=min)

R, W_, RW = 'r', 'w', 'rw'
WS = (RW, 'bytes', 'workspace_bytes')


def _act(mode, P, C, ld):
    return (mode, 'nhwc', P, C, ld)


def _n(mode, count):
    return (mode, 'n', count)


def _conv_fwd(w_count, extra=None, acc=True):
    row = {'in': _act(R, 'B*H*W', 'C', 'ld_in'), 'bias': _n(R, 'N'), 'out': _act('w+accumulate' if acc else W_, 'B*H*W', 'N', 'ld_out')}
    row.update(w_count)
    row.update(extra or {})
    return row


_BN_FWD_TAIL = {'scale': _n(R, 'N'), 'shift': _n(R, 'N'), 'stats': (W_, 'bytes', 'stats_bytes'), 'rows_out': ('r', 'host')}
_WINO_WS = {'workspace': WS, 'v_keep': _n(W_, 'vkeep(C, B, H, W, dil)')}
_GC = 'groups*C'
_BN_ROWS = {k: _n(R, _GC) for k in ('scale', 'shift', 'save_mean', 'save_invstd')}
_PGRADS = {k: _n('w+accumulate_param_grads', 'C') for k in ('dgamma', 'dbeta', 'dbias_conv')}


def _bn_bwd(P, rows=_BN_ROWS, z='z', pool=None, dz=True, amax=True, ws=True, extra=None):
    row = {'dy': _act(R, P, 'C', 'ld_dy'), z: _act(R, P, 'C', 'ld_' + z), 'gamma': _n(R, 'C')}
    row.update(rows)
    row.update(_PGRADS)
    if pool:
        row['dpool'] = _act(R, pool, 'C', 'ld_dpool')
    if dz:
        row['dz'] = _act(W_, P, 'C', 'ld_dz')
    if amax:
        row['dz_amax'] = _n(RW, '1')
    if ws:
        row['workspace'] = WS
    row.update(extra or {})
    return row


_EVAL_ROWS = {'scale': _n(R, 'C'), 'beta': _n(R, 'C')}
_GN_ROWS = {k: _n(R, 'N*C') for k in ('scale', 'shift', 'save_mean', 'save_invstd', 'save_xbar')}
_WG = {'dz': _act(R, 'B*H*W', 'O', 'ld_dz'), 'x': _act(R, 'B*H*W', 'Cpad', 'ld_x'), 'dw_oihw': _n('w+accumulate', 'O*I_true*9'),
       'workspace': WS}
_WINO_WG = {'dz': _act(R, 'B*H*W', 'O', 'ld_dz'), 'x': _act(R, 'B*H*W if v_cached is None else 0', 'C', 'ld_x'),
            'dw_oihw': _n('w+accumulate', 'O*C*9'), 'v_cached': _n(R, 'vkeep(C, B, H, W, dil)'), 'workspace': WS}
_BWD_DATA = {'dz': _act(R, 'B*H*W', 'O', 'ld_dz'), 'dx': _act('w+accumulate', 'B*H*W', 'I', 'ld_dx')}
_C1 = {'dw_o1hw': _n('w+accumulate_dw', 'C*9')}
_FINALIZE = {'sums': _n(R, 'groups*rows*2*C'), 'gamma': _n(R, 'C'), 'beta': _n(R, 'C'), 'running_mean': _n(RW, 'C'),
             'running_var': _n(RW, 'C'), 'num_batches_tracked': _n(RW, '1'), 'save_mean': _n(W_, _GC), 'save_invstd': _n(W_, _GC),
             'scale': _n(W_, _GC), 'shift': _n(W_, _GC)}
_NKHW = 'N*K*H*W'
_CRF_FWD = {'logits': _n(R, _NKHW), 'image': _n(R, 'N*C*H*W'), 'valid_mask': _n(R, 'N*H*W'), 'unit_grad': _n(W_, _NKHW),
            'sums': _n(W_, '2'), 'workspace': WS}
_OPT_HEAD = {'p': _n(RW, 'n'), 'g': _n(R, 'n'), 'lr_dev': _n(R, '1'), 'step_dev': _n(RW, '1'), 'skip': _n(RW, '2'),
             'clip_dev': _n(R, '1'), 'ema': _n(RW, 'n')}
_ADAM = dict(_OPT_HEAD, m=_n(RW, 'n'), v=_n(RW, 'n'))
_SGD = dict(_OPT_HEAD, momentum_buf=_n(RW, 'n'))
_PACK_ITEM = {'w_oihw': (R, 'O*I*9'), 'wf16': (W_, 'O*9*Ipad'), 'wb16': (W_, 'I*9*O')}
_WINO_ITEM = {'w_oihw': (R, 'O*I*9'), 'Uf16': (W_, '36*O*I'), 'Ub16': (W_, '36*O*I')}
_COEF_ITEM = dict({k: (R, 'C') for k in ('gamma', 'beta', 'running_mean', 'running_var')},
                  **{k: (W_, _GC) for k in ('save_mean', 'save_invstd', 'scale', 'shift')})

TABLE = {
    # ---- layout / packs
    'pp_pack_image_nchw_to_nhwc': {'src': _n(R, 'N*C*H*W'), 'dst': _act(W_, 'N*H*W', 'Cpad', 'ld_dst')},
    'pp_pack_conv3x3_weights': {'w_oihw': _n(R, 'O*I*9'), 'wf': _n(W_, 'O*9*Ipad'), 'wb': _n(W_, 'I*9*O')},
    'pp_pack_conv3x3_weights_f16x3': {'w_oihw': _n(R, 'O*I*9'), 'wf16': _n(W_, 'O*9*Ipad*4'), 'wb16': _n(W_, 'I*9*O*4')},
    'pp_pack_conv3x3_weights_f16x3_batch': {'items': (R, 'items', _PACK_ITEM)},
    'pp_wino_pack_weights': {'w_oihw': _n(R, 'O*I*9'), 'Uf': _n(W_, '(tile+2)**2*O*I'), 'Ub': _n(W_, '(tile+2)**2*O*I')},
    'pp_wino_pack_weights_f16x3': {'w_oihw': _n(R, 'O*I*9'), 'Uf16': _n(W_, '(tile+2)**2*O*I*4'), 'Ub16': _n(W_, '(tile+2)**2*O*I*4')},
    'pp_wino_pack_weights_f16x3_batch': {'items': (R, 'items', _WINO_ITEM)},
    # ---- 3x3 convolution
    'pp_conv3x3_fwd': _conv_fwd({'wf': _n(R, 'N*9*C')}),
    'pp_conv3x3_fwd_f16x3': _conv_fwd({'wf16': _n(R, 'N*9*C*4')}, {'in_amax': _n(R, '1')}),
    'pp_conv3x3_fwd_bn': _conv_fwd({'wf': _n(R, 'N*9*C*4')}, dict(_BN_FWD_TAIL, in_amax=_n(R, '1')), acc=False),
    'pp_conv3x3_fwd_bn_lazy': _conv_fwd({'wf': _n(R, 'N*9*C*4')}, dict(_BN_FWD_TAIL, in_amax=_n(R, '1'), lazy_in=(R, 'lazy', 'C')), acc=False),
    'pp_conv3x3_wino_fwd': _conv_fwd({'Uf': _n(R, 'planes(H, W, dil)*N*C')}, _WINO_WS),
    'pp_conv3x3_wino_fwd_f16x3': _conv_fwd({'Uf16': _n(R, 'planes(H, W, dil)*N*C*4')}, _WINO_WS),
    'pp_conv3x3_wino_fwd_bn': _conv_fwd({'U': _n(R, 'planes(H, W, dil)*N*C*4')}, dict(_BN_FWD_TAIL, **_WINO_WS), acc=False),
    'pp_conv3x3_bwd_data': dict(_BWD_DATA, wb=_n(R, 'I*9*O')),
    'pp_conv3x3_bwd_data_f16x3': dict(_BWD_DATA, wb16=_n(R, 'I*9*O*4'), dz_amax=_n(R, '1')),
    'pp_conv3x3_wino_bwd_data': dict(_BWD_DATA, Ub=_n(R, 'planes(H, W, dil)*I*O'), workspace=WS),
    'pp_conv3x3_wino_bwd_data_f16x3': dict(_BWD_DATA, Ub16=_n(R, 'planes(H, W, dil)*I*O*4'), workspace=WS, dz_amax=_n(R, '1')),
    'pp_conv3x3_bwd_weight': _WG,
    'pp_conv3x3_bwd_weight_f16x3': dict(_WG, dz_amax=_n(R, '1')),
    'pp_conv3x3_bwd_weight_f16x3_lazy': dict(_WG, dz_amax=_n(R, '1'), lazy_x=(R, 'lazy', 'Cpad')),
    'pp_conv3x3_wino_bwd_weight': _WINO_WG,
    'pp_conv3x3_wino_bwd_weight_f16x3': dict(_WINO_WG, dz_amax=_n(R, '1')),
    # ---- BatchNorm / GroupNorm
    'pp_bn_train_stats': dict({k: v for k, v in _FINALIZE.items() if k != 'sums'}, z=_act(R, 'P_per_group*groups', 'C', 'ld'),
                              workspace=WS),
    'pp_bn_eval_coeffs': dict({k: _n(R, 'C') for k in ('gamma', 'beta', 'running_mean', 'running_var')},
                              **{k: _n(W_, _GC) for k in ('save_mean', 'save_invstd', 'scale', 'shift')}),
    'pp_bn_eval_coeffs_batch': {'items': (R, 'items', _COEF_ITEM)},
    'pp_bn_lrelu_fwd': {'z': _act(R, 'P_per_group*groups', 'C', 'ld_z'), 'scale': _n(R, _GC), 'shift': _n(R, _GC),
                        'y': _act(W_, 'P_per_group*groups', 'C', 'ld_y')},
    'pp_bn_lrelu_fwd_pool': {'z': _act(R, 'B*H*W', 'C', 'ld_z'), 'scale': _n(R, _GC), 'shift': _n(R, _GC),
                             'y': _act(W_, 'B*H*W', 'C', 'ld_y'), 'pooled': _act(W_, 'B*(H//2)*(W//2)', 'C', 'ld_pooled')},
    'pp_bn_stats_sums': {'z': _act(R, 'P_per_group*groups', 'C', 'ld'), 'sums': _n(W_, 'groups*2*C'), 'workspace': WS},
    'pp_bn_train_finalize': _FINALIZE,
    'pp_bn_train_finalize_lazy': dict(_FINALIZE, lazy_coef=(W_, 'coefrows', 'C', 'lazy_ld', 'groups')),
    'pp_lazy_materialize': {'src': _act(R, 'B*HW', 'C', 'ld_src'), 'lazy': (R, 'lazy', 'C'), 'dst': _act(W_, 'B*HW', 'C', 'ld_dst')},
    'pp_bn_lrelu_bwd': _bn_bwd('P_per_group*groups', amax=False),
    'pp_bn_lrelu_bwd_amax': _bn_bwd('P_per_group*groups'),
    'pp_bn_lrelu_bwd_pool': _bn_bwd('B*H*W', pool='B*(H//2)*(W//2)'),
    'pp_bn_lrelu_bwd_eval': _bn_bwd('P_total', rows=_EVAL_ROWS, z='y'),
    'pp_bn_lrelu_bwd_eval_pool': _bn_bwd('B*H*W', rows=_EVAL_ROWS, z='y', pool='B*(H//2)*(W//2)'),
    'pp_bn_lrelu_bwd_sums': {'dy': _act(R, 'P_per_group*groups', 'C', 'ld_dy'), 'z': _act(R, 'P_per_group*groups', 'C', 'ld_z'),
                             **_BN_ROWS, 'sums': _n(W_, 'groups*2*C'), 'workspace': WS},
    'pp_bn_lrelu_bwd_apply': _bn_bwd('P_per_group*groups', extra={'local_sums': _n(R, 'groups*2*C'), 'global_sums': _n(R, 'groups*2*C')}),
    'pp_bn_lrelu_bwd_wgrad_c1': _bn_bwd('P_per_group*groups', dz=False, amax=False,
                                        extra=dict(_C1, x=_act(R, 'P_per_group*groups', '1', 'ld_x'))),
    'pp_bn_lrelu_bwd_eval_wgrad_c1': _bn_bwd('P_total', rows=_EVAL_ROWS, z='y', dz=False, amax=False,
                                             extra=dict(_C1, x=_act(R, 'P_total', '1', 'ld_x'))),
    'pp_gn_stats': {'z': _act(R, 'N*HW', 'C', 'ld'), 'gamma': _n(R, 'C'), 'beta': _n(R, 'C'),
                    **{k: _n(W_, 'N*C') for k in ('save_mean', 'save_invstd', 'save_xbar', 'scale', 'shift')}, 'workspace': WS},
    'pp_gn_lrelu_bwd': _bn_bwd('N*HW', rows=_GN_ROWS),
    'pp_gn_lrelu_bwd_pool': _bn_bwd('N*H*W', rows=_GN_ROWS, pool='N*(H//2)*(W//2)'),
    # ---- pooling / resampling / copies
    'pp_maxpool2_fwd': {'x': _act(R, 'N*H*W', 'C', 'ld_x'), 'y': _act(W_, 'N*(H//2)*(W//2)', 'C', 'ld_y')},
    'pp_maxpool2_bwd': {'x': _act(R, 'N*H*W', 'C', 'ld_x'), 'dy': _act(R, 'N*(H//2)*(W//2)', 'C', 'ld_dy'),
                        'dx': _act('w+accumulate', 'N*H*W', 'C', 'ld_dx')},
    'pp_bilinear_fwd': {'x': _act(R, 'N*Hi*Wi', 'C', 'ld_x'), 'y': _act(W_, 'N*Ho*Wo', 'C', 'ld_y')},
    'pp_bilinear_bwd': {'dy': _act(R, 'N*Ho*Wo', 'C', 'ld_dy'), 'dx': _act('w+accumulate', 'N*Hi*Wi', 'C', 'ld_dx')},
    'pp_copy_slab': {'x': _act(R, 'P', 'C', 'ld_x'), 'y': _act('w+accumulate', 'P', 'C', 'ld_y')},
    'pp_channel_scale': {'x': _act(R, 'N*HW', 'C', 'ld_x'), 'y': _act('w+accumulate', 'N*HW', 'C', 'ld_y'), 'scale': _n(R, 'N*C')},
    'pp_stride2_gather': {'full': _act(R, 'N*4*Ho*Wo', 'C', 'ld_full'), 'out': _act(W_, 'N*Ho*Wo', 'C', 'ld_out')},
    'pp_stride2_scatter': {'dz': _act(R, 'N*Ho*Wo', 'C', 'ld_dz'), 'full': _act(W_, 'N*4*Ho*Wo', 'C', 'ld_full')},
    'pp_convtranspose_fwd': {'x': _act(R, 'N*H*W', 'Cin', 'ld_x'), 'w': _n(R, 'Cin*Cout*k*k'),
                             'out': _act(W_, 'N*k*H*k*W', 'Cout', 'ld_out')},
    'pp_convtranspose_bwd_data': {'dout': _act(R, 'N*k*H*k*W', 'Cout', 'ld_dout'), 'w': _n(R, 'Cin*Cout*k*k'),
                                  'dx': _act('w+accumulate', 'N*H*W', 'Cin', 'ld_dx')},
    'pp_convtranspose_bwd_weight': {'dout': _act(R, 'N*k*H*k*W', 'Cout', 'ld_dout'), 'x': _act(R, 'N*H*W', 'Cin', 'ld_x'),
                                    'dw': _n('w+accumulate', 'Cin*Cout*k*k'), 'workspace': WS},
    # ---- 1x1 heads
    'pp_conv1x1_nhwc_to_nchw_fwd': {'x': _act(R, 'N*HW', 'C', 'ld_x'), 'w': _n(R, 'K*C'), 'bias': _n(R, 'K'), 'logits': _n(W_, 'N*K*HW')},
    'pp_conv1x1_nhwc_to_nchw_fwd_lazy': {'x': _act(R, 'N*HW', 'C', 'ld_x'), 'w': _n(R, 'K*C'), 'bias': _n(R, 'K'),
                                         'logits': _n(W_, 'N*K*HW'), 'lazy_x': (R, 'lazy', 'C')},
    'pp_conv1x1_nchw_to_nhwc_bwd': {'dlogits': _n(R, 'N*K*HW'), 'x': _act(R, 'N*HW', 'C', 'ld_x'), 'w': _n(R, 'K*C'),
                                    'dx': _act('w+accumulate_dx', 'N*HW', 'C', 'ld_dx'), 'dw': _n('w+accumulate_param_grads', 'K*C'),
                                    'dbias': _n('w+accumulate_param_grads', 'K'), 'workspace': WS},
    # ---- losses
    'pp_argmax_channels': {'x': _n(R, 'N*C*HW'), 'out': _n(W_, 'N*HW')},
    'pp_seg_losses_fwd': {'logits_w': _n(R, 'N*K*HW'), 'logits_s': _n(R, 'N*K*HW'), 'target': _n(R, 'N*HW'), 'valid_mask': _n(R, 'N*HW'),
                          'sums': _n(W_, '6'), 'workspace': WS},
    # pCE reads sums[0:2], the masked / unmasked ratio sums[2:4], the consistency ratio sums[4:6]: the hull of the pairs asked for
    'pp_losses_finalize': {'sums': _n(R, '6 if loss_cr is not None else (4 if loss_ent is not None else 2)'),
                           'loss_pce': _n(W_, '1'), 'loss_ent': _n(W_, '1'), 'loss_cr': _n(W_, '1')},
    'pp_seg_losses_bwd': {'logits_w': _n(R, 'N*K*HW'), 'logits_s': _n(R, 'N*K*HW'), 'target': _n(R, 'N*HW'), 'valid_mask': _n(R, 'N*HW'),
                          'sums': _n(R, '6'), 'g_pce': _n(R, '1'), 'g_ent': _n(R, '1'), 'g_cr': _n(R, '1'),
                          'dlogits_w': _n(W_, 'N*K*HW'), 'dlogits_s': _n(W_, 'N*K*HW')},
    'pp_aux_pce_fwd': {'lo': _n(R, 'N*K*h*w'), 'target': _n(R, 'N*H*W'), 'logits_up': _n(W_, _NKHW), 'sums': _n(W_, '2'), 'workspace': WS},
    'pp_aux_pce_bwd': {'logits_up': _n(R, _NKHW), 'target': _n(R, 'N*H*W'), 'g_aux': _n(R, '1'), 'sums': _n(R, '2'), 'dlo': _n(W_, 'N*K*h*w')},
    'pp_memory_update': {'feat0': _act(R, 'h*w', 'hid', 'ld'), 'scribble0': _n(R, '(K+1)*H*W'), 'bank': _n(RW, 'K*hid'), 'workspace': WS},
    'pp_memory_ce_fwd': {'bank': _n(R, 'K*hid'), 'wfc': _n(R, 'K*hid'), 'loss': _n(W_, '1')},
    'pp_memory_ce_bwd': {'bank': _n(R, 'K*hid'), 'wfc': _n(R, 'K*hid'), 'g': _n(R, '1'), 'dwfc': _n('w+accumulate', 'K*hid')},
    'pp_weighted_sum_fwd': {'terms': (R, 'ptrs', '1'), 'weights': ('r', 'host'), 'out': _n(W_, '1')},
    'pp_weighted_sum_bwd': {'g': _n(R, '1'), 'weights': ('r', 'host'), 'gout': _n(W_, 'n')},
    'pp_crf_loss_fwd': _CRF_FWD,
    'pp_crf_loss_bwd': {'unit_grad': _n(R, 'n'), 'sums': _n(R, '2'), 'g_up': _n(R, '1'), 'dlogits': _n(RW, 'n')},
    'pp_nc_loss_fwd': dict(_CRF_FWD, assoc_vol=_n(W_, 'N*K*2')),
    'pp_nc_loss_bwd': {'unit_grad': _n(R, 'n'), 'sums': _n(R, '2'), 'g_up': _n(R, '1'), 'dlogits': _n(RW, 'n')},
    # ---- optimiser
    'pp_scale': {'p': _n(RW, 'n')},
    'pp_scale_guard': {'p': _n(RW, 'n'), 'bad': _n(RW, '2')},
    'pp_fill': {'p': _n(W_, 'n')},
    'pp_grad_sumsq': {'g': _n(R, 'n'), 'partial': _n(W_, 'sumsq_rows(n)')},
    'pp_grad_clip_finalize': {'partial': _n(R, 'rows'), 'skip': _n(R, '2'), 'out2': _n(W_, '2'), 'stats': _n(RW, '4')},
    'pp_adam_step_dev': {k: v for k, v in _ADAM.items() if k not in ('clip_dev', 'ema')},
    'pp_adam_step_clip': {k: v for k, v in _ADAM.items() if k != 'ema'},
    'pp_adam_step_ema': _ADAM,
    'pp_sgd_momentum_step_dev': {k: v for k, v in _SGD.items() if k not in ('clip_dev', 'ema')},
    'pp_sgd_momentum_step_clip': {k: v for k, v in _SGD.items() if k != 'ema'},
    'pp_sgd_momentum_step_ema': _SGD,
}
TABLE['pp_conv1x1_nchw_to_nhwc_bwd_lazy'] = dict(TABLE['pp_conv1x1_nchw_to_nhwc_bwd'], lazy_x=(R, 'lazy', 'C'))


def base_entry(entry):
    """The row an entry point reads its extents from: the _h16 / _bf16 twins share the fp32 entry's row."""
    for suf in ('_h16', '_bf16'):
        if entry.endswith(suf) and entry[:-len(suf)] in TABLE:
            return entry[:-len(suf)]
    return entry


class MissingRow(KeyError):
    pass


Access = namedtuple('Access', 'param mode base rows row_bytes stride')


def _hull(a):
    return a.base, a.base + (a.rows - 1) * a.stride + a.row_bytes


def accesses(entry, vals):
    """The device accesses of one recorded launch: [Access].  vals: the argument values without the stream."""
    row = TABLE.get(base_entry(entry))
    if row is None:
        raise MissingRow(f'{entry}: a recorded launch without a row in tests/_stream_hazards.TABLE')
    params = header_params()[entry][:-1]
    env = dict(_QUERIES)
    for p, v in zip(params, vals):
        env[p.name] = v
    out = []
    for p, v in zip(params, vals):
        if not p.pointer:
            continue
        if p.name not in row:
            raise MissingRow(f'{entry}: pointer parameter {p.name} is not classified in tests/_stream_hazards.TABLE')
        if v is None:
            continue                                   # a nullable pointer that is null is no access
        spec = row[p.name]
        mode, kind = spec[0], spec[1]
        if mode.startswith('w+'):
            mode = RW if env[mode[2:]] else W_
        ev = lambda e, **more: int(eval(e, {}, dict(env, es=p.size, **more)))       # noqa: E731
        if kind == 'host':
            continue
        if kind == 'nhwc':
            P, C, ld = (ev(e) for e in spec[2:5])
            if P > 0:
                out.append(Access(p.name, mode, v, P, C * p.size, ld * p.size))
        elif kind in ('n', 'bytes'):
            n = ev(spec[2]) * (p.size if kind == 'n' else 1)
            if n > 0:
                out.append(Access(p.name, mode, v, 1, n, n))
        elif kind == 'lazy':
            _, coef, ld, groups = v
            if coef:
                out.append(Access(p.name + '.coef', mode, coef, groups * 3, 4 * ev(spec[2]), 4 * ld))
        elif kind == 'coefrows':
            C, ld, groups = (ev(e) for e in spec[2:5])
            out.append(Access(p.name, mode, v, groups * 3, 4 * C, 4 * ld))
        elif kind == 'items':
            for i, item in enumerate(v[1]):
                for field, (m, count) in spec[2].items():
                    if item.get(field):
                        n = 4 * int(eval(count, {}, dict(item)))
                        out.append(Access(f'{p.name}[{i}].{field}', m, item[field], 1, n, n))
        elif kind == 'ptrs':
            for i, ptr in enumerate(v[1]):
                if ptr:
                    n = 4 * ev(spec[2])
                    out.append(Access(f'{p.name}[{i}]', mode, ptr, 1, n, n))
        else:
            raise ValueError(kind)
    return out


def overlap(a, b):
    """Two boxes with the same stride and disjoint column ranges do not overlap; any other two boxes whose hulls intersect do."""
    a0, a1 = _hull(a)
    b0, b1 = _hull(b)
    if a1 <= b0 or b1 <= a0:
        return False
    if a.stride == b.stride and a.rows > 1 and b.rows > 1:
        S = a.stride
        d = (b.base - a.base) % S                      # modulo S the bytes of a are columns [0, wa), those of b [d, d + wb)
        if d >= a.row_bytes and d + b.row_bytes <= S:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------ checker
Hazard = namedtuple('Hazard', 'first second range')       # first / second: (log position, entry, parameter, mode, stream, (lo, hi))


def _join(a, b):
    for k, v in b.items():
        if a.get(k, 0) < v:
            a[k] = v


def clocks(log):
    """[(log position, entry, vals, stream, own tick, vector clock)] for the launches of the log."""
    clock = {}                   # stream -> {stream: ticks}
    floor = {}                   # what every stream, also one not seen yet, is ordered behind (host barriers)
    events = {}                  # event -> clock at its latest record
    out = []

    def of(s):
        if s not in clock:
            clock[s] = dict(floor)
        return clock[s]

    def barrier(c):
        _join(floor, c)
        for s in clock:
            _join(clock[s], c)

    for pos, item in enumerate(log):
        kind = item[0]
        if kind == 'L':
            s = item[3]
            c = of(s)
            c[s] = c.get(s, 0) + 1
            out.append((pos, item[1], item[2], s, c[s], dict(c)))
        elif kind == 'R':
            events[item[1]] = dict(of(item[2]))
        elif kind == 'W':
            if item[1] in events:                      # a wait on an event that was never recorded orders nothing
                _join(of(item[2]), events[item[1]])
        elif kind == 'WS':
            _join(of(item[1]), of(item[2]))
        elif kind == 'B':
            every = {}
            for c in clock.values():
                _join(every, c)
            barrier(every)
        elif kind == 'SS':
            barrier(dict(of(item[1])))
        elif kind == 'ES':
            if item[1] in events:
                barrier(dict(events[item[1]]))
        else:
            raise ValueError(f'unknown log entry {item!r}')
    return out


def check(log, limit=50):
    """Returns (hazards, total): one Hazard per unordered conflicting PAIR OF LAUNCHES (its first conflicting pair of accesses),
    at most `limit` of them, and the number of all unordered conflicting pairs of accesses."""
    acc = []                     # (hull lo, hull hi, launch index, Access)
    launches = clocks(log)
    for li, (pos, entry, vals, s, tick, vc) in enumerate(launches):
        for a in accesses(entry, vals):
            lo, hi = _hull(a)
            acc.append((lo, hi, li, a))
    acc.sort(key=lambda t: (t[0], t[2]))
    found, total = [], 0
    seen = set()
    active = []
    for lo, hi, li, a in acc:
        active = [t for t in active if t[1] > lo]
        sa, ta, vca = launches[li][3:6]
        for blo, bhi, lj, b in active:
            sb = launches[lj][3]
            if sb == sa or (a.mode == R and b.mode == R):
                continue
            tb, vcb = launches[lj][4], launches[lj][5]
            # the earlier launch in host order can only come first: is its tick inside the later one's clock?
            (i1, t1, s1), (i2, vc2) = ((li, ta, sa), (lj, vcb)) if li < lj else ((lj, tb, sb), (li, vca))
            if vc2.get(s1, 0) >= t1:
                continue
            if not overlap(a, b):
                continue
            total += 1
            key = (min(li, lj), max(li, lj))
            if key in seen or len(found) >= limit:
                continue
            seen.add(key)
            x, y = ((li, a), (lj, b)) if li < lj else ((lj, b), (li, a))
            found.append(Hazard(_side(launches, *x), _side(launches, *y), (max(lo, blo), min(hi, bhi))))
        active.append((lo, hi, li, a))
    return found, total


def _side(launches, li, a):
    pos, entry, _, s, _, _ = launches[li]
    return (pos, entry, a.param, a.mode, s, _hull(a))


def describe(h):
    def one(x):
        pos, entry, param, mode, s, (lo, hi) = x
        return f'#{pos} {entry}({param}: {mode} [{lo:#x}, {hi:#x})) on stream {s:#x}'
    return f'{one(h.first)}  <->  {one(h.second)}  overlap [{h.range[0]:#x}, {h.range[1]:#x})'


def report(hazards, total):
    return f'{total} unordered conflicting access pair(s); the first {len(hazards)} launch pairs:\n' + '\n'.join(describe(h) for h in hazards)


# ------------------------------------------------------------------------------------------------------------ log surgery
JOIN_SITE = '_join_side_stream'
EVENT_KINDS = ('dz_ready', 'wg_done', 'aux_fork', 'aux_join', 'bucket_ev', 'join')


def wait_kind(item, event_names):
    """Which of the engine's six kinds of wait a ('W', ...) entry is, or None (somebody else's event).  The waits of
    StepEngine._join_side_stream are their own kind: they are on the wg_done events too, but protect the optimizer's reads."""
    if item[0] != 'W':
        return None
    name = event_names.get(item[1])
    if name == 'wg_done' and item[3] == JOIN_SITE:
        return 'join'
    return name


def without_waits(log, event_names, kind):
    """The log with every wait of one kind deleted (a planted mistake, made on the log)."""
    return [it for it in log if wait_kind(it, event_names) != kind]
