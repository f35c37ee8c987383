"""One recording of every launch the engine makes in real full-width steps, shared by the two censuses.

engine.lib_for is patched so that each plan's entry-point table (plan.K) is a recording proxy, and so is the module-level `lib`
of engine.py, through which the launches go that belong to no storage kind (the batched weight packs, the eval-mode coefficient
rows of all layers in one launch, the unscaling of the gradient slab; recorded as 'fp32').  A launch is any entry of
_lib._PROTOS whose last argument is the stream (shape and workspace queries are not).  Every call is stored as (storage kind, entry point, launch shape) --
the launch shape is the argument list with pointers replaced by 'p' / None (null), buffer sizes by 'sz' and a lazy input by
('lazy', ld, groups) -- together with the configurations that made it.  The configurations run once per process (record() is
cached): tests/test_gpu_conv_census.py replays the convolution family of the record, tests/test_gpu_stream_census.py the rest.
record_batches() is a second recording of the same kind at other batch sizes and of the Control plan (batch_configs()).
"""
import ctypes
import functools
from collections import defaultdict

import torch

from oracle import pacing_oracle as O


def is_launch(name):
    from pacingpseudo_amd._lib import _PROTOS
    args = _PROTOS.get(name, (None, []))[1]
    return bool(args) and args[-1] is ctypes.c_void_p          # a launch takes a stream; shape queries do not


def _is_pointer(t):
    return t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _shape_of(name, args):
    """The launch with pointers (activations, int64 targets, double sums, pointer arrays: whatever the type) replaced by 'p' / None
    (null), buffer sizes by 'sz', a lazy input by ('lazy', ld, groups)."""
    from pacingpseudo_amd._lib import _PROTOS, lazy_p
    out = []
    for t, a in zip(_PROTOS[name][1], args):
        if t is lazy_p:
            out.append(None if a is None else ('lazy', a._obj.ld, a._obj.groups))
        elif _is_pointer(t):
            out.append(None if a is None else 'p')
        elif t is ctypes.c_size_t:
            out.append('sz')
        else:
            out.append(float(a) if isinstance(a, float) else int(a))
    return tuple(out)


class _Recorder:
    """Stands in for a plan's entry-point table: every attribute lookup reaches __getattr__ (nothing is cached here -- _Lib and
    _H16Lib cache their wrappers on themselves), launches are recorded and forwarded unchanged."""

    def __init__(self, inner, storage, sink):
        self._inner, self._storage, self._sink = inner, storage, sink

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not is_launch(name):
            return fn

        def call(*a):
            self._sink((self._storage, name, _shape_of(name, a)))
            return fn(*a)
        return call


def _configs():
    """label -> (storage, size, classes, output stride, variant)"""
    c = {'256/os8': ('fp32', 256, 5, 8, ''), '224/os8/4cls': ('fp32', 224, 4, 8, ''), '224/os8/2cls': ('fp32', 224, 2, 8, '')}
    for s in (256, 224):
        for os_ in (16, 32):
            c[f'{s}/os{os_}'] = ('fp32', s, 5 if s == 256 else 4, os_, '')
    c['256/strided'] = ('fp32', 256, 5, 8, 'strided')
    c['256/groupnorm'] = ('fp32', 256, 5, 8, 'gn')
    c['256/sync_bn'] = ('fp32', 256, 5, 8, 'sync_bn')
    for kind in ('fp16', 'bf16'):
        c[f'256/{kind}'] = (kind, 256, 5, 8, '')
        c[f'224/{kind}'] = (kind, 224, 4, 8, '')
    return c


def _run_config(label, name, storage, size, classes, os_, variant, batch=2):
    from tests.test_gpu_step import build_model
    # output stride 32 pools encoder stage 6 below stage 5: no auxiliary path there (as the golden case 'stride32')
    over = dict(do_aux_path=False, do_memory=False) if os_ == 32 else {}
    if variant == 'control':        # the Control plan of test_full_width_model_against_oracle: one backbone pass, no optional branch
        args = O.default_args(num_classes=classes, ignored_index=classes, output_stride=os_)
    else:
        args = O.full_flags(num_classes=classes, ignored_index=classes, output_stride=os_, **over)
    args.storage = storage
    if variant == 'strided':
        args.is_stride_conv = args.is_trans_conv = True
    torch.manual_seed(1)
    if variant == 'gn':
        from tests.test_gpu_groupnorm import build_gn_model
        model = build_gn_model(args)
    else:
        model = build_model(args)
    if variant == 'sync_bn':        # the split train-mode BatchNorm of --sync_bn on one rank (test_synchronised_batchnorm_backward)
        from tests._bucket_probe import NoopComm
        model.engine.comm = NoopComm()
        model.engine.sync_bn = True
    batch = {k: v.cuda() for k, v in O.synthetic_batch(batch, size, size, num_classes=classes, seed=7, keep=0.03).items() if k != 'label'}
    for bn_eval in (False, True):
        label[0] = f'{name}/{"eval" if bn_eval else "train"}-BN'
        model.train()
        if bn_eval:
            model.eval()
        model.zero_grad(set_to_none=True)
        out = model(batch, mode='train', step=0)
        loss = sum(out[k] * wt for k, wt in O.loss_weights(args, 0).items())
        loss.backward()
        torch.cuda.synchronize()
    del model, out, loss


def _run_inference():
    from pacingpseudo_amd.models import UNet
    args = O.full_flags(num_classes=4)
    torch.manual_seed(1)
    net = UNet(input_ch=1, init_ch=args.init_ch, max_ch=args.max_ch, num_classes=4, output_stride=8).cuda().eval()
    with torch.no_grad():
        net(torch.randn(1, 1, 256, 272, device='cuda'))
    torch.cuda.synchronize()
    del net


def _record(configs, inference):
    from pacingpseudo_amd import engine as E
    rec = defaultdict(set)
    real, real_lib = E.lib_for, E.lib
    label = ['']

    def patched(storage):
        s = {4: 'fp32', 2: 'fp16'}.get(storage, storage)
        return _Recorder(real(storage), s, lambda key: rec[key].add(label[0]))
    E.lib_for = patched
    E.lib = _Recorder(real_lib, 'fp32', lambda key: rec[key].add(label[0]))
    try:
        for name, cfg in configs.items():
            try:
                _run_config(label, name, *cfg)
            except Exception as e:
                raise RuntimeError(f'census configuration {label[0]} failed: {e}') from e
            torch.cuda.empty_cache()
        if inference:
            label[0] = '256x272/inference'
            _run_inference()
            torch.cuda.empty_cache()
    finally:
        E.lib_for, E.lib = real, real_lib
    return dict(rec)


@functools.lru_cache(maxsize=None)
def record():
    """{(storage, entry, launch shape): set of configuration labels}, over every configuration (cached for the process)."""
    return _record(_configs(), True)


BATCH_IMAGE_SIZE = 128        # the smallest square size of the batch recordings: every stage of the full-flags model exists (Dice phantoms)


def batch_configs():
    """label -> (storage, size, classes, output stride, variant, batch): batches that are no power of two, the reference's default
    batch of 12 and the Control plan, on small images.  The launch plans of the convolution family are functions of B * H * W and
    of tile counts; record() runs every configuration at batch 2."""
    s = BATCH_IMAGE_SIZE
    return {f'{s}/b3': ('fp32', s, 5, 8, '', 3), f'{s}/b12': ('fp32', s, 5, 8, '', 12),
            f'{s}/b3/fp16': ('fp16', s, 5, 8, '', 3), f'{s}/b3/bf16': ('bf16', s, 5, 8, '', 3),
            f'{s}/b8/control': ('fp32', s, 5, 8, 'control', 8)}


@functools.lru_cache(maxsize=None)
def record_batches():
    """As record(), over batch_configs(): {(storage, entry, launch shape): set of labels '<configuration>/<train|eval>-BN'}."""
    return _record(batch_configs(), False)
