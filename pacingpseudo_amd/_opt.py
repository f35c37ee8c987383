"""ctypes binding of libpacingpseudo_opt.so (the C ABI declared in include/pacingpseudo_opt.h): the fused AdamW update with a
per-element exemption from the weight decay (``pacingpseudo_amd.optim.FusedAdamW``; ``--optimizer adamw [--wd_exempt_1d]``).

It is loaded on first use, never at import.  As with ``_lib``, ``_prep``, ``_rwp``, ``_unc``, ``_dist``, ``_geo``, ``_vol`` and
``_morph`` there is NO fallback: a missing or stale library raises.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` (or ``make opt``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

_HERE = os.path.dirname(os.path.abspath(__file__))
OPT_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_opt.so')

vp, i32, i64, f32, f64 = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double

# p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step_dev, skip, count_skip, exempt
_COMMON = [vp, vp, vp, vp, i64, f32, vp, f32, f32, f32, f32, vp, vp, i32, vp]

# name -> (restype, argtypes); mirrors include/pacingpseudo_opt.h one to one
_PROTOS = {
    'popt_version': (i32, []),
    'popt_last_error': (C.c_char_p, []),
    'popt_trip_elements': (i64, []),
    'popt_adamw_step': (i32, _COMMON + [vp]),
    'popt_adamw_step_clip': (i32, _COMMON + [vp, vp]),
    'popt_adamw_step_ema': (i32, _COMMON + [vp, f64, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_OPT_VERSION = 100       # include/pacingpseudo_opt.h (pp_adamw.hip: POPT_VERSION)
_NO_STATUS = ('popt_version', 'popt_last_error', 'popt_trip_elements')      # a value, not a status code


class _OptLib:
    def __init__(self, path=OPT_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the fused AdamW update has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make opt`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'popt_version'):
                dll.popt_version.restype = i32
                have = dll.popt_version()
            if have < MIN_OPT_VERSION:
                raise HipLibraryError(f'{path} reports popt_version() = {have}; this host side needs >= {MIN_OPT_VERSION} '
                                      '(an older build of the library: rebuild with `make opt`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (popt_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make opt`')
            for name, (res, args) in _PROTOS.items():
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = res, args
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        fn = getattr(self.load(), name)
        if name in _NO_STATUS:
            return fn

        def checked(*a):
            rc = fn(*a)
            if rc != 0:
                msg = self.load().popt_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


opt = _OptLib()
