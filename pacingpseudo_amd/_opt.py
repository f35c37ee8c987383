"""ctypes binding of libpacingpseudo_opt.so (the C ABI declared in include/pacingpseudo_opt.h): the fused AdamW update with a
per-element exemption from the weight decay (``pacingpseudo_amd.optim.FusedAdamW``; ``--optimizer adamw [--wd_exempt_1d]``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make opt``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

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


class _OptLib(CLibrary):
    prefix, target, no_fallback = 'popt', 'opt', 'the fused AdamW update has no CPU fallback'
    int_values = ('popt_version',)

    def _spec(self):
        return self._path or OPT_LIB_PATH, _PROTOS, MIN_OPT_VERSION


opt = _OptLib()
