"""ctypes binding of libpacingpseudo_unc.so (the C ABI declared in include/pacingpseudo_unc.h): the uncertainty mask of the
mean-teacher consistency term (``--cr_uncertainty``) -- noisy teacher inputs from a counter-based generator whose (seed, step) live
on the device, the mean soft-max over the passes, its entropy, the mask and three statistics.

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make unc``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
UNC_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_unc.so')

vp, i32, i64, f32, sz = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/pacingpseudo_unc.h one to one
_PROTOS = {
    'punc_version': (i32, []),
    'punc_last_error': (C.c_char_p, []),
    'punc_workspace_bytes': (sz, [i32, i32, i32]),
    'punc_noise_add': (i32, [vp, i64, f32, f32, vp, i32, vp, vp]),
    'punc_accumulate': (i32, [vp, i32, i32, i32, i32, i32, vp, f32, vp, vp, vp, vp, vp, sz, vp]),
    'punc_advance': (i32, [vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_UNC_VERSION = 100      # include/pacingpseudo_unc.h (pp_uncertainty.hip: PUNC_VERSION)


class _UncLib(CLibrary):
    prefix, target, no_fallback = 'punc', 'unc', 'the uncertainty mask has no CPU fallback'
    int_values = ('punc_version',)

    def _spec(self):
        return self._path or UNC_LIB_PATH, _PROTOS, MIN_UNC_VERSION


unc = _UncLib()
