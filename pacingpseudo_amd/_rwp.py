"""ctypes binding of libpacingpseudo_rwp.so (the C ABI declared in include/pacingpseudo_rwp.h): the random walker with priors that
the training driver re-runs every few epochs to refresh the scribble pseudo-labels (``--rw_refresh``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make rwp``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
RWP_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_rwp.so')

vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
ip = C.POINTER(C.c_int)        # `sizes`: a HOST array of (h, w) pairs, or None

# name -> (restype, argtypes); mirrors include/pacingpseudo_rwp.h one to one
_PROTOS = {
    'prwp_version': (i32, []),
    'prwp_last_error': (C.c_char_p, []),
    'prwp_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'prwp_solve': (i32, [vp, vp, vp, ip, i32, i32, i32, i32, f32, f32, f32, f32, i32, vp, vp, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_RWP_VERSION = 100      # include/pacingpseudo_rwp.h (pp_rw_prior.hip: PRWP_VERSION)


class _RwpLib(CLibrary):
    prefix, target, no_fallback = 'prwp', 'rwp', 'the random walker with priors has no CPU fallback'
    int_values = ('prwp_version',)

    def _spec(self):
        return self._path or RWP_LIB_PATH, _PROTOS, MIN_RWP_VERSION


rwp = _RwpLib()
