"""ctypes binding of libpacingpseudo_prep.so (the C ABI declared in include/pacingpseudo_prep.h): the companion library for work
done once on the training data before the first step (the random-walker expansion of scribbles).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make prep``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
PREP_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_prep.so')

vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
ip = C.POINTER(C.c_int)        # `sizes`: a HOST array of (h, w) pairs, or None

# name -> (restype, argtypes); mirrors include/pacingpseudo_prep.h one to one
_PROTOS = {
    'pprep_version': (i32, []),
    'pprep_last_error': (C.c_char_p, []),
    'pprep_rw_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'pprep_rw_solve': (i32, [vp, vp, ip, i32, i32, i32, i32, f32, f32, f32, i32, vp, vp, vp, vp]),
    'pprep_rw_labels': (i32, [vp, vp, ip, i32, i32, i32, i32, f32, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_PREP_VERSION = 100     # include/pacingpseudo_prep.h (pp_random_walker.hip: PPREP_VERSION)


class _PrepLib(CLibrary):
    prefix, target, no_fallback = 'pprep', 'prep', 'the random-walker expansion has no CPU fallback'
    int_values = ('pprep_version',)

    def _spec(self):
        return self._path or PREP_LIB_PATH, _PROTOS, MIN_PREP_VERSION


prep = _PrepLib()
