"""ctypes binding of libpacingpseudo_morph.so (the C ABI declared in include/pacingpseudo_morph.h): the size threshold per class and
the hole filling that work on the component labels of a hard class map (``inference.py --min_component_size`` / ``--fill_holes``,
``utils.morphology``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make morph``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
MORPH_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_morph.so')

vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
hostp = C.POINTER(C.c_int32)     # min_size: K thresholds in HOST memory

# name -> (restype, argtypes); mirrors include/pacingpseudo_morph.h one to one
_PROTOS = {
    'pmor_version': (i32, []),
    'pmor_last_error': (C.c_char_p, []),
    'pmor_workspace': (sz, [i32, i32, i32, i32, i32, i32]),
    'pmor_remove_small': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, hostp, vp, vp, vp, sz, vp]),
    'pmor_fill_holes': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_MORPH_VERSION = 100     # include/pacingpseudo_morph.h (pp_morph.hip: PMOR_VERSION)


class _MorphLib(CLibrary):
    prefix, target, no_fallback = 'pmor', 'morph', 'the size threshold and hole filling have no CPU fallback'
    int_values = ('pmor_version',)

    def _spec(self):
        return self._path or MORPH_LIB_PATH, _PROTOS, MIN_MORPH_VERSION


morph = _MorphLib()
