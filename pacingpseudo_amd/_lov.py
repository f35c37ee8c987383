"""ctypes binding of libpacingpseudo_lov.so (the C ABI declared in include/pacingpseudo_lov.h): a segmented, stable, descending radix
sort on the device and the Lovasz-softmax loss built on it (``upper_bound_chaos.py --do_loss_lovasz``, ``utils.sort_descending``,
``losses.lovasz_softmax_loss``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make lov``).  ``TILE`` (a module attribute
that loads the library) is the largest number of keys one block handles per pass."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LOV_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_lov.so')

vp, i32, i64, sz = C.c_void_p, C.c_int, C.c_longlong, C.c_size_t

# name -> (restype, argtypes); mirrors include/pacingpseudo_lov.h one to one
_PROTOS = {
    'plov_version': (i32, []),
    'plov_last_error': (C.c_char_p, []),
    'plov_tile': (i32, []),
    'plov_sort_workspace': (sz, [i32, i32]),
    'plov_sort_descending': (i32, [vp, i32, i32, vp, vp, vp, sz, vp]),
    'plov_loss_workspace': (sz, [i32, i32, i32, i32, i32]),
    'plov_loss_fwd': (i32, [vp, vp, i32, i32, i32, i32, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'plov_loss_bwd': (i32, [vp, vp, i32, i32, i32, i32, i32, i64, i32, vp, vp, vp, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_LOV_VERSION = 100      # include/pacingpseudo_lov.h (pp_lovasz.hip: PLOV_VERSION)


class _LovLib(CLibrary):
    prefix, target, no_fallback = 'plov', 'lov', 'the device sort and the Lovasz-softmax loss have no CPU fallback'
    int_values = ('plov_version', 'plov_tile')

    def _spec(self):
        return self._path or LOV_LIB_PATH, _PROTOS, MIN_LOV_VERSION


lov = _LovLib()


def __getattr__(name):
    if name == 'TILE':
        return int(lov.plov_tile())
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
