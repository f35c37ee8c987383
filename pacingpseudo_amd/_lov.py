"""ctypes binding of libpacingpseudo_lov.so (the C ABI declared in include/pacingpseudo_lov.h): a segmented, stable, descending radix
sort on the device and the Lovasz-softmax loss built on it (``upper_bound_chaos.py --do_loss_lovasz``, ``utils.sort_descending``,
``losses.lovasz_softmax_loss``).

It is loaded on first use, never at import.  As with ``_lib``, ``_dist`` and ``_opt`` there is NO fallback: a missing or stale
library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make lov``).  ``TILE`` (a module
attribute that loads the library) is the largest number of keys one block handles per pass."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('plov_version', 'plov_last_error', 'plov_tile', 'plov_sort_workspace', 'plov_loss_workspace')      # a value, not a status code


class _LovLib:
    def __init__(self, path=LOV_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the device sort and the Lovasz-softmax loss have no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make lov`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'plov_version'):
                dll.plov_version.restype = i32
                have = dll.plov_version()
            if have < MIN_LOV_VERSION:
                raise HipLibraryError(f'{path} reports plov_version() = {have}; this host side needs >= {MIN_LOV_VERSION} '
                                      '(an older build of the library: rebuild with `make lov`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (plov_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make lov`')
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
                msg = self.load().plov_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


lov = _LovLib()


def __getattr__(name):
    if name == 'TILE':
        return int(lov.plov_tile())
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
