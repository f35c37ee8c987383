"""ctypes binding of libpacingpseudo_prep.so (the C ABI declared in include/pacingpseudo_prep.h): the companion library for work
done once on the training data before the first step (the random-walker expansion of scribbles).

It is loaded on first use, never at import.  As with ``_lib`` there is NO fallback: a missing or stale library raises.  Build it
with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make prep``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('pprep_version', 'pprep_last_error', 'pprep_rw_workspace_bytes')      # a value, not a status code


class _PrepLib:
    def __init__(self, path=PREP_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the random-walker expansion has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make prep`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'pprep_version'):
                dll.pprep_version.restype = i32
                have = dll.pprep_version()
            if have < MIN_PREP_VERSION:
                raise HipLibraryError(f'{path} reports pprep_version() = {have}; this host side needs >= {MIN_PREP_VERSION} '
                                      '(an older build of the library: rebuild with `make prep`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (pprep_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make prep`')
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
                msg = self.load().pprep_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


prep = _PrepLib()
