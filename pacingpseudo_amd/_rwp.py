"""ctypes binding of libpacingpseudo_rwp.so (the C ABI declared in include/pacingpseudo_rwp.h): the random walker with priors that
the training driver re-runs every few epochs to refresh the scribble pseudo-labels (``--rw_refresh``).

It is loaded on first use, never at import.  As with ``_lib`` and ``_prep`` there is NO fallback: a missing or stale library raises.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make rwp``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('prwp_version', 'prwp_last_error', 'prwp_workspace_bytes')      # a value, not a status code


class _RwpLib:
    def __init__(self, path=RWP_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the random walker with priors has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make rwp`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'prwp_version'):
                dll.prwp_version.restype = i32
                have = dll.prwp_version()
            if have < MIN_RWP_VERSION:
                raise HipLibraryError(f'{path} reports prwp_version() = {have}; this host side needs >= {MIN_RWP_VERSION} '
                                      '(an older build of the library: rebuild with `make rwp`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (prwp_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make rwp`')
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
                msg = self.load().prwp_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


rwp = _RwpLib()
