"""ctypes binding of libpacingpseudo_unc.so (the C ABI declared in include/pacingpseudo_unc.h): the uncertainty mask of the
mean-teacher consistency term (``--cr_uncertainty``) -- noisy teacher inputs from a counter-based generator whose (seed, step) live
on the device, the mean soft-max over the passes, its entropy, the mask and three statistics.

It is loaded on first use, never at import.  As with ``_lib``, ``_prep`` and ``_rwp`` there is NO fallback: a missing or stale
library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make unc``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('punc_version', 'punc_last_error', 'punc_workspace_bytes')      # a value, not a status code


class _UncLib:
    def __init__(self, path=UNC_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the uncertainty mask has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make unc`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'punc_version'):
                dll.punc_version.restype = i32
                have = dll.punc_version()
            if have < MIN_UNC_VERSION:
                raise HipLibraryError(f'{path} reports punc_version() = {have}; this host side needs >= {MIN_UNC_VERSION} '
                                      '(an older build of the library: rebuild with `make unc`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (punc_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make unc`')
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
                msg = self.load().punc_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


unc = _UncLib()
