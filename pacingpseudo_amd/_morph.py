"""ctypes binding of libpacingpseudo_morph.so (the C ABI declared in include/pacingpseudo_morph.h): the size threshold per class and
the hole filling that work on the component labels of a hard class map (``inference.py --min_component_size`` / ``--fill_holes``,
``utils.morphology``).

It is loaded on first use, never at import.  As with ``_lib``, ``_prep``, ``_rwp``, ``_unc``, ``_dist``, ``_geo`` and ``_vol`` there
is NO fallback: a missing or stale library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or
``make morph``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('pmor_version', 'pmor_last_error', 'pmor_workspace')      # a value, not a status code


class _MorphLib:
    def __init__(self, path=MORPH_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the size threshold and hole filling have no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make morph`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'pmor_version'):
                dll.pmor_version.restype = i32
                have = dll.pmor_version()
            if have < MIN_MORPH_VERSION:
                raise HipLibraryError(f'{path} reports pmor_version() = {have}; this host side needs >= {MIN_MORPH_VERSION} '
                                      '(an older build of the library: rebuild with `make morph`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (pmor_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make morph`')
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
                msg = self.load().pmor_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


morph = _MorphLib()
