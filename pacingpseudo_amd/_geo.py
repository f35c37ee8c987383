"""ctypes binding of libpacingpseudo_geo.so (the C ABI declared in include/pacingpseudo_geo.h): geodesic distance transforms of
scribble seeds on the device and the pseudo-labels taken from them (``train_chaos.py --geo_scribbles``,
``utils.geodesic_distance`` / ``utils.geodesic_expand_scribbles``, ``scripts/expand_scribbles.py --method geo``).

It is loaded on first use, never at import.  As with ``_lib``, ``_prep``, ``_rwp``, ``_unc`` and ``_dist`` there is NO fallback: a
missing or stale library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make geo``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

_HERE = os.path.dirname(os.path.abspath(__file__))
GEO_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_geo.so')

vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
ip = C.POINTER(C.c_int)          # the HOST table of sizes, or None

# name -> (restype, argtypes); mirrors include/pacingpseudo_geo.h one to one
_PROTOS = {
    'pgeo_version': (i32, []),
    'pgeo_last_error': (C.c_char_p, []),
    'pgeo_normalize': (i32, [vp, ip, i32, i32, i32, vp, vp]),
    'pgeo_distance_workspace': (sz, [i32, i32, i32, i32]),
    'pgeo_distance': (i32, [vp, vp, ip, i32, i32, i32, i32, f32, i32, vp, vp, vp, sz, vp]),
    'pgeo_labels': (i32, [vp, vp, ip, i32, i32, i32, i32, f32, f32, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_GEO_VERSION = 100       # include/pacingpseudo_geo.h (pp_geodesic.hip: PGEO_VERSION)
_NO_STATUS = ('pgeo_version', 'pgeo_last_error', 'pgeo_distance_workspace')      # a value, not a status code


class _GeoLib:
    def __init__(self, path=GEO_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the geodesic distance transform has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make geo`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'pgeo_version'):
                dll.pgeo_version.restype = i32
                have = dll.pgeo_version()
            if have < MIN_GEO_VERSION:
                raise HipLibraryError(f'{path} reports pgeo_version() = {have}; this host side needs >= {MIN_GEO_VERSION} '
                                      '(an older build of the library: rebuild with `make geo`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (pgeo_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make geo`')
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
                msg = self.load().pgeo_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


geo = _GeoLib()
