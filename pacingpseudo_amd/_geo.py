"""ctypes binding of libpacingpseudo_geo.so (the C ABI declared in include/pacingpseudo_geo.h): geodesic distance transforms of
scribble seeds on the device and the pseudo-labels taken from them (``train_chaos.py --geo_scribbles``,
``utils.geodesic_distance`` / ``utils.geodesic_expand_scribbles``, ``scripts/expand_scribbles.py --method geo``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make geo``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

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


class _GeoLib(CLibrary):
    prefix, target, no_fallback = 'pgeo', 'geo', 'the geodesic distance transform has no CPU fallback'
    int_values = ('pgeo_version',)

    def _spec(self):
        return self._path or GEO_LIB_PATH, _PROTOS, MIN_GEO_VERSION


geo = _GeoLib()
