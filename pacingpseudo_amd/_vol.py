"""ctypes binding of libpacingpseudo_vol.so (the C ABI declared in include/pacingpseudo_vol.h): 3-D connected components, the
keep-largest-3-D-component filter, the exact 3-D Euclidean distance transform and the surface-distance sets of a pair of volumes
(``inference.py --volumes``, ``utils.volume``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make vol``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
VOL_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_vol.so')

vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/pacingpseudo_vol.h one to one
_PROTOS = {
    'pvol_version': (i32, []),
    'pvol_last_error': (C.c_char_p, []),
    'pvol_label_workspace': (sz, [i32, i32, i32]),
    'pvol_keep_largest_workspace': (sz, [i32, i32, i32, i32]),
    'pvol_edt_workspace': (sz, [i32, i32, i32]),
    'pvol_surface_workspace': (sz, [i32, i32, i32, i32]),
    'pvol_label_components': (i32, [vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    'pvol_keep_largest_components': (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    'pvol_edt': (i32, [vp, i32, i32, i32, f32, f32, f32, i32, vp, vp, sz, vp]),
    'pvol_surface_distances': (i32, [vp, vp, i32, i32, i32, i32, f32, f32, f32, vp, vp, vp, sz, vp]),
    'pvol_dice_counts': (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_VOL_VERSION = 100       # include/pacingpseudo_vol.h (pp_volume.hip: PVOL_VERSION)
BRICK = (4, 16, 32)         # voxels (z, y, x) one block joins in LDS (pp_volume.hip: PVOL_BD, PVOL_BH, PVOL_BW)


class _VolLib(CLibrary):
    prefix, target, no_fallback = 'pvol', 'vol', 'volume-wise evaluation has no CPU fallback'
    int_values = ('pvol_version',)

    def _spec(self):
        return self._path or VOL_LIB_PATH, _PROTOS, MIN_VOL_VERSION


vol = _VolLib()
