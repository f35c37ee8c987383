"""ctypes binding of libpacingpseudo_dist.so (the C ABI declared in include/pacingpseudo_dist.h): exact Euclidean distance
transforms on the device, the signed level-set maps of the boundary loss and the loss itself (``upper_bound_chaos.py
--do_loss_boundary``, ``utils.distance_transform_edt`` / ``utils.signed_distance_maps``, ``losses.boundary_loss``).

It is loaded on first use, never at import, by the loader of ``_binding``.  There is NO fallback: a missing or stale library
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make dist``)."""
from __future__ import annotations

import ctypes as C
import os

from ._binding import CLibrary, HipLibraryError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
DIST_LIB_PATH = os.path.join(_HERE, 'lib', 'libpacingpseudo_dist.so')

vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/pacingpseudo_dist.h one to one
_PROTOS = {
    'pdist_version': (i32, []),
    'pdist_last_error': (C.c_char_p, []),
    'pdist_edt_workspace': (sz, [i32, i32, i32]),
    'pdist_edt': (i32, [vp, i32, i32, i32, f32, f32, i32, vp, vp, sz, vp]),
    'pdist_signed_maps_workspace': (sz, [i32, i32, i32, i32]),
    'pdist_signed_maps': (i32, [vp, i32, i32, i32, i32, f32, f32, vp, vp, sz, vp]),
    'pdist_boundary_loss_workspace': (sz, [i32, i32, i32, i32]),
    'pdist_boundary_loss_fwd': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    'pdist_boundary_loss_bwd': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
MIN_DIST_VERSION = 100      # include/pacingpseudo_dist.h (pp_distance.hip: PDIST_VERSION)


class _DistLib(CLibrary):
    prefix, target, no_fallback = 'pdist', 'dist', 'the distance transforms and the boundary loss have no CPU fallback'
    int_values = ('pdist_version',)

    def _spec(self):
        return self._path or DIST_LIB_PATH, _PROTOS, MIN_DIST_VERSION


dist = _DistLib()
