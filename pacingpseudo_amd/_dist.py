"""ctypes binding of libpacingpseudo_dist.so (the C ABI declared in include/pacingpseudo_dist.h): exact Euclidean distance
transforms on the device, the signed level-set maps of the boundary loss and the loss itself (``upper_bound_chaos.py
--do_loss_boundary``, ``utils.distance_transform_edt`` / ``utils.signed_distance_maps``, ``losses.boundary_loss``).

It is loaded on first use, never at import.  As with ``_lib``, ``_prep``, ``_rwp`` and ``_unc`` there is NO fallback: a missing or
stale library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make dist``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('pdist_version', 'pdist_last_error', 'pdist_edt_workspace', 'pdist_signed_maps_workspace',
              'pdist_boundary_loss_workspace')      # a value, not a status code


class _DistLib:
    def __init__(self, path=DIST_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: the distance transforms and the boundary loss have no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make dist`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'pdist_version'):
                dll.pdist_version.restype = i32
                have = dll.pdist_version()
            if have < MIN_DIST_VERSION:
                raise HipLibraryError(f'{path} reports pdist_version() = {have}; this host side needs >= {MIN_DIST_VERSION} '
                                      '(an older build of the library: rebuild with `make dist`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (pdist_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make dist`')
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
                msg = self.load().pdist_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


dist = _DistLib()
