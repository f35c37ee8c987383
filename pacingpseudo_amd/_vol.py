"""ctypes binding of libpacingpseudo_vol.so (the C ABI declared in include/pacingpseudo_vol.h): 3-D connected components, the
keep-largest-3-D-component filter, the exact 3-D Euclidean distance transform and the surface-distance sets of a pair of volumes
(``inference.py --volumes``, ``utils.volume``).

It is loaded on first use, never at import.  As with ``_lib``, ``_prep``, ``_rwp``, ``_unc``, ``_dist`` and ``_geo`` there is NO
fallback: a missing or stale library raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make vol``)."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipLibraryError

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
_NO_STATUS = ('pvol_version', 'pvol_last_error', 'pvol_label_workspace', 'pvol_keep_largest_workspace', 'pvol_edt_workspace',
              'pvol_surface_workspace')      # a value, not a status code


class _VolLib:
    def __init__(self, path=VOL_LIB_PATH):
        self._path = path
        self._dll = None

    def load(self):
        if self._dll is None:
            path = self._path
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: volume-wise evaluation has no CPU fallback. '
                    'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `make vol`)')
            dll = C.CDLL(path)
            have = -1
            if hasattr(dll, 'pvol_version'):
                dll.pvol_version.restype = i32
                have = dll.pvol_version()
            if have < MIN_VOL_VERSION:
                raise HipLibraryError(f'{path} reports pvol_version() = {have}; this host side needs >= {MIN_VOL_VERSION} '
                                      '(an older build of the library: rebuild with `make vol`)')
            missing = [name for name in _PROTOS if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} (pvol_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `make vol`')
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
                msg = self.load().pvol_last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper
        return checked


vol = _VolLib()
