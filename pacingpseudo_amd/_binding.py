"""How a C-ABI library of this project is found, version-checked, symbol-checked, typed and status-wrapped: the one loader behind
``_lib`` (the per-step library) and its companions, and the list of all of them.

There is deliberately NO fallback: a missing or stale library, or a call that fails, raises.  Nothing is loaded at import; a
library is loaded the first time one of its entry points is asked for."""
from __future__ import annotations

import ctypes as C
import importlib
import os

# every library of the project, in the order they were added: `name` is bound by the module ``_<name>`` whose singleton is ``<name>``
LIBRARIES = ('lib', 'prep', 'rwp', 'unc', 'dist', 'geo', 'vol', 'morph', 'opt', 'lov')


def binding(name):
    """(binding module, its lazily loading singleton) of one of ``LIBRARIES``."""
    module = importlib.import_module(f'{__package__}._{name}')
    return module, getattr(module, name)


class HipLibraryError(RuntimeError):
    pass


class CLibrary:
    """One shared library behind ctypes.  A binding module subclasses it with the symbol prefix, the make target that builds the
    library, the phrase of the "is missing" message that says what has no CPU fallback, the int-typed entry points that return a
    value (every other ``int`` is a status code), and ``_spec()``."""
    prefix = target = no_fallback = None
    int_values = ()
    or_else = ''           # what else a stale library's message may advise

    def __init__(self, path=None):
        self._path = path
        self._dll = None

    def _spec(self):
        """(path, {name: (restype, argtypes)}, minimum version) -- read from the binding module when the library is loaded, not
        when the instance is made."""
        raise NotImplementedError

    def load(self):
        if self._dll is None:
            path, protos, min_version = self._spec()
            prefix, make = self.prefix, f'make {self.target}'.rstrip()
            if not os.path.exists(path):
                raise HipLibraryError(
                    f'{path} is missing: {self.no_fallback}. '
                    f'Build it first: python -c "import __graft_entry__ as g; g.build()" (or `{make}`)')
            dll = C.CDLL(path)
            # a library of another revision must say so in words, not fail with an AttributeError in the middle of a step
            # (ADVICE r05): version first, then every symbol the host side binds
            have = -1
            if hasattr(dll, f'{prefix}_version'):
                version = getattr(dll, f'{prefix}_version')
                version.restype = C.c_int
                have = version()
            if have < min_version:
                raise HipLibraryError(f'{path} reports {prefix}_version() = {have}; this host side needs >= {min_version} '
                                      f'(an older build of the library: rebuild with `{make}`{self.or_else})')
            missing = [name for name in protos if not hasattr(dll, name)]
            if missing:
                raise HipLibraryError(f'{path} ({prefix}_version {have}) lacks {len(missing)} entry point(s) this host side binds, e.g. '
                                      f'{", ".join(missing[:4])}: header / library mismatch, rebuild with `{make}`')
            for name, (res, args) in protos.items():
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = res, args
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        dll = self.load()
        fn = getattr(dll, name)
        if fn.restype is not C.c_int or name in self.int_values:      # a size, a query, a text: a value, not a status code
            return fn
        last_error = getattr(dll, f'{self.prefix}_last_error')

        def checked(*a):
            rc = fn(*a)
            if rc != 0:
                msg = last_error()
                raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else "?"}')
        checked.__name__ = name
        setattr(self, name, checked)             # cache the wrapper: the next lookup finds an instance attribute
        return checked
