"""The registry of the project's C-ABI libraries (pacingpseudo_amd/_binding.py: LIBRARIES): it is the set of binding modules and the
set of libraries `make all` links, every registered library loads through the one loader and resolves every symbol it binds, and
build() checks all of them.  No GPU."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pacingpseudo_amd import _binding  # noqa: E402
from tests import _wiring  # noqa: E402


def test_registry_is_the_binding_modules_and_the_libraries_of_make_all():
    modules = {os.path.basename(p)[1:-3] for p in glob.glob(os.path.join(ROOT, 'pacingpseudo_amd', '_*.py'))} - {'_init__', 'binding'}
    assert set(_binding.LIBRARIES) == modules and len(set(_binding.LIBRARIES)) == len(_binding.LIBRARIES) == 10
    files = {os.path.basename(_binding.binding(name)[1]._spec()[0]) for name in _binding.LIBRARIES}
    assert files == {f'libpacingpseudo_{n}.so' for n in _wiring.libraries_of_all()} and len(files) == 10
    companions = [n for n in _binding.LIBRARIES if n != 'lib']
    assert files == {'libpacingpseudo_hip.so'} | {f'libpacingpseudo_{n}.so' for n in companions}
    phony = _wiring.phony_targets()
    assert set(companions) | {f'asan-{n}' for n in companions} | {'all', 'asan', 'trace', 'study', 'clean'} == set(phony)


@pytest.mark.parametrize('name', _binding.LIBRARIES)
def test_registered_library_loads_through_the_loader_and_resolves_every_symbol(name):
    module, singleton = _binding.binding(name)
    assert type(singleton).load is _binding.CLibrary.load and type(singleton).__getattr__ is _binding.CLibrary.__getattr__
    path, protos, min_version = singleton._spec()
    assert protos is module._PROTOS and tuple(protos) == module.EXPORTED_SYMBOLS
    assert os.path.exists(path), f'{path} is not built (run __graft_entry__.build())'
    fresh = type(singleton)()
    assert fresh._dll is None
    dll = fresh.load()
    for symbol, (restype, argtypes) in protos.items():
        fn = getattr(dll, symbol)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), symbol
    assert getattr(fresh, f'{singleton.prefix}_version')() >= min_version
    assert f'{singleton.prefix}_version' in singleton.int_values and set(singleton.int_values) <= set(protos)


def test_build_checks_every_registered_library_in_order():
    record = _wiring.build_record()
    assert [loaded for loaded, _ in record][:10] == list(_binding.LIBRARIES)
    for (_, resolved), name in zip(record, _binding.LIBRARIES):
        assert set(_binding.binding(name)[0].EXPORTED_SYMBOLS) <= set(resolved), name
