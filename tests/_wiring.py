"""What "this library is wired into the build" means, as facts and not as text of the Makefile or of __graft_entry__.py: the library
is in the registry (pacingpseudo_amd/_binding.py: LIBRARIES), build() loads every library of the registry through the shared loader
and resolves every symbol its module binds, and `make <name>` / `make asan-<name>` resolve, are phony, and name the expected source
and output.  No GPU, and nothing is compiled: make is only asked what it would do."""
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=None)
def make(*args):
    """stdout of `make <args>`, which must succeed."""
    r = subprocess.run(['make', '-C', ROOT, '--no-print-directory', *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.stdout[-2000:] + r.stderr[-2000:])
    return r.stdout


def would_run(*targets):
    """The commands `make -B <targets>` would run, one per line, without running any."""
    return make('-n', '-B', *targets).splitlines()


def phony_targets():
    return re.search(r'^\.PHONY:(.*)$', make('-pn'), flags=re.M).group(1).split()


def libraries_of_all():
    """{name} of every libpacingpseudo_<name>.so that `make all` links."""
    return set(re.findall(r'-o pacingpseudo_amd/lib/libpacingpseudo_(\w+)\.so\b', '\n'.join(would_run('all'))))


_SPY_ON_BUILD = '''
import json, subprocess, sys
import __graft_entry__ as entry
from pacingpseudo_amd import _binding

class Recorder:
    def __init__(self, dll, seen):
        self.__dict__.update(_dll=dll, _seen=seen)

    def __getattr__(self, name):
        self._seen.append(name)
        return getattr(self._dll, name)

names = {id(_binding.binding(name)[1]): name for name in _binding.LIBRARIES}
record, load = [], _binding.CLibrary.load

def spy(self):
    record.append((names.get(id(self)), []))
    return Recorder(load(self), record[-1][1])

_binding.CLibrary.load, subprocess.run = spy, lambda *a, **kw: None          # build() without make: the libraries are built
entry.build()
print('RECORD ' + json.dumps(record))
'''


@functools.lru_cache(maxsize=None)
def build_record():
    """Runs __graft_entry__.build(), with make left out, in a process of its own (this one's singletons stay unloaded) and returns
    [(registry name of the singleton, [symbols resolved on what its load() returned])] in the order build() loaded them."""
    import json
    r = subprocess.run([sys.executable, '-c', _SPY_ON_BUILD], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RECORD ')][-1][len('RECORD '):])


def wired(name, source):
    """Every fact at once for the companion library `name` built from `source` (a path below the repository root)."""
    from pacingpseudo_amd import _binding
    assert name in _binding.LIBRARIES
    module, singleton = _binding.binding(name)
    assert isinstance(singleton, _binding.CLibrary) and os.path.basename(singleton._spec()[0]) == f'libpacingpseudo_{name}.so'
    # build() loads it through the loader and resolves every symbol the module binds
    resolved = [seen for loaded, seen in build_record() if loaded == name]
    assert resolved and set(module.EXPORTED_SYMBOLS) <= set(resolved[0])
    # `make <name>` and `make all` link the library from its source; `make asan-<name>` instruments the source, links it with the
    # stand-alone program and runs that
    out = f'pacingpseudo_amd/lib/libpacingpseudo_{name}.so'
    assert [c for c in would_run(name) if 'hipcc' in c and ' -shared ' in c and source in c and c.endswith(f'-o {out}')]
    assert name in libraries_of_all()
    asan = would_run(f'asan-{name}')
    obj = os.path.splitext(os.path.basename(source))[0] + '.o'
    assert [c for c in asan if 'hipcc' in c and '-Xarch_host -fsanitize=address' in c and f'-c {source} ' in c and c.endswith(obj)]
    assert [c for c in asan if 'clang++' in c and '-fsanitize=address' in c and f'-c tests/native/asan_{name}_args.cpp ' in c]
    assert [c for c in asan if 'hipcc' in c and '-fsanitize=address' in c and f'asan_{name}_args.o' in c and obj in c and c.endswith('-ldl')]
    assert re.fullmatch(rf'ASAN_OPTIONS=detect_leaks=0 \S*/asan_{name}_args', asan[-1])
    assert name in phony_targets() and f'asan-{name}' in phony_targets()
