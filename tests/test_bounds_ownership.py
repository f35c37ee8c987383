"""Ownership gate (no GPU): every launch entry point of the library -- an entry of _lib._PROTOS whose last argument is the stream,
the _h16 / _bf16 twins included -- runs behind sentinel bands somewhere: it is owned by an adapter of one of the two censuses
(tests/test_gpu_conv_census.py, tests/test_gpu_stream_census.py; an adapter owns its entry in every storage type -- that the twin
is really replayed in its storage type is measured on the GPU,
tests/test_gpu_stream_census.py::test_twins_the_ownership_gate_counts_are_replayed; the six twins no 16-bit plan reaches are in the
bounds table by name) or by a family of the bounds table (tests/test_gpu_bounds.py).  A new entry point without either fails
here BY NAME, before anybody has a GPU."""
import ctypes

# Launch entry points that may go without bands: only ones that write no caller-provided buffer, each with its reason.  Nothing
# that takes an output or a workspace pointer belongs here.  (The profiling, range and query calls -- pp_prof_*, pp_range_*,
# pp_*_workspace / _rows / _elems / _bytes / _plan / _splits -- take no stream and are no launches; pp_mfma_probe writes `out`
# and is in the bounds table.)
EXEMPT = {}


def _launches():
    from pacingpseudo_amd._lib import _PROTOS
    return {name: args for name, (_, args) in _PROTOS.items() if args and args[-1] is ctypes.c_void_p}


def _base(name):
    from pacingpseudo_amd._lib import _PROTOS
    for suffix in ('_h16', '_bf16'):
        if name.endswith(suffix) and name[:-len(suffix)] in _PROTOS:
            return name[:-len(suffix)], suffix
    return name, ''


def _owners():
    """{launch entry: owner}"""
    from tests import test_gpu_bounds as B
    from tests import test_gpu_conv_census as CC
    from tests import test_gpu_stream_census as SC
    table = {e: f'bounds table: {family}' for family, entries in B.owned_by_family().items() for e in entries}
    census = {**{e: 'convolution census' for e in CC.ADAPTERS}, **{e: 'stream census' for e in SC.ADAPTERS}}
    out = {}
    for name in _launches():
        base, _ = _base(name)
        if name in table:
            out[name] = table[name]
        elif base in census:
            out[name] = census[base]
        elif name in EXEMPT:
            out[name] = 'exempt: ' + EXEMPT[name]
    return out


def test_every_launch_entry_point_is_owned_by_a_census_or_the_bounds_table():
    launches, owners = _launches(), _owners()
    orphans = sorted(set(launches) - set(owners))
    assert not orphans, f'launch entry points that never run behind sentinel bands (no census adapter, no bounds-table family): {orphans}'
    per = {'': 0, '_h16': 0, '_bf16': 0}
    for name in launches:
        if name not in EXEMPT:
            per[_base(name)[1]] += 1
    print(f'\nlaunch entry points: {len(launches)}; behind bands: fp32 {per[""]}, fp16 {per["_h16"]}, bf16 {per["_bf16"]}; '
          f'exempt: {sorted(EXEMPT)}')
    assert len(launches) >= 200 and per['_h16'] == per['_bf16'] >= 42


def test_exemptions_take_no_buffer():
    """An exempt entry has no pointer argument but the stream: it cannot write a caller's buffer."""
    launches = _launches()
    for name, reason in EXEMPT.items():
        assert name in launches and reason, name
        pointers = [t for t in launches[name][:-1] if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))]
        assert not pointers, f'{name} takes {len(pointers)} pointer(s): it needs an owner, not an exemption'


def test_bounds_table_names_real_launches_and_calls_what_it_claims():
    """Every entry a bounds case names exists and is a launch; no family is empty; the table does not claim what a census owns
    only through a twin it never calls (a name is owned by the table only if a case calls exactly that name)."""
    from tests import test_gpu_bounds as B
    launches = _launches()
    for family, entries in B.owned_by_family().items():
        assert entries, family
        for e in entries:
            assert e in launches, (family, e)
    for tag, (_, entries) in B.CASES.items():
        assert entries, tag


def test_removing_a_family_names_its_entry_points(monkeypatch):
    """The gate bites: without one family's row the gate names exactly the entry points only that family owned."""
    from tests import test_gpu_bounds as B
    family = next(f for f in B.FAMILIES if 'clipping' in f)
    monkeypatch.setitem(B.FAMILIES, family, lambda: {})
    orphans = sorted(set(_launches()) - set(_owners()))
    assert orphans == ['pp_grad_clip_finalize', 'pp_grad_sumsq'], orphans
