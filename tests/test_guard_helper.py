"""tests/_guard.py on CPU tensors: damage planted with plain tensor writes is reported, buffer by buffer, and the intact case
passes -- the proof that the bounds gate of tests/test_gpu_bounds.py and of the two censuses bites, without a kernel."""
import pytest
import torch

from tests._guard import GUARD, PATTERNS, Banded, BandSet, GuardedWs

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8]


def test_guard_width_keeps_the_base_alignment():
    assert GUARD == 32 * 1024 and GUARD % 512 == 0
    b = Banded((3, 5), torch.float16)
    assert b.t.data_ptr() == b.full.data_ptr() + GUARD == b.data_ptr()
    assert b.full.numel() == 2 * GUARD + 3 * 5 * 2 and b.nbytes == 30


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).replace('torch.', ''))
def test_patterns_read_as_documented(pattern, dtype):
    """0xFF: NaN in every float type, -1 in every signed integer; 0xA5: finite and small in every float type."""
    t = Banded((4,), dtype, pattern).t
    if dtype.is_floating_point:
        if pattern == 0xFF:
            assert bool(torch.isnan(t).all())
        else:
            assert bool(torch.isfinite(t).all()) and float(t.double().abs().max()) < 0.05 and float(t.double().abs().min()) > 0
    elif dtype != torch.uint8:
        assert bool((t == -1).all()) if pattern == 0xFF else bool((t < 0).all())


@pytest.mark.parametrize('pattern', PATTERNS)
def test_payload_of_a_tensor_is_copied_and_bands_are_intact(pattern):
    src = torch.arange(35, dtype=torch.float32).reshape(5, 7)
    b = Banded(src, pattern=pattern)
    assert torch.equal(b.t, src) and b.t.shape == src.shape and b.ok()
    b.t.mul_(2.0)                                           # writing the whole payload touches no band
    assert b.ok()
    assert Banded((2, 3), torch.float32, pattern, fill=7.0).t.eq(7.0).all()


PLANTS = {'one byte just before the payload': lambda b: GUARD - 1, 'one byte just after the payload': lambda b: GUARD + b.nbytes,
          'the far end of the front band': lambda b: 0, 'the far end of the tail band': lambda b: 2 * GUARD + b.nbytes - 1}


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('where', sorted(PLANTS))
def test_one_planted_byte_is_reported_for_that_buffer_alone(where, dtype, pattern):
    bs = BandSet(pattern)
    a, b, c = (bs.banded((3, 5), dtype, label=lab) for lab in 'abc')
    ws = bs.ws(1000, label='ws')
    assert bs.damaged() == [] and all(ok for _, ok in bs.verdicts())
    b.full[PLANTS[where](b)] = 0x00                         # a plain tensor write; any value but the pattern
    assert bs.damaged() == ['b'], where
    assert a.ok() and not b.ok() and c.ok() and ws.ok()


@pytest.mark.parametrize('pattern', PATTERNS)
def test_half_an_overwritten_16_bit_element_is_seen(pattern):
    """Bands are compared as bytes: a 16-bit value whose low byte equals the pattern and whose high byte does not."""
    b = Banded((7,), torch.float16, pattern)
    b.full[GUARD + b.nbytes + 1] = pattern ^ 0x80
    assert not b.ok()


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('nbytes', [1, 13, 16, 1000, 4096 + 8])
def test_one_byte_past_a_workspace_size_is_reported(nbytes, pattern):
    """GuardedWs holds exactly nbytes: byte nbytes - 1 is the workspace's, byte nbytes is not (no rounding up to 16)."""
    bs = BandSet(pattern)
    ws = bs.ws(nbytes, label='ws')
    assert ws.n == nbytes and ws.t.numel() == nbytes and bool((ws.t == pattern).all()), 'the payload starts stale'
    ws.t[nbytes - 1] = 0
    assert bs.damaged() == []
    ws.full[GUARD + nbytes] = 0
    assert bs.damaged() == ['ws']


def test_workspace_regions_the_caller_clears():
    ws = GuardedWs(64, 0xA5, zero=[(16, 8)])
    assert ws.t[16:24].eq(0).all() and ws.t[:16].eq(0xA5).all() and ws.t[24:].eq(0xA5).all() and ws.ok()


def test_default_labels_name_the_buffer():
    bs = BandSet(0xFF)
    x = bs.tensor(torch.zeros(2, 3))
    bs.ws(40)
    x.view(-1)[0] = 1.0
    bs.items[1][1].full[GUARD + 40] = 1
    assert bs.damaged() == ['workspace 1 (40 bytes)']
    assert bs.verdicts()[0] == ('buffer 0 (float32[2, 3])', True)


def test_an_empty_payload_has_adjacent_bands():
    b = Banded((0,), torch.float32)
    assert b.nbytes == 0 and b.ok() and b.full.numel() == 2 * GUARD


def test_replay_table_reports_a_device_pointer_that_is_not_between_bands():
    """The censuses' entry-point table (_Checked) looks at every void* argument of a launch: one that points into no banded buffer
    of the run adds a failing result line naming the argument; banded pointers, null pointers and the stream add none."""
    from types import SimpleNamespace
    from tests.test_gpu_conv_census import _Checked
    calls = []
    inner = SimpleNamespace(pp_scale=lambda *a: calls.append(a), pp_grad_sumsq_rows=lambda n: 7)
    run = SimpleNamespace(bands=BandSet(0xFF), res=[])
    table = _Checked(inner, run)
    inside, outside = run.bands.tensor(torch.zeros(8)), torch.zeros(8)
    table.pp_scale(inside.data_ptr(), 8, 2.0, 0)
    table.pp_scale(inside[4:].data_ptr(), 4, 2.0, None)
    assert run.res == [] and len(calls) == 2
    table.pp_scale(outside.data_ptr(), 8, 2.0, 0)
    table.pp_scale(inside.data_ptr() + 32, 1, 2.0, 0)          # one past the payload: the tail band, not the buffer
    assert len(run.res) == 2
    del run.res[1]
    assert [r[0] for r in run.res] == ['pp_scale argument 0 points into no banded buffer'] and run.res[0][2] is False and len(calls) == 4
    assert table.pp_grad_sumsq_rows(5) == 7                     # a query, not a launch: passed through
