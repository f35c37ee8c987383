"""Sentinel bands around the operands of a launch (device-agnostic: tests/test_guard_helper.py exercises it on CPU tensors).

A kernel's outputs, inputs and workspaces are each placed inside one allocation of their own with GUARD bytes of a known byte
pattern in front of and behind the payload, the tail band starting at the very byte after the payload (no alignment padding: an
8-byte store that begins on the last 4 bytes of a buffer lands in the band).  After the launch the bands are compared AS BYTES,
so half an overwritten fp16 element shows.  Two patterns:
  0xFF  NaN as fp16, bf16, fp32 and fp64 and -1 as any integer: a read outside an input's extent that reaches a result turns
        that result into NaN, and an index read from a band is negative;
  0xA5  a small finite negative value in all of those types (fp32 -2.87e-16, fp16 -0.0201, bf16 -2.87e-16, fp64 -1.2e-127) and
        a large negative integer: what a kernel makes of it differs from what it makes of 0xFF, so two runs of one case that
        differ only in the pattern give the same bits exactly when nothing outside the stated extents is read.
Workspace payloads (GuardedWs) and output payloads built from a shape start as the pattern too: a kernel that depends on stale
workspace content, or leaves part of an output unwritten, gives different bits under the two patterns.  include/pacingpseudo_hip.h
names no workspace region the caller has to clear, so none is cleared; `zero` is there for one that would.
Verdicts are formed on the device -- BandSet.verdicts() concatenates all bands of a launch, compares once and reads ONE result
back -- because a host synchronisation per band would dominate a census of thousands of launches.

The limit: a band sees GUARD = 32 KiB on either side and nothing beyond.  An access further out lands in some other allocation of
the process (or in none) and is not seen here; the bands are that wide so that an off-by-one row, tile or block of the sizes these
kernels use still falls inside them.  Reads are seen only through their effect on a result (NaN, or a difference between the two
patterns), never directly."""
import math

import torch

GUARD = 32 * 1024          # bytes on either side; a multiple of 512: the payload keeps the allocation's base alignment
PATTERNS = (0xFF, 0xA5)
assert GUARD % 512 == 0
_ONE_FILL = 1 << 20          # payloads up to this many bytes: the pattern is laid over the whole allocation in one fill


def _shape_of(x):
    return (int(x),) if isinstance(x, int) else tuple(int(s) for s in x)


class Banded:
    """`payload` (a tensor: copied in; or a shape: filled with the pattern, or with `fill`) between two bands of GUARD bytes.
    .t is the payload view (dtype, shape), .full the whole allocation as bytes."""

    def __init__(self, payload, dtype=None, pattern=0xFF, device=None, fill=None):
        if torch.is_tensor(payload):
            dtype = payload.dtype if dtype is None else dtype
            device = payload.device if device is None else device
            shape = tuple(payload.shape)
        else:
            dtype = torch.float32 if dtype is None else dtype
            shape = _shape_of(payload)
        self.pattern = int(pattern)
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = item * math.prod(shape)
        self.full = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=device)
        stale = not torch.is_tensor(payload) and fill is None
        if stale or self.nbytes <= _ONE_FILL:                  # one fill over everything costs less than two over the bands
            self.full.fill_(self.pattern)
        else:
            self.full[:GUARD] = self.pattern
            self.full[GUARD + self.nbytes:] = self.pattern
        inner = self.full[GUARD:GUARD + self.nbytes]
        self.t = inner.view(dtype).view(shape) if self.nbytes else torch.empty(shape, dtype=dtype, device=device)
        if torch.is_tensor(payload):
            self.t.copy_(payload)
        elif fill is not None:
            self.t.fill_(fill)

    def data_ptr(self):
        return self.full.data_ptr() + GUARD

    ptr = data_ptr

    def bands(self):
        return [self.full[:GUARD], self.full[GUARD + self.nbytes:]]

    def ok(self):
        """One buffer alone, with a host read (tests of the helper; a launch's buffers go through BandSet.verdicts())."""
        return not bool(torch.stack([(b != self.pattern).any() for b in self.bands()]).any())


class GuardedWs(Banded):
    """A workspace of EXACTLY `nbytes` (what the size query returned) with a band behind it (and one in front), the payload stale:
    filled with the pattern, except the (offset, length) byte ranges of `zero` -- regions the header says the caller clears."""

    def __init__(self, nbytes, pattern=0xFF, device=None, zero=()):
        super().__init__((int(nbytes),), torch.uint8, pattern, device)
        self.n = int(nbytes)
        for off, length in zero:
            self.t[off:off + length] = 0


class BandSet:
    """The banded buffers of one launch (or one case): make them here, ask once."""

    def __init__(self, pattern=0xFF, device=None):
        self.pattern, self.device = int(pattern), device
        self.items = []

    def add(self, label, b):
        self.items.append((label or f'buffer {len(self.items)} ({b.t.dtype}{list(b.t.shape)})'.replace('torch.', ''), b))
        return b

    def banded(self, payload, dtype=None, label=None, fill=None):
        dev = None if torch.is_tensor(payload) and self.device is None else self.device
        return self.add(label, Banded(payload, dtype, self.pattern, dev, fill))

    def tensor(self, payload, dtype=None, label=None, fill=None):
        return self.banded(payload, dtype, label, fill).t

    def ws(self, nbytes, label=None, zero=()):
        b = GuardedWs(nbytes, self.pattern, self.device, zero)
        self.items.append((label or f'workspace {len(self.items)} ({b.n} bytes)', b))
        return b

    def verdicts(self):
        """[(label, intact)] of every buffer made so far: one comparison over all bands, one read."""
        if not self.items:
            return []
        bands = torch.cat([band for _, b in self.items for band in b.bands()]).view(len(self.items), 2 * GUARD)
        bad = (bands != self.pattern).any(1).cpu().tolist()
        return [(label, not hit) for (label, _), hit in zip(self.items, bad)]

    def damaged(self):
        return [label for label, ok in self.verdicts() if not ok]
