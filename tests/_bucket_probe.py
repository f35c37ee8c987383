"""Two identical data-parallel ranks emulated on one GPU: a GradReducer whose "all-reduce" doubles the bucket in place.

The real reducer hands `flat.grads[lo:hi]` to an asynchronous SUM all-reduce the moment the engine announces bucket `tag`
(StepEngine._bucket -> engine.bucket_hook -> GradReducer.bucket_ready), on the stream the engine chose for the hook.  With two ranks
that hold the same weights and the same batch the sum is 2 x the local gradient, and 2 x is exact in fp32.  ProbeReducer does that
doubling itself, at the same place, on the same stream: after the backward pass the slab must equal twice the slab of the same step
without a reducer, bit for bit.  A gradient stored after its bucket's announcement comes out 1 x, one accumulated afterwards
2 x partial + rest, a bucket announced twice 4 x, one never announced 1 x.

The tiling check at the bottom needs no GPU (tests/test_parallel_gloo.py uses it on CPU slabs).
"""
import torch

from pacingpseudo_amd import parallel


class ProbeReducer(parallel.GradReducer):
    """comm=None: nothing here touches torch.distributed; engine.comm stays None and engine.world 1.  `_range` is inherited, so the
    bucket ranges are the product's own.

    fenced: after the doubling the stream the backward runs on (`main`, set by the test right before loss.backward()) waits for
    it.  Every launch enqueued after the announcement, on either stream, then lands after the doubling, so a late producer is
    caught deterministically instead of merely racing it.  The fence only adds ordering: it cannot make a correct plan fail."""

    def __init__(self, model, fenced=True):
        super().__init__(model, comm=None)
        self.fenced = bool(fenced)
        self.main = None
        self.log = []                 # (tag, the hook ran on the main stream) per announcement of the current backward
        self.snap = {}                # tag -> the bucket as the "all-reduce" found it (the last announcement's, if there were several)
        self.events = {tag: torch.cuda.Event() for tag, _ in parallel.backbone_buckets(model)}      # none created inside a capture
        self.recorded = []

    def bucket_ready(self, flat, tag):
        if self.main is None:
            raise RuntimeError('ProbeReducer.main must be the stream loss.backward() is called on')
        s = torch.cuda.current_stream()
        self.log.append((tag, s == self.main))
        lo, hi = self._range(flat, tag)
        with torch.no_grad():
            self.snap[tag] = flat.grads[lo:hi].clone()
            flat.grads[lo:hi].mul_(2)
        ev = self.events[tag]
        ev.record(s)
        self.recorded.append(ev)
        if self.fenced:
            self.main.wait_event(ev)

    def reduce(self, flat, active):
        """What `work.wait()` does for the real all-reduces: the current stream waits for every bucket (which also rejoins the
        second stream, as a graph capture requires)."""
        cur = torch.cuda.current_stream()
        for ev in self.recorded:
            cur.wait_event(ev)
        self.recorded = []


class NoopComm:
    """Stand-in for parallel.Comm on ONE rank without a process group, to reach the synchronised-BatchNorm kernels
    (pp_bn_lrelu_bwd_sums / _apply): a one-rank SUM is the identity, a one-rank broadcast too."""
    world, rank, group, small = 1, 0, None, None

    def allreduce_sums(self, t):
        pass

    def broadcast_bank(self, bank):
        pass


def loss_fn(args, w_crf=0.3):
    """The loss assembly of tests/test_gpu_graph.py::_loss_fn for whatever losses the flags switch on (plus the gated-CRF term)."""
    from pacingpseudo_amd.utils import gaussian_ramp_up

    def f(out, epoch):
        loss = out['loss_pce']
        if 'loss_ent' in out:
            loss = loss + out['loss_ent'] * gaussian_ramp_up(epoch, args.loss_ent_weight, scale=args.ramp_up_scale)
        if 'loss_cr' in out:
            loss = loss + out['loss_cr'] * gaussian_ramp_up(epoch, args.loss_cr_weight, scale=args.ramp_up_scale)
        if 'loss_crf' in out:
            loss = loss + out['loss_crf'] * w_crf
        if 'loss_aux_cls' in out:
            loss = loss + out['loss_aux_cls'] * args.loss_aux_weight
        if 'loss_memory' in out:
            loss = loss + out['loss_memory'] * args.loss_memory_weight
        return loss
    return f


def expected_tags(model, do_aux):
    return [t for t, _ in parallel.backbone_buckets(model) if do_aux or t != 'aux']


def tiling_errors(flat, ranges, active):
    """ranges: {tag: (lo, hi)} of the buckets a backward announces; active: the slab segments that backward writes.  The ranges must
    be pairwise disjoint and tile every active segment without a gap from its start to the end of its last parameter (what is left
    of the segment is alignment padding, fewer than FlatSlab.ALIGN floats).  Returns a list of messages, empty when all is well."""
    errs = []
    left = dict(ranges)
    for name in active:
        a, b = flat.segments[name]
        end = max(flat.offsets[p] + p.numel() for p in flat.seg_params[name])
        mine = sorted((r, t) for t, r in left.items() if a <= r[0] < b)
        for _, t in mine:
            del left[t]
        pos = a
        for (lo, hi), t in mine:
            if lo != pos or hi <= lo:
                errs.append(f'{name}: bucket {t} covers [{lo}, {hi}) where [{pos}, ...) is next')
            pos = hi
        if pos != end:
            errs.append(f'{name}: the buckets end at {pos}, the last parameter at {end}')
        if not 0 <= b - end < flat.ALIGN:
            errs.append(f'{name}: {b - end} floats between the last parameter and the end of the segment')
    for t, r in left.items():
        errs.append(f'bucket {t} {r} lies in no active segment')
    return errs


def snapshot_failures(probe, flat, loss_scale=1.0):
    """Tags whose final bucket is not exactly twice what the "all-reduce" found (16-bit storage: the backward divides the slab by
    the power-of-two loss scale after the reduce, the snapshot was taken before)."""
    bad = set()
    for tag, snap in probe.snap.items():
        lo, hi = probe._range(flat, tag)
        want = snap * 2
        if loss_scale != 1.0:
            want = want * (1.0 / loss_scale)
        if not torch.equal(flat.grads[lo:hi], want):
            bad.add(tag)
    return bad


def check_buckets(probe, model, flat, ref_grads, two_stream, do_aux, loss_scale=1.0, expect=frozenset()):
    """THE check of tests/test_gpu_buckets.py.  probe: the ProbeReducer of the backward that just ran (synchronised) on `model`;
    ref_grads: the gradient slab of the same step on an identical model without a reducer.  Returns the set of failing tags (plus
    'tiling' / 'padding' / 'reference' entries for failures that belong to no bucket) and asserts that it equals `expect` -- empty
    everywhere but in the positive controls."""
    notes = []
    bad = set()
    want_tags = expected_tags(model, do_aux)
    got_tags = [t for t, _ in probe.log]
    # each expected tag once, nothing else, in the order the backward completes them
    for t in set(want_tags) | set(got_tags):
        n = got_tags.count(t)
        if n != (1 if t in want_tags else 0):
            bad.add(t)
            notes.append(f'{t}: announced {n} times')
    if sorted(got_tags) == sorted(want_tags) and got_tags != want_tags:
        for g, w in zip(got_tags, want_tags):
            if g != w:
                bad.update((g, w))
        notes.append(f'announced in the order {got_tags}, expected {want_tags}')
    # the stream the engine chose for the hook
    for t, on_main in probe.log:
        if on_main == bool(two_stream):
            bad.add(t)
            notes.append(f'{t}: announced on the {"main" if on_main else "second"} stream')
    # final == 2 x what the "all-reduce" found
    late = snapshot_failures(probe, flat, loss_scale)
    bad |= late
    notes += [f'{t}: the bucket changed after its announcement by more than the doubling' for t in sorted(late)]
    # final == 2 x the step without a reducer, bucket by bucket, and the reference is a real gradient
    ranges = {}
    for t in want_tags:
        lo, hi = probe._range(flat, t)
        ranges[t] = (lo, hi)
        r = ref_grads[lo:hi]
        if not (bool(torch.isfinite(r).all()) and bool((r != 0).any())):
            bad.add('reference')
            notes.append(f'{t}: the reference gradient is empty or not finite')
        if not torch.equal(flat.grads[lo:hi], r * 2):
            bad.add(t)
            n1 = int((flat.grads[lo:hi] == r).sum()) - int((r == 0).sum())
            notes.append(f'{t}: not 2 x the reference ({int((flat.grads[lo:hi] != r * 2).sum())} of {hi - lo} elements differ, '
                         f'about {max(n1, 0)} of them 1 x)')
    active = ['backbone'] + (['aux_path'] if do_aux else [])
    for name in active:
        a, b = flat.segments[name]
        end = max(flat.offsets[p] + p.numel() for p in flat.seg_params[name])
        if not torch.equal(flat.grads[a:b], ref_grads[a:b] * 2) and not (bad & set(want_tags)):
            bad.add('reference')
            notes.append(f'segment {name}: not 2 x the reference outside the announced buckets')
        if bool((flat.grads[end:b] != 0).any()) or bool((ref_grads[end:b] != 0).any()):
            bad.add('padding')
            notes.append(f'segment {name}: the alignment padding [{end}, {b}) is not zero')
    errs = tiling_errors(flat, ranges, active)
    if errs:
        bad.add('tiling')
        notes += errs
    assert bad == set(expect), f'failing buckets {sorted(bad)}, expected {sorted(expect)}: ' + '; '.join(notes)
    return bad
