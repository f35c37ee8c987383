"""The happens-before checker of tests/_stream_hazards.py on synthetic logs with a known verdict, and its access table against the
header.  No GPU: the logs are a few lines each, written by hand in the recorder's format; launches are real entry points with
their header argument lists, so every extent goes through the same table the recorded steps go through.
"""
import pytest

from tests import _stream_hazards as H

MAIN, SIDE = 0, 0x7f00dead0000          # stream handles: the null stream and some other one
A, B, X, WS0, WS1 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
GRADS, PARAMS, M, V, STEP = 0x60000000, 0x61000000, 0x62000000, 0x63000000, 0x64000000
N = 4096                                # floats per plain buffer


def L(entry, stream, **kw):
    """One launch: the header's arguments by name (pointers default to null, numbers to 0)."""
    vals = [kw.pop(p.name, None if p.pointer else 0) for p in H.header_params()[entry][:-1]]
    assert not kw, f'{entry} has no parameter {sorted(kw)}'
    return ('L', entry, vals, stream)


def write(buf, stream, n=N):
    return L('pp_fill', stream, p=buf, n=n)


def read(buf, stream, n=N, into=X):
    """Reads buf[0:n) (and writes a scratch buffer of the reader's own)."""
    return L('pp_copy_slab', stream, x=buf, ld_x=n, y=into + (0 if stream == MAIN else 0x1000000), ld_y=n, C=n, P=1)


def col_write(base, c0, c, ld, rows, stream):
    """Writes columns [c0, c0 + c) of a (rows, ld) fp32 row buffer."""
    return L('pp_copy_slab', stream, x=X + (0 if stream == MAIN else 0x1000000), ld_x=c, y=base + 4 * c0, ld_y=ld, C=c, P=rows)


def hazards(log):
    found, total = H.check(log)
    assert (total == 0) == (not found)
    for h in found:             # each report names both entry points, the parameters, the byte ranges and the log positions
        for pos, entry, param, mode, stream, (lo, hi) in (h.first, h.second):
            assert log[pos][1] == entry and param and mode in ('r', 'w', 'rw') and lo < hi
        assert h.first[0] < h.second[0] and h.first[4] != h.second[4] and h.range[0] < h.range[1]
        assert 'w' in h.first[3] + h.second[3]
        assert H.describe(h)
    return found


def dz_protocol(layers=3, buf_of=lambda i: i % 2, drop=()):
    """The engine's weight-gradient protocol (StepEngine._convbn_bwd / _join_side_stream) for `layers` layers and one optimizer
    step: BatchNorm backward writes dz into slot i % 2 on the main stream, the weight gradient reads it on the second stream into
    its piece of the gradient slab (own workspace), the data gradient reads it on the main stream.  Events: 0, 1 = dz_ready[slot],
    2, 3 = wg_done[slot].  buf_of: which dz buffer layer i really uses; drop: kinds of wait left out ('dz_ready', 'wg_done', 'join')."""
    dz = (A, B)
    log, pending = [('B',)], [False, False]
    O = C = 8
    P = 64
    for i in range(layers):
        slot = i % 2
        buf = dz[buf_of(i)]
        if pending[slot] and 'wg_done' not in drop:
            log.append(('W', 2 + slot, MAIN, '_convbn_bwd'))
        log.append(L('pp_bn_lrelu_bwd', MAIN, dy=X, ld_dy=C, z=X + 0x100000, ld_z=C, scale=X + 0x200000, shift=X + 0x201000,
                     save_mean=X + 0x202000, save_invstd=X + 0x203000, gamma=X + 0x204000, dz=buf, ld_dz=C,
                     dgamma=GRADS + 0x8000 + 64 * i, dbeta=GRADS + 0x9000 + 64 * i, dbias_conv=GRADS + 0xa000 + 64 * i,
                     C=C, P_per_group=P, groups=1, workspace=WS0, workspace_bytes=4096))
        log.append(('R', slot, MAIN))
        if 'dz_ready' not in drop:
            log.append(('W', slot, SIDE, '_convbn_bwd'))
        log.append(L('pp_conv3x3_bwd_weight', SIDE, dz=buf, ld_dz=C, O=O, x=X + 0x300000, ld_x=C, Cpad=C, I_true=C, B=1, H=8, W=8, dil=1,
                     dw_oihw=GRADS + 4 * O * C * 9 * i, workspace=WS1, workspace_bytes=4096))
        log.append(('R', 2 + slot, SIDE))
        pending[slot] = True
        log.append(L('pp_conv3x3_bwd_data', MAIN, dz=buf, ld_dz=C, O=O, wb=X + 0x400000, dx=X, ld_dx=C, I=C, B=1, H=8, W=8, dil=1))
    if 'join' not in drop:
        for slot in (0, 1):
            if pending[slot]:
                log.append(('W', 2 + slot, MAIN, '_join_side_stream'))
    log.append(L('pp_adam_step_dev', MAIN, p=PARAMS, g=GRADS, m=M, v=V, n=0x4000, step_dev=STEP))
    return log


NAMES = {0: 'dz_ready', 1: 'dz_ready', 2: 'wg_done', 3: 'wg_done'}


# ------------------------------------------------------------------------------------------------------------ clean
def test_record_then_wait_orders_a_write_against_a_later_read():
    assert not hazards([write(A, MAIN), ('R', 0, MAIN), ('W', 0, SIDE, 'f'), read(A, SIDE)])
    # ... and through a third stream, and through Stream.wait_stream
    T = 0x7f00beef0000
    assert not hazards([write(A, MAIN), ('R', 0, MAIN), ('W', 0, T, 'f'), ('R', 1, T), ('W', 1, SIDE, 'f'), read(A, SIDE)])
    assert not hazards([write(A, MAIN), ('WS', SIDE, MAIN), read(A, SIDE)])


def test_the_dz_slot_protocol_three_layers_deep_is_clean():
    assert not hazards(dz_protocol(3))
    assert not hazards(dz_protocol(5))


def test_reads_of_one_buffer_are_no_hazard():
    assert not hazards([('B',), read(A, MAIN), read(A, SIDE), read(A, MAIN)])


def test_one_stream_throughout_is_clean():
    assert not hazards([write(A, SIDE), read(A, SIDE), write(A, SIDE), write(A, SIDE)])


def test_disjoint_column_slices_of_one_row_buffer_are_clean():
    assert not hazards([col_write(A, 0, 32, 96, 50, MAIN), col_write(A, 32, 64, 96, 50, SIDE)])
    # a 16-bit row buffer through the _h16 twin: columns [0, 32) and [32, 96) of 2-byte elements
    assert not hazards([L('pp_copy_slab_h16', MAIN, x=X, ld_x=32, y=A, ld_y=96, C=32, P=50),
                        L('pp_copy_slab_h16', SIDE, x=X + 0x1000000, ld_x=64, y=A + 2 * 32, ld_y=96, C=64, P=50)])


def test_disjoint_ranges_of_one_slab_are_clean():
    assert not hazards([write(GRADS, MAIN, 1000), write(GRADS + 4000, SIDE, 1000)])


def test_host_barriers_order_everything_before_against_everything_after():
    assert not hazards([write(A, MAIN), ('B',), read(A, SIDE)])
    assert not hazards([write(A, SIDE), ('SS', SIDE), read(A, MAIN)])
    assert not hazards([write(A, SIDE), ('R', 0, SIDE), ('ES', 0), read(A, MAIN)])
    assert hazards([write(A, SIDE), ('SS', MAIN), read(A, MAIN)])           # the wrong stream was synchronised
    assert hazards([('R', 0, SIDE), write(A, SIDE), ('ES', 0), read(A, MAIN)])


# ------------------------------------------------------------------------------------------------------------ flagged
def test_the_same_log_without_the_wait_is_flagged():
    found = hazards([write(A, MAIN), ('R', 0, MAIN), read(A, SIDE)])
    assert len(found) == 1
    h = found[0]
    assert (h.first[1], h.first[2], h.first[3]) == ('pp_fill', 'p', 'w') and (h.second[1], h.second[2], h.second[3]) == ('pp_copy_slab', 'x', 'r')
    assert h.range == (A, A + 4 * N) and (h.first[0], h.second[0]) == (0, 2)


def test_a_wait_issued_before_the_record_binds_to_the_older_record():
    log = [('R', 0, MAIN), write(A, MAIN), ('W', 0, SIDE, 'f'), ('R', 0, MAIN), read(A, SIDE)]
    assert hazards(log)
    assert not hazards([log[0], log[1], log[3], log[2], log[4]])            # the wait behind the second record: ordered


def test_a_wait_on_an_unrecorded_event_orders_nothing():
    assert hazards([write(A, MAIN), ('W', 5, SIDE, 'f'), read(A, SIDE)])


def test_overlapping_column_slices_are_flagged():
    assert hazards([col_write(A, 0, 40, 96, 50, MAIN), col_write(A, 32, 64, 96, 50, SIDE)])
    # other strides: the hulls decide
    assert hazards([col_write(A, 0, 32, 96, 50, MAIN), col_write(A, 32, 32, 64, 50, SIDE)])
    # a column range that wraps round the row is no column range
    assert hazards([col_write(A, 0, 32, 96, 50, MAIN), col_write(A, 80, 48, 96, 49, SIDE)])


def test_a_workspace_shared_by_two_streams_is_flagged():
    def stats(stream, ws):
        return L('pp_bn_stats_sums', stream, z=(A if stream == MAIN else B), ld=8, C=8, P_per_group=64, groups=1,
                 sums=X + (0 if stream == MAIN else 0x1000), workspace=ws, workspace_bytes=4096)
    found = hazards([('B',), stats(MAIN, WS0), stats(SIDE, WS0)])
    assert found and {found[0].first[2], found[0].second[2]} == {'workspace'}
    assert not hazards([('B',), stats(MAIN, WS0), stats(SIDE, WS1)])


def test_a_dz_slot_reused_one_layer_too_early_is_flagged():
    found = hazards(dz_protocol(3, buf_of=lambda i: 0))         # every layer writes dz buffer 0; the events alternate as designed
    pairs = {(h.first[1], h.first[2], h.second[1], h.second[2]) for h in found}
    assert ('pp_conv3x3_bwd_weight', 'dz', 'pp_bn_lrelu_bwd', 'dz') in pairs


@pytest.mark.parametrize('kind', ['dz_ready', 'wg_done', 'join'])
def test_each_wait_of_the_dz_protocol_protects_something(kind):
    """... whether it is never issued or deleted from the finished log (the planted mistakes of the GPU module)."""
    assert hazards(dz_protocol(3, drop=(kind,)))
    full = dz_protocol(3)
    cut = H.without_waits(full, NAMES, kind)
    assert len(cut) < len(full) and hazards(cut)
    assert cut == dz_protocol(3, drop=(kind,))


def test_an_accumulate_flag_turns_a_write_into_a_read_write():
    def slab(acc):
        return H.accesses('pp_copy_slab', L('pp_copy_slab', MAIN, x=A, ld_x=8, y=B, ld_y=8, C=8, P=4, accumulate=acc)[2])
    assert [a.mode for a in slab(0)] == ['r', 'w'] and [a.mode for a in slab(1)] == ['r', 'rw']


def test_a_launch_without_a_row_fails_by_name():
    with pytest.raises(H.MissingRow, match='pp_tta_view'):
        H.check([L('pp_tta_view', MAIN, x=A, out=B, planes=1, H=4, W=4)])


# ------------------------------------------------------------------------------------------------------------ the table
_INTS = dict(dil=1, k=2, tile=4, groups=2, G=2, rows=3, n=1000, training=1, workspace_bytes=4096, stats_bytes=4096, lazy_ld=16)


def _sample(entry, flags=1):
    row = H.TABLE[H.base_entry(entry)]
    vals, addr = [], 0x100000000
    for p in H.header_params()[entry][:-1]:
        if not p.pointer:
            v = _INTS.get(p.name, flags if p.name.startswith('accumulate') else 8)
            vals.append(float(v) if p.ctype in ('float', 'double') else v)
            continue
        addr += 0x10000000
        kind = row[p.name][1]
        if kind == 'host':
            vals.append(('host',))
        elif kind == 'lazy':
            vals.append(('lazy', addr, 16, 2))
        elif kind == 'ptrs':
            vals.append(('ptrs', [addr, addr + 0x1000]))
        elif kind == 'items':
            fields = {f: addr + 0x100000 * (i + 1) for i, f in enumerate(row[p.name][2])}
            vals.append(('items', [dict(fields, O=8, I=8, Ipad=8, C=8, groups=2)]))
        else:
            vals.append(addr)
    return vals


def test_every_row_names_only_parameters_of_the_header():
    hp = H.header_params()
    assert len(hp) >= 200
    for entry, row in H.TABLE.items():
        assert entry in hp, f'{entry} is no entry point of include/pacingpseudo_hip.h'
        assert hp[entry][-1].name == 'stream', f'{entry} is no launch'
        names = {p.name for p in hp[entry] if p.pointer}
        assert set(row) <= names, f'{entry}: {sorted(set(row) - names)} are no pointer parameters of the header'


def test_every_row_classifies_every_pointer_parameter():
    hp = H.header_params()
    for entry, row in H.TABLE.items():
        for p in hp[entry][:-1]:
            if p.pointer:
                assert p.name in row, f'{entry}: {p.name} is not classified'
                assert row[p.name][0] in ('r', 'w', 'rw') or row[p.name][0][2:] in {q.name for q in hp[entry]}, (entry, p.name)


def test_every_row_evaluates_on_a_sample_argument_list():
    from pacingpseudo_amd import _lib
    hp = H.header_params()
    for entry in H.TABLE:
        twins = [entry] + [entry + s for s in ('_h16', '_bf16') if entry + s in hp]
        assert (len(twins) == 3) == (entry in _lib._H16_SET), entry
        for e in twins:
            acc = H.accesses(e, _sample(e))
            assert acc, e
            pointers = [p.name for p in hp[e][:-1] if p.pointer and H.TABLE[entry][p.name][1] != 'host']
            got = {a.param.split('[')[0].split('.')[0] for a in acc}
            # (an operand the call does not read when another one is given -- x beside a cached V -- has a conditional row count)
            optional = {k for k, v in H.TABLE[entry].items() if v[1] == 'nhwc' and 'None' in v[2]}
            assert got <= set(pointers) and set(pointers) - got <= optional, (e, set(pointers) ^ got)
            for a in acc:
                assert a.rows >= 1 and a.row_bytes > 0 and a.base > 0 and (a.rows == 1 or a.stride >= a.row_bytes), (e, a)
            # a 'w+flag' parameter is read-write with the flag and a plain write without it
            flagged = {k for k, v in H.TABLE[entry].items() if v[0].startswith('w+')}
            off = {a.param: a.mode for a in H.accesses(e, _sample(e, flags=0))}
            for a in acc:
                if a.param in flagged:
                    assert (a.mode, off[a.param]) == ('rw', 'w'), (e, a.param)


def test_element_sizes_come_from_the_prototype_that_was_called():
    z32 = {a.param: a for a in H.accesses('pp_bn_lrelu_fwd', _sample('pp_bn_lrelu_fwd'))}
    for twin in ('pp_bn_lrelu_fwd_h16', 'pp_bn_lrelu_fwd_bf16'):
        z16 = {a.param: a for a in H.accesses(twin, _sample(twin))}
        assert (z32['z'].row_bytes, z16['z'].row_bytes) == (32, 16) and (z32['y'].stride, z16['y'].stride) == (32, 16)
        assert z32['scale'].row_bytes == z16['scale'].row_bytes == 4 * 2 * 8       # coefficient rows stay fp32
