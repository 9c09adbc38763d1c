"""tbk_bam_decode_open: a batch of whole BGZF members whose record stream may end inside a record.  Hand-built records
(tests/bam_craft.py) framed around a member edge and cut at EVERY byte offset of a three-record window: the record count and tail_off
are the model's (the records that end at or before the cut; where the last of them ends) on both record-index routes; and feeding the
tail forward, batch after batch, reproduces tbk_bam_decode_spans of the whole stream column for column."""
import ctypes
import struct

import numpy as np
import pytest

import bam_craft as bc

pytestmark = pytest.mark.gpu

CORE = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")
N_REF = len(bc.REFS)


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.set_debug("")
    c.bam_release()
    c.close()


def _recs(n=9):
    out = []
    for i in range(n):
        aux, kw = b"", {}
        if i % 3 == 1:
            aux, kw = bc.tag("YC", "f", 2.0 + i), dict(yc=2.0 + i, seen=1)
        elif i % 3 == 2:
            aux, kw = bc.tag("YC", "f", 0.0) + bc.tag("YX", "C", 3 + i), dict(yc=0.0, yx=3 + i, seen=3)
        cigar = ((20 + i, bc.M),) if i % 2 else ((10, bc.M), (100 + i, bc.N), (7, bc.M), (2, bc.S))
        out.append(bc.Rec(tid=i // 8, pos=100 + 13 * (i % 4), flag=4 if i == 5 else 0, cigar=cigar, name=b"q%d" % i + b"x" * (i % 5), aux=aux, **kw))
    return out


def _stream(recs):
    s = b"".join(r.raw for r in recs)
    offs = np.concatenate([[0], np.cumsum([len(r.raw) for r in recs])]).astype(int)
    return s, offs


def _members(stream, cuts):
    """whole members of the stream cut at `cuts`, without the EOF member; and their payload sizes"""
    data = bc.frame(stream, cuts)[:-28]
    edges = [0] + sorted(cuts) + [len(stream)]
    return data, [b - a for a, b in zip(edges, edges[1:])]


def _seen(ptr, n):
    a = np.empty(n, np.uint8)
    if n:
        assert ptr
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(n), 2) == 0
    return a


def _expect(recs):
    return bc.Scene("open", [], [recs], [1]).expect()


def _assert_tile(ctx, s, seen, recs, what):
    want = _expect(recs)
    assert s.n_records == len(recs) and s.n_cigar_ops == len(want["cig"]), what
    if not recs:
        return
    got = ctx.soa_to_numpy(s, fields=CORE + bc.CARRIED)
    for a in CORE + bc.CARRIED:
        assert np.array_equal(got[a], want[a]), (what, a)
    assert np.array_equal(_seen(seen, s.n_records), want["seen"]), what


@pytest.mark.parametrize("route", ["default", "chain"])
@pytest.mark.parametrize("edge", ["inside_a_record", "on_a_record_boundary"])
def test_every_cut_of_a_window_around_a_member_edge(ctx, route, edge):
    recs = _recs()
    stream, offs = _stream(recs)
    k = 4
    E = int(offs[k]) + (17 if edge == "inside_a_record" else 0)     # the member edge: inside record k, or where it begins
    lo, hi = int(offs[k - 1]), int(offs[k + 2])                      # records k - 1, k, k + 1
    assert lo < E < hi and (E in offs) == (edge == "on_a_record_boundary")
    ctx.set_debug("index_chain=1" if route == "chain" else "")
    seen_counts = set()
    for c in range(lo, hi + 1):
        data, sizes = _members(stream[:c], [E] if E < c else [])
        count = int(np.searchsorted(offs, c, side="right")) - 1      # records that end at or before c
        s, seen, tail = ctx.bam_decode_open(data, 0, N_REF)
        assert (s.n_records, tail) == (count, int(offs[count])), (c, s.n_records, tail)
        seen_counts.add(count)
        if c in (lo, E, E + 1, hi - 1, hi) or c - int(offs[count]) in (0, 1, 3, 4, 5):   # (the columns where the cut is of a new kind)
            _assert_tile(ctx, s, seen, recs[:count], c)
    assert seen_counts == {k - 1, k, k + 1, k + 2}
    ctx.set_debug("")


@pytest.mark.parametrize("route", ["default", "chain"])
@pytest.mark.parametrize("msize,per_batch", [(97, 2), (31, 3), (4096, 1)], ids=["straddle_one", "straddle_two", "one_member"])
def test_feeding_the_tail_forward_gives_the_whole_stream(ctx, route, msize, per_batch):
    """members of msize payload bytes (97: records straddle one edge; 31: two and more; 4096: everything in one member), per_batch new
    members a batch.  The next batch starts again with the member that holds the tail."""
    recs = _recs(23)
    stream, offs = _stream(recs)
    cuts = list(range(msize, len(stream), msize))
    data, sizes = _members(stream, cuts)
    if msize == 31:
        assert max(len(r.raw) for r in recs) > 2 * msize
    # the members' extents in the compressed bytes
    cstart, off = [], 0
    while off < len(data):
        cstart.append(off)
        off += struct.unpack_from("<H", data, off + 16)[0] + 1
    cstart.append(len(data))
    ustart = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    nm = len(sizes)
    ctx.set_debug("index_chain=1" if route == "chain" else "")
    whole, _, wseen = ctx.bam_decode_spans([(data, 0, 0)], N_REF)
    _assert_tile(ctx, whole, wseen, recs, "whole")
    got, m0, uoff, m1, batches = [], 0, 0, 0, 0
    while m1 < nm:
        m1 = min(nm, max(m1, m0) + per_batch)                        # at least per_batch members beyond what the last batch had
        s, seen, tail = ctx.bam_decode_open(data[cstart[m0]:cstart[m1]], uoff, N_REF)
        n = int(s.n_records)
        first = len(got)
        _assert_tile(ctx, s, seen, recs[first:first + n], (m0, m1))
        got += recs[first:first + n]
        a = int(ustart[m0]) + tail                                   # the tail in the stream
        assert a == int(offs[len(got)]) and a <= int(ustart[m1])
        if n == 0:
            assert tail == uoff
        m = int(np.searchsorted(ustart, a, side="right")) - 1        # the member that holds it
        m0, uoff = min(m, nm - 1), a - int(ustart[min(m, nm - 1)])
        batches += 1
    assert len(got) == len(recs) and int(ustart[m0]) + uoff == len(stream) and (batches >= 2 or msize == 4096)
    ctx.set_debug("")


def test_what_stays_an_error(ctx):
    from tiebrush_amd import api
    recs = _recs()
    stream, offs = _stream(recs)
    good, sizes = _members(stream, [int(offs[4]) + 9])
    # a block_size below 32 in the tail, whole or cut
    for extra in (struct.pack("<I", 31) + b"\0" * 31, struct.pack("<I", 31)):
        data, _ = _members(stream + extra, [int(offs[4]) + 9])
        for spec in ("", "index_chain=1"):
            ctx.set_debug(spec)
            with pytest.raises(api.TbkError) as e:
                ctx.bam_decode_open(data, 0, N_REF)
            assert e.value.status == -1
    ctx.set_debug("")
    with pytest.raises(api.TbkError) as e:                            # an offset outside its member
        ctx.bam_decode_open(good, sizes[0] + 1, N_REF)
    assert e.value.status == -1
    with pytest.raises(api.TbkError) as e:                            # a refID the header does not have
        ctx.bam_decode_open(good, 0, 1)
    assert e.value.status == -1
    s, seen, tail = ctx.bam_decode_open(good, 0, N_REF)              # and the context takes the next call
    assert (s.n_records, tail) == (len(recs), len(stream))
    # no whole record: an empty tile, the tail where the stream started; no member at all: the same
    data, _ = _members(stream[:int(offs[1]) - 1], [])
    s, seen, tail = ctx.bam_decode_open(data, 0, N_REF)
    assert (s.n_records, tail) == (0, 0)
    s, seen, tail = ctx.bam_decode_open(b"", 0, N_REF)
    assert (s.n_records, tail) == (0, 0)
    # tbk_bam_decode_spans still refuses the stream that ends inside a record
    data, _ = _members(stream[:int(offs[3]) + 5], [])
    with pytest.raises(api.TbkError) as e:
        ctx.bam_decode_spans([(data, 0, 0)], N_REF)
    assert e.value.status == -1
