"""The one-region entries run the table path (region.hip: one region is a table of one interval).  Hand-built rows and records at the
sizes where a 256-thread block, and the n + 1 launch of the closing offsets, can go wrong (0, 1, 255, 256, 257), held against the numpy
restatement of the contract: region_fixtures.clip_cov / clip_sample for the rows (for sorted, disjoint rows that mask IS the bisected
range, an empty region included) and Fixture.brute for the records.  Wherever the region is not empty the table entry with that one
interval must give the same arrays, byte for byte.  The one thing the fold changes is asserted at the end: interval rows that are not
sorted and disjoint are refused by the one-region clips too."""
import numpy as np
import pytest

import bam_craft as bc
import csi_reader as cr
import region_fixtures as rf
from test_gpu_region import COV_KEYS, SAMP_KEYS, _assert_rows, ctx  # noqa: F401  (the context fixture and the byte compare of `tiecov -r`)
from test_gpu_regions import _view_arrays

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257)
J_KEYS = COV_KEYS[4:]
J_DTYPES = dict(j_tid=np.int32, j_start=np.int32, j_end=np.int32, j_strand=np.uint8, j_val=np.float64)
FAR = 1 << 40
NAMES, LENS = ["chrA", "chrB", "chrC", "chrD"], [1000000, 1000000, 1000000, 1000000]


# ---- the clips --------------------------------------------------------------------------------------------------------------------------
def _rows(n):
    """n interval rows, sorted and disjoint, on references 0 and 2 (none on 1 and 3): 20 long, 10 apart, every third one abuts its
    successor; the payload columns tell the rows apart"""
    i = np.arange(n)
    h = (n + 1) // 2                                                   # rows [0, h) on reference 0, the rest on reference 2
    k = np.where(i < h, i, i - h)
    start = (100 + 30 * k).astype(np.int32)
    end = (start + np.where(k % 3 == 1, 30, 20)).astype(np.int32)     # (row 3q + 1 reaches its successor's start)
    tid = np.where(i < h, 0, 2).astype(np.int32)
    w = dict(iv_tid=tid, iv_start=start, iv_end=end, iv_val=i + 0.5, s_tid=tid.copy(), s_start=start.copy(), s_end=end.copy(),
             s_count=(3 * i + 1).astype(np.int64), s_heat=(i / 7).astype(np.float32))
    w.update({k: np.zeros(0, dtype=d) for k, d in J_DTYPES.items()})
    return w


def test_the_rows_are_sorted_and_disjoint_and_some_abut():
    for n in SIZES[1:]:
        w = _rows(n)
        t, s, e = w["iv_tid"], w["iv_start"], w["iv_end"]
        same = t[1:] == t[:-1]
        assert np.all(e > s) and np.all(t[1:] >= t[:-1]) and np.all(s[1:][same] >= e[:-1][same])
        if n > 4:
            assert np.any(s[1:][same] == e[:-1][same]) and np.any(s[1:][same] > e[:-1][same]) and set(t) == {0, 2}


def _clip_regions(w):
    """(what, tid, beg, end) around the middle row, the first and the last one; `what` names the shape the model must show"""
    t, s, e = w["iv_tid"], w["iv_start"], w["iv_end"]
    n = len(t)
    if n == 0:
        return [("none", 0, 0, 100), ("none", 0, 50, 50), ("none", 1, 0, FAR)]
    k = 3 * (n // 6)                                                   # a row with a gap on both sides (k % 3 == 0), on reference 0
    T, S, E = int(t[k]), int(s[k]), int(e[k])
    L = n - 1
    R = [("one", T, S, E),                                             # equals a row
         ("not-k", T, E, E + 15),                                      # starts at the row's end: that row is dropped
         ("none", T, S - 5, S),                                        # ends at the row's start (inside the gap before it)
         ("one", T, S + 3, E - 3),                                     # strictly inside the row
         ("none", int(t[0]), 0, int(s[0])), ("none", int(t[0]), 0, int(s[0]) - 1),       # before the first row
         ("none", int(t[L]), int(e[L]), int(e[L]) + 100), ("none", int(t[L]), int(e[L]) + 5, FAR),   # behind the last row
         ("none", 1, 0, 100000), ("none", 3, 0, FAR),                  # references without a row: between the rows' two, behind both
         ("point", T, S + 5, S + 5),                                   # empty, at a point inside the row: that row, trimmed to length 0
         ("none", T, E + 5, E + 5),                                    # empty, in the gap
         ("tail", int(t[L]), int(s[L]) + 2, FAR)]                      # beg inside the last row, an end beyond 2^31
    h = int(np.count_nonzero(t == 0))
    if 0 < h < n:                                                      # across the change of reference, from either side
        R += [("some", 0, int(s[h - 1]) + 1, FAR), ("some", 2, 0, int(e[h]) - 1), ("some", 0, 0, FAR), ("some", 2, 0, FAR)]
    return R


def _model(w, tid, beg, end):
    """(coverage rows, sample rows) the clip must give; the bounds as int64, so that an end beyond 2^31 compares as one"""
    return rf.clip_cov(w, tid, np.int64(beg), np.int64(end)), rf.clip_sample(w, tid, np.int64(beg), np.int64(end))


def _claimed(what, w, want, tid, beg):
    m = len(want["iv_tid"])
    if what == "none":
        assert m == 0
    elif what in ("one", "tail"):
        assert m == 1 and want["iv_start"][0] == beg
    elif what == "point":
        assert m == 1 and want["iv_start"][0] == want["iv_end"][0] == beg
    elif what == "not-k":
        assert np.any((w["iv_tid"] == tid) & (w["iv_end"] == beg)) and np.all(want["iv_end"] > beg)   # (kept, it would come out [beg, beg))
    else:
        assert m >= 1


def _place(w, keys, dev):
    import torch
    if not dev:
        return {k: w[k] for k in keys}
    return {k: torch.from_numpy(np.ascontiguousarray(w[k])).to("cuda:0") for k in keys}


def _np(d):
    from tiebrush_amd import api
    return api.to_numpy(d)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_clips_at_block_edges(ctx, n, dev):
    w = _rows(n)
    rows, srows = _place(w, COV_KEYS, dev), _place(w, SAMP_KEYS, dev)
    for what, tid, beg, end in _clip_regions(w):
        wc, ws = _model(w, tid, beg, end)
        _claimed(what, w, wc, tid, beg)
        cov, samp = _np(ctx.cov_clip(rows, tid, beg, end)), _np(ctx.sample_clip(srows, tid, beg, end))
        assert cov["n_intervals"] == len(wc["iv_tid"]) and cov["n_junctions"] == 0 and samp["n_sample"] == len(ws["s_tid"])
        _assert_rows(cov, wc, COV_KEYS, (what, tid, beg, end))
        _assert_rows(samp, ws, SAMP_KEYS, (what, tid, beg, end))
        if beg < end:                                                  # the table of that one interval: the same arrays
            _assert_rows(_np(ctx.cov_clip_regions(rows, [(tid, beg, end)])), cov, COV_KEYS, ("table", tid, beg, end))
            _assert_rows(_np(ctx.sample_clip_regions(srows, [(tid, beg, end)])), samp, SAMP_KEYS, ("table", tid, beg, end))
    assert np.array_equal(_np(rows)["iv_start"], w["iv_start"]) and np.array_equal(_np(srows)["s_end"], w["s_end"])   # (copied, not cut)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("pad", [0, 251])
def test_junction_rows_are_kept_whole_in_their_order(ctx, pad, dev):
    """junction rows are sorted inside a bundle only: the rows here are not sorted at all.  One that touches the region at either end
    is dropped, one that overlaps it by one base is kept whole; with `pad` rows outside the region in front the six lie across a block edge"""
    beg, end = 1000, 2000
    j = [(0, 1999, 2500, "+"), (0, 900, 1000, "-"), (0, 1200, 1300, "+"), (1, 1200, 1300, "+"), (0, 2000, 2100, "-"), (0, 900, 1001, "."),
         (0, 1100, 1150, "-")]
    j = [(0, 5000 + 3 * i, 5002 + 3 * i, "+") for i in range(pad)] + j
    w = _rows(4)
    w.update(j_tid=np.array([x[0] for x in j], dtype=np.int32), j_start=np.array([x[1] for x in j], dtype=np.int32),
             j_end=np.array([x[2] for x in j], dtype=np.int32), j_strand=np.array([ord(x[3]) for x in j], dtype=np.uint8),
             j_val=np.arange(len(j)) + 0.25)
    want, _ = _model(w, 0, beg, end)
    assert [int(v - 0.25) - pad for v in want["j_val"]] == [0, 2, 5, 6] and len(want["iv_tid"]) == 0
    rows = _place(w, COV_KEYS, dev)
    got = _np(ctx.cov_clip(rows, 0, beg, end))
    _assert_rows(got, want, COV_KEYS, "junctions")
    _assert_rows(_np(ctx.cov_clip_regions(rows, [(0, beg, end)])), got, COV_KEYS, "junctions, table")
    point = _np(ctx.cov_clip(rows, 0, 1250, 1250))                     # an empty region inside a junction row keeps it
    _assert_rows(point, _model(w, 0, 1250, 1250)[0], COV_KEYS, "junctions, empty region")
    assert [int(v - 0.25) - pad for v in point["j_val"]] == [2]


# ---- the view and the tile --------------------------------------------------------------------------------------------------------------
BEG, END, POINT = 1000, 2000, 1500
M50 = ((50, bc.M),)
NOREF = ((10, bc.S), (5, bc.I))                                        # reference length 0: the record ends at pos + 1
EDGES = [(950, M50), (951, M50),                                       # rec_end == beg (out), rec_end == beg + 1 (in)
         (999, NOREF), (1000, NOREF),                                  # the pos + 1 rule: ends at beg (out), starts at beg (in)
         (1300, ((10, bc.M), (100, bc.N), (10, bc.M))),
         (1450, M50), (1480, M50), (1500, M50),                        # ends at POINT, holds POINT inside, starts at POINT
         (1999, M50), (2000, M50)]                                     # pos == end - 1 (in), pos == end (out)


def _records(n):
    """n records in (tid, pos) order: the edge records on references 0 and 1 (n >= 255), short fillers in front of them on 0 and behind
    them on 1; reference 2 has none"""
    if n < 2:
        spec = [(0, 1480, M50)][:n]
    else:
        fill = n - 2 * len(EDGES)
        a = fill // 2
        spec = [(0, 10 + 3 * i, ((5, bc.M),)) for i in range(a)] + [(0, p, c) for p, c in EDGES] + [(1, p, c) for p, c in EDGES] + \
               [(1, 3000 + 7 * i, ((5, bc.M), (2, bc.D), (4, bc.M))) for i in range(fill - a)]
        assert spec == sorted(spec, key=lambda x: x[:2]) and 10 + 3 * a + 5 < 950
    return [bc.Rec(tid=t, pos=p, flag=16 * (i & 1), mapq=i % 200, cigar=c, name=b"r%d" % i) for i, (t, p, c) in enumerate(spec)]


class Crafted:
    def __init__(self, d, n):
        self.recs = _records(n)
        path = str(d / ("n%d.bam" % n))
        cr.write_bam(path, NAMES, LENS, [r.raw for r in self.recs])
        self.fx = rf.Fixture(path, kinds=())
        assert len(self.fx.recs) == n and [(r[0], r[1]) for r in self.fx.recs] == [(r.tid, r.pos) for r in self.recs]
        self.spans = self.fx.spans([(self.fx.recs[0][3], self.fx.vend)]) if n else []   # every record of the file

    def kept(self, tid, beg, end):
        """indices of the records the brute-force scan keeps"""
        at = {r[3]: i for i, r in enumerate(self.fx.recs)}
        return [at[r[3]] for r in self.fx.brute(tid, beg, end)]

    def columns(self, idx, fields):
        R = [self.recs[i] for i in idx]
        col = dict(tid=np.array([r.tid for r in R], dtype=np.int32), pos=np.array([r.pos for r in R], dtype=np.int32),
                   flag=np.array([r.flag for r in R], dtype=np.uint16), mapq=np.array([r.mapq for r in R], dtype=np.uint8),
                   cig=np.array([x for r in R for x in r.cig], dtype=np.uint32))
        return {k: col[k] for k in fields if k in col}, [len(r.cig) for r in R]


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_region_fold")
    return {n: Crafted(d, n) for n in SIZES}


VIEW_REGIONS = [(0, BEG, END), (1, BEG, END), (0, POINT, POINT), (1, POINT, POINT), (2, 0, 1000000), (0, BEG, FAR), (1, 0, BEG), (0, 0, FAR),
                (0, 951 + 49, 951 + 50), (1, END, END + 1)]


def test_the_edge_records_are_what_they_claim(crafted):
    c = crafted[257]
    pos = lambda tid, beg, end: [c.recs[i].pos for i in c.kept(tid, beg, end)]   # noqa: E731
    for tid in (0, 1):
        assert pos(tid, BEG, END) == [951, 1000, 1300, 1450, 1480, 1500, 1999]
        assert pos(tid, POINT, POINT) == [1480]
    assert pos(2, 0, 1000000) == [] and pos(0, 1000, 1001) == [951, 1000] and pos(1, END, END + 1) == [1999, 2000]
    assert crafted[1].kept(0, POINT, POINT) == [0] and crafted[0].kept(0, BEG, END) == []


def _same_columns(got, want, lens, what):
    for k, w in want.items():
        assert np.array_equal(got[k], w), (what, k)
    assert np.array_equal(got["cig_off"], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)), what


@pytest.mark.parametrize("n", SIZES)
def test_view_keeps_the_brute_force_records(ctx, crafted, n):
    c = crafted[n]
    tile, span_off, seen = ctx.bam_decode_spans(c.spans, len(LENS))    # (decoded once: a view does not consume the tile)
    assert int(tile.n_records) == n
    for region in VIEW_REGIONS:
        idx = c.kept(*region)
        want, lens = c.columns(idx, ("tid", "pos", "flag", "cig"))
        forms = [ctx.region_view(tile, seen, *region)] + ([ctx.regions_view(tile, seen, [region])] if region[1] < region[2] else [])
        for view in forms:
            assert view.n_records == len(idx) and view.n_cigar_ops == sum(lens), region
            if idx:
                _same_columns(_view_arrays(ctx, view), want, lens, region)


@pytest.mark.parametrize("n,m", list(zip(SIZES, SIZES[1:] + SIZES[:1])))
def test_tile_keeps_the_brute_force_records_of_two_files(ctx, crafted, n, m):
    a, b = crafted[n], crafted[m]
    fields = ("tid", "pos", "flag", "mapq", "cig_off", "cig")
    for region in VIEW_REGIONS:
        ia, ib = a.kept(*region), b.kept(*region)
        (wa, la), (wb, lb) = a.columns(ia, fields), b.columns(ib, fields)
        want = {k: np.concatenate([wa[k], wb[k]]) for k in wa}
        for table in (False, True)[:1 + (region[1] < region[2])]:
            tile, fo = ctx.bam_decode_file_spans([a.spans, b.spans], len(LENS))   # (decoded per call: the region tile consumes it)
            assert list(fo) == [0, n, n + m]
            out, fo2 = ctx.tile_regions(tile, [region]) if table else ctx.tile_region(tile, *region)
            assert int(out.n_records) == len(ia) + len(ib) and list(fo2) == [0, len(ia), len(ia) + len(ib)], (region, table)
            if ia or ib:
                _same_columns(ctx.soa_to_numpy(out, fields=fields), want, la + lb, (region, table))


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_rows_out_of_order_or_overlapping_are_refused(ctx, dev):
    """tbk.h: TBK_EINVAL for interval rows that are not sorted by (tid, start) and disjoint; nothing faults, the caller's arrays stay as
    they were, and the context takes the next call"""
    from tiebrush_amd import _lib
    good = _rows(257)
    rev = {k: (v[::-1].copy() if k[:2] != "j_" else v) for k, v in good.items()}
    lap = _rows(2)
    for k in ("iv", "s"):
        lap[k + "_tid"][:] = 0
        lap[k + "_start"][:] = (100, 150)
        lap[k + "_end"][:] = (200, 250)
    region = (0, 120, 5000)
    for bad in (rev, lap):
        rows, srows = _place(bad, COV_KEYS, dev), _place(bad, SAMP_KEYS, dev)
        for call, arg in ((ctx.cov_clip, rows), (ctx.sample_clip, srows)):
            with pytest.raises(_lib.TbkError) as e:
                call(arg, *region)
            assert e.value.status == -1
        for k in COV_KEYS:
            assert np.array_equal(_np(rows)[k], bad[k]), k
        for k in SAMP_KEYS:
            assert np.array_equal(_np(srows)[k], bad[k]), k
        wc, ws = _model(good, *region)
        assert len(wc["iv_tid"]) > 1
        _assert_rows(_np(ctx.cov_clip(_place(good, COV_KEYS, dev), *region)), wc, COV_KEYS, "after a refusal")
        _assert_rows(_np(ctx.sample_clip(_place(good, SAMP_KEYS, dev), *region)), ws, SAMP_KEYS, "after a refusal")


def test_an_empty_interval_is_a_region_but_not_a_table(ctx, crafted):
    """`-r` of a BEG behind the reference's end gives an empty region, which the one-region entries take; a caller's table has none"""
    from tiebrush_amd import _lib
    c = crafted[257]
    w = _rows(5)
    rows, srows = {k: w[k] for k in COV_KEYS}, {k: w[k] for k in SAMP_KEYS}
    empty = (0, 100, 100)

    def tile():
        return ctx.bam_decode_file_spans([c.spans], len(LENS))[0]

    tl, _, seen = ctx.bam_decode_spans(c.spans, len(LENS))
    for call in (lambda: ctx.regions_view(tl, seen, [empty]), lambda: ctx.tile_regions(tile(), [empty]),
                 lambda: ctx.cov_clip_regions(rows, [empty]), lambda: ctx.sample_clip_regions(srows, [empty])):
        with pytest.raises(_lib.TbkError) as e:
            call()
        assert e.value.status == -1
    tl, _, seen = ctx.bam_decode_spans(c.spans, len(LENS))
    assert ctx.region_view(tl, seen, *empty).n_records == len(c.kept(*empty))
    out, fo = ctx.tile_region(tile(), *empty)
    assert int(out.n_records) == len(c.kept(*empty)) and list(fo) == [0, int(out.n_records)]
    wc, ws = _model(w, *empty)
    assert len(wc["iv_tid"]) == 0                                      # (the first row starts at 100: it does not hold the point inside)
    _assert_rows(ctx.cov_clip(rows, *empty), wc, COV_KEYS, empty)
    _assert_rows(ctx.sample_clip(srows, *empty), ws, SAMP_KEYS, empty)
