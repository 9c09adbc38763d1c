"""The hand-over of the collapsed groups inside the window path (wgroup.hip): the tie flags wg_compact_k writes beside the keys, and
the windows' record bases wg_offsets_transpose_k sums on its way through the offsets matrix (at most 64 input files; more: wg_rowsum_k).
Every case runs on small tiles forced onto the window path (TBK_PATH=window) and is compared with the oracle: the seven group arrays,
then — through the device chain — the intervals and the junctions.

Where the windows lie: with k input files the partition samples every s-th record of the files laid end to end (s the largest
power of two with k s <= 2048, at most 1024) and every g-th sorted sample (g = 1024 / s) is a splitter; a splitter owns two bounds,
so the offsets matrix has nrows = 2 nsp + 2 rows (always even).  One file: s = 1024, g = 1 — record 1024 j opens a window of its own
when its key differs from the key before it, and three splitters in a row on one key give that key a window [v, v + 1)."""
import numpy as np
import pytest

from helpers import tbk_debug
from helpers import tile_from_records as _tile

pytestmark = pytest.mark.gpu

M, I, D, N, S = 0, 1, 2, 3, 4
GROUP_KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end", "rec_group")
COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
SNUM = {"cigar": 0, "full": 1, "clip": 2, "exon": 3}


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


@pytest.fixture(params=["1", "0"], ids=["raw", "compacted"])
def window_mode(request, monkeypatch):
    tbk_debug(monkeypatch, path="window", raw=request.param)
    return request.param


def _check(ctx, tile, want=None, keys=GROUP_KEYS, **kw):
    """collapse on the window path, then the device chain into tiecov: groups, intervals and junctions against the oracle; returns
    the names of the kernels the collapse ran"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, synth
    if want is None:
        okw = dict(kw)
        okw["strategy"] = SNUM[okw.get("strategy", "cigar")]
        want = orc.collapse(tile, want_rec_group=True, **okw)
    res = ctx.collapse(api.to_device(tile, "cuda:0"), want_rec_group=True, **kw)
    ran = set(ctx.kernel_times())
    got = api.to_numpy(res)
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    cw = orc.coverage(synth.collapsed_to_cov_input(tile, want))
    cg = api.to_numpy(ctx.coverage(ctx.groups_to_cov_in(res)))
    for k in COV_KEYS:
        assert np.array_equal(cg[k], cw[k]), k
    assert "wg_compact" in ran and "wg_tie" not in ran, ran    # the window path ran, and the flags came with the compaction
    return ran


# ---- A. tie flags ------------------------------------------------------------------------------------------------------------------
# members of a tie set: equal (tid, start, strand, end), different CIGARs (span 10 each)
TIE = [[(10, M)], [(4, M), (2, D), (4, M)], [(3, M), (4, D), (3, M)]]


def _line(n, ties, first_pos=100):
    """one file of n reads 10M on distinct starts (3 apart: neighbours overlap, one bundle), except that the records at the indices
    in `ties` (tuples of consecutive record indices) share the start of the tuple's first record and take the CIGARs of TIE"""
    recs = [(0, first_pos + 3 * i, 0, 60, "+", 1, TIE[0]) for i in range(n)]
    for t in ties:
        for j, i in enumerate(t):
            recs[i] = (0, first_pos + 3 * t[0], 0, 60, "+", 1, TIE[j])
    return recs


N_LINE = 3 * 1024 + 500    # one file: windows open at records 1024, 2048 and 3072

TIE_PLACES = {
    "first-two-of-a-window": [(1024, 1025), (2048, 2049)],
    "last-two-of-a-window": [(1022, 1023), (2046, 2047), (N_LINE - 2, N_LINE - 1)],
    "lanes-63-and-64": [(63, 64), (1024 + 63, 1024 + 64), (2048 + 127, 2048 + 128)],
    "three-in-a-set": [(1500, 1501, 1502), (1024 + 62, 1024 + 63, 1024 + 64), (2046, 2047, 2048)],
    "first-groups-of-the-tile": [(0, 1)],
    "no-tie": [],
}


@pytest.mark.parametrize("place", list(TIE_PLACES))
def test_tie_sets_at_window_and_lane_edges(ctx, window_mode, place):
    """every record is a group of its own, so a group's lane in wg_compact_k is its record's offset in the window: tie sets on a
    window's first and last groups, across lanes 63 / 64 (the carry from one round of 64 groups to the next), of three groups — the
    third of (2046, 2047, 2048) sits on the record that is sampled, which then shares the window of the other two —, and none at all"""
    _check(ctx, _tile([_line(N_LINE, TIE_PLACES[place])]))


def test_tie_sets_around_a_pileup_window(ctx, window_mode):
    """2100 reads on one base put three splitters on one key: bounds v and v + 1, a window of the pile-up's own.  Tie sets lie on the last
    two groups of the window before it, on its own first groups (three members, among other spans) and on the first two groups of
    the window behind it"""
    pre = _line(1000, [(998, 999)])
    p = 100 + 3 * 1000
    pile = []
    for i in range(2100):
        pile.append((0, p, 0, 60, "+", 1, TIE[i % 3] if i % 5 else [(20 + 5 * (i % 3), M)]))
    post = _line(500, [(0, 1)], first_pos=p + 1)
    _check(ctx, _tile([pre + pile + post]))
    # the same with the pile-up spread over three files (every file brings a piece of each window)
    files = [[], [], []]
    for i, r in enumerate(pre + pile + post):
        files[i % 3].append(r)
    _check(ctx, _tile(files))


def _all_tie_records():
    """200 alignments a M b D c M of span 40 on one start and strand, each three times: one window, every group in one tie set"""
    shapes = [[(a, M), (b, D), (40 - a - b, M)] for a in range(1, 21) for b in range(1, 11)]
    return [(0, 700, 0, 60, "-", 1, c) for c in shapes for _ in range(3)]


def test_every_group_of_the_tile_in_one_tie_set(ctx, window_mode):
    recs = _all_tie_records()
    _check(ctx, _tile([recs]))
    _check(ctx, _tile([recs[0::2], recs[1::2]]), strategy="clip")


def test_tie_sets_of_group_partials(ctx, monkeypatch):
    """group partials of other ranks (every file TieBrush-merged, explicit priorities, carried YC / YX / YD) take the same compaction
    kernel in its PART form"""
    from dist_helpers import OracleCompute
    tbk_debug(monkeypatch, path="window")
    line = _line(N_LINE, sum(TIE_PLACES.values(), []))
    files = [[], [], []]
    for i, r in enumerate(line + _all_tie_records()):
        files[i % 3].append(r)
    for f in files:
        f.sort(key=lambda r: (r[0], r[1]))
    tile = _tile(files)
    n = tile.n_records
    rng = np.random.default_rng(31)
    tile.tbmerged = np.ones(3, np.uint8)
    tile.yc_in = rng.integers(1, 9, n).astype(np.float64)
    tile.yx_in = rng.integers(1, 4, n).astype(np.int64)
    tile.yd_in = rng.integers(0, 50, n).astype(np.int64)
    tile.prio_hi = rng.integers(0, 1000, n).astype(np.uint64)
    tile.prio_lo = np.arange(n).astype(np.uint64)
    want = OracleCompute().collapse(tile, strategy="clip")
    _check(ctx, tile, want=want, strategy="clip")


# ---- B. window bases ---------------------------------------------------------------------------------------------------------------
def _nrows(m, k):
    """rows of the offsets matrix for m records in k files (tbk_window_groups)"""
    s = 1
    while s * 2 * k <= 2048 and s * 2 <= 1024:
        s *= 2
    g = 1024 // s
    ns = -(-m // s)
    nsp = (ns - 1) // g if ns > 1 else 0
    return 2 * nsp + 2


def _files_tile(rng, m, k, empty, last):
    """m reads in k sorted files; file `empty` holds nothing, the reads of file `last` (40 of them) all lie on the highest start of
    the tile — in the last window that holds records"""
    from tiebrush_amd import soa
    span = 40 * m
    n_last = 40 if last is not None else 0
    normal = [f for f in range(k) if f != empty and f != last]
    fo = rng.choice(normal, m - n_last)
    pos = rng.integers(0, span, m - n_last)
    if last is not None:
        fo = np.concatenate([fo, np.full(n_last, last)])
        pos = np.concatenate([pos, np.full(n_last, span + 100)])
    order = np.lexsort((pos, fo))
    fo, pos = fo[order], pos[order].astype(np.int32)
    file_off = np.zeros(k + 1, np.uint32)
    file_off[1:] = np.cumsum(np.bincount(fo, minlength=k))
    spliced = rng.random(m) < 0.1
    ncig = np.where(spliced, 3, 1)
    cig_off = np.zeros(m + 1, np.uint32)
    cig_off[1:] = np.cumsum(ncig)
    cig = np.empty(int(cig_off[-1]), np.uint32)
    first = cig_off[:-1].astype(np.int64)
    cig[first] = (np.where(spliced, 20, 50) << 4) | M
    cig[first[spliced] + 1] = (rng.integers(30, 200, int(spliced.sum())) << 4) | N
    cig[first[spliced] + 2] = (30 << 4) | M
    return soa.SoATile(n_files=k, file_off=file_off, tbmerged=np.zeros(k, np.uint8), tid=np.zeros(m, np.int32), pos=pos,
                       flag=np.zeros(m, np.uint16), mapq=np.full(m, 60, np.uint8), strand=rng.choice(np.frombuffer(b"+-", np.uint8), m),
                       nh=np.ones(m, np.int32), cig_off=cig_off, cig=cig)


# nrows is even by construction (two bounds per splitter): one row block of the transpose exactly full (64), one row and one block
# beyond it (66, 130) stand for the odd counts 65 and 129, which no input produces
@pytest.mark.parametrize("nrows", [2, 64, 66, 130])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65])
def test_window_bases_from_the_transpose(ctx, window_mode, k, nrows):
    """k <= 64: the transpose's blocks hold whole rows and leave the windows' record bases (no wg_rowsum launch); k = 65: two block
    columns, wg_rowsum_k stays.  Row counts at the edges of the 64-row blocks; an empty file and a file that lies in the last window"""
    m = 1024 * ((nrows - 2) // 2) + 1000
    assert _nrows(m, k) == nrows
    rng = np.random.default_rng(1000 * k + nrows)
    shapes = [(None, None)] if k == 1 else ([(1, None), (None, 1), (None, 0)] if k == 2 else [(k // 2, k - 1), (0, 1)])
    for empty, last in shapes:
        ran = _check(ctx, _files_tile(rng, m, k, empty, last))
        assert ("wg_rowsum" in ran) == (k > 64), ran
        assert "wg_offsets_transpose" in ran


# ---- C. the view builder's two passes and tiecov's tile aggregates -------------------------------------------------------------------
TILE = 4096                                     # groups per block of the view builder's passes = records per tile of tiecov's bundle passes
FAR = [[(5, M), (1, I), (5, M)], [(3, S), (20, M)], [(5, M), (20, N), (5, M), (20, N), (5, M), (20, N), (5, M)]]
VIEW_KEYS = ("tid", "pos", "cig_off", "cig", "yc", "strand", "yx")


def _view_records(ng, edge):
    """ng reads, each a group of its own, group index = record index: 30M five bases apart (one bundle), every 7th an M N M, every
    11th / 13th / 17th a shape the key cannot describe (insertion, soft clip under the default strategy, four exons); far shapes on
    the last group of the first tile and the first group of the second.  `edge`: what happens at group 4096 —
    overlap: the bundle goes on across the tile boundary; ends: it ends with group 4095 (a gap); ref: the reference changes there;
    mixed: the reference changes inside the first tile, so the second tile lies on one reference behind a tile that does not"""
    recs = []
    for i in range(ng):
        cig = [(30, M)]
        if i % 7 == 3:
            cig = [(10, M), (50, N), (10, M)]
        for q, every in enumerate((11, 13, 17)):
            if i % every == every - 1:
                cig = FAR[q]
        if i == TILE - 1:
            cig = FAR[0]
        if i == TILE:
            cig = FAR[2]
        tid, pos = 0, 1000 + 5 * i
        if edge == "ends" and i >= TILE:
            pos += 10000
        if edge == "ref" and i >= TILE:
            tid, pos = 1, 50 + 5 * (i - TILE)
        if edge == "mixed" and i >= 2000:
            tid, pos = 1, 50 + 5 * (i - 2000)
        recs.append((tid, pos, 0, 60, "+-."[i % 3], 1, cig))
    return recs


def _grab(ptr, count, dt):
    """a copy of `count` elements of context-owned device memory (device to device)"""
    import ctypes as C
    import torch
    hip = C.CDLL("libamdhip64.so")
    t = torch.empty(max(count, 1), dtype=dt, device="cuda:0")
    if count:
        assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(count * t.element_size()), 3) == 0
    torch.cuda.synchronize()
    return t[:count]


@pytest.mark.parametrize("ng,edge", [(1, "overlap"), (TILE - 1, "overlap"), (TILE, "overlap"), (TILE + 1, "overlap"), (2 * TILE + 3, "overlap"),
                                     (TILE + 1, "ends"), (2 * TILE + 3, "ends"), (TILE + 1, "ref"), (2 * TILE + 3, "ref"),
                                     (TILE + 1, "mixed"), (2 * TILE + 3, "mixed")])
def test_view_from_keys_with_tile_aggregates(ctx, monkeypatch, ng, edge):
    """groups_to_cov_in into coverage: the view's arrays are the numpy gather of the representatives; the intervals and junctions are
    the oracle's on the view as built (the bundle passes start from the builder's tile aggregates: one cov_bundles launch), with
    TBK_COV_PREP and on a caller's copy of the view (cb_agg_k runs: two launches) — three identical results"""
    import torch
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, soa, synth
    tile = _tile([_view_records(ng, edge)])
    want = orc.collapse(tile, want_rec_group=True)
    assert want["n_groups"] == ng
    cw = orc.coverage(synth.collapsed_to_cov_input(tile, want))
    res = ctx.collapse(api.to_device(tile, "cuda:0"), want_rec_group=True)
    got = api.to_numpy(res)
    for k in GROUP_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    view = ctx.groups_to_cov_in(res)
    ran = set(ctx.kernel_times())
    assert ran == {"g2c_count", "g2c_gather"}, ran             # two kernels, no scan between them
    s = view.struct
    nc = view.n_cigar_ops
    copy = soa.CovInput(tid=_grab(s.tid, ng, torch.int32), pos=_grab(s.pos, ng, torch.int32), flag=None,
                        cig_off=_grab(s.cig_off, ng + 1, torch.int32), cig=_grab(s.cig, nc, torch.int32), yc=_grab(s.yc, ng, torch.float64),
                        strand=_grab(s.strand, ng, torch.uint8), yx=_grab(s.yx, ng, torch.int64))
    ref = synth.collapsed_to_cov_input(tile, want)
    for k in VIEW_KEYS:
        a = getattr(copy, k).cpu().numpy()
        b = np.asarray(getattr(ref, k))
        assert np.array_equal(a.view(b.dtype) if a.dtype.itemsize == b.dtype.itemsize else a, b), k
    covs, launches = {}, {}

    def run(name, cin):
        covs[name] = api.to_numpy(ctx.coverage(cin))
        launches[name] = ctx.kernel_times()["cov_bundles"][1]

    run("view", view)
    tbk_debug(monkeypatch, cov_prep="1")
    run("prep", view)
    tbk_debug(monkeypatch, cov_prep=None)
    run("copy", copy)
    assert launches == {"view": 1, "prep": 2, "copy": 2}, launches
    for name, c in covs.items():
        for k in COV_KEYS:
            assert np.array_equal(c[k], cw[k]), (name, k)
        for k in ("n_bases", "n_intervals", "n_junctions", "span_bases"):
            assert c[k] == cw[k], (name, k)
