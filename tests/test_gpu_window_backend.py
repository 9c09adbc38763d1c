"""The back end of the raw window form (wgroup.hip), between the last tier kernel and the YD stage: the compaction wave that also
verifies its window's listed records (those whose key word is hashed), the identity order it leaves in gperm / ginv, and wg_tie_k
(label col_tie_sets), which sorts the tie sets of several groups and rewrites their members alone.  Every case runs on small tiles
forced onto the raw window form, is compared with the oracle, and is run a second time on the same context under wg_back=split —
the sequence of separate passes (wg_finish, col_tie_sort, col_write, the scan of the incidence counts) — with identical results.

Where the windows lie: one file, so record 1024 j opens a window when its key differs from the key before it (test_gpu_handover.py);
every record is a group of its own unless said otherwise, so a group's lane in its window's wave is its record's offset there."""
import functools

import numpy as np
import pytest

import window_scenes as ws
from helpers import tbk_debug
from helpers import tile_from_records as _tile

pytestmark = pytest.mark.gpu

M, I, D, N, S = 0, 1, 2, 3, 4
GROUP_KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end")
SNUM = {"cigar": 0, "full": 1, "clip": 2, "exon": 3}
BACK = ("wg_finish", "col_tie_sort", "col_write")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def raw_window(monkeypatch):
    tbk_debug(monkeypatch, path="window", raw=1)


def _oracle(tile, **kw):
    from oracle import oracle_ffi as orc
    okw = dict(kw)
    okw["strategy"] = SNUM[okw.get("strategy", "cigar")]
    return orc.collapse(tile, want_rec_group=True, **okw)


def _ab(ctx, monkeypatch, tile, rec_group=False, want=None, **kw):
    """the fused back end, then wg_back=split on the same context: both equal the oracle (so each other); returns the kernels of both"""
    from tiebrush_amd import api
    want = _oracle(tile, **kw) if want is None else want
    keys = GROUP_KEYS + (("rec_group",) if rec_group else ())
    ran = {}
    for back in ("fused", "split"):
        tbk_debug(monkeypatch, wg_back=back)
        got = api.to_numpy(ctx.collapse(api.to_device(tile, "cuda:0"), want_rec_group=rec_group, **kw))
        ran[back] = ctx.kernel_times()
        assert ctx.collapse_route()["form"] == "raw" and ctx.collapse_route()["reseeds"] == 0
        assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
        for k in keys:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (back, k)
    tbk_debug(monkeypatch, wg_back=None)
    assert "wg_compact" in ran["fused"] and "wg_compact" in ran["split"]
    assert "col_tie_sets" in ran["fused"] and "col_tie_sort" not in ran["fused"], ran["fused"]
    assert "col_tie_sort" in ran["split"] and "col_write" in ran["split"] and "col_tie_sets" not in ran["split"], ran["split"]
    return ran


# ---- tie sets ------------------------------------------------------------------------------------------------------------------------
# members of a tie set: equal (tid, start, strand, end), different CIGARs — a M b D c M of span 40, two hundred of them (hashed key words)
SHAPES = [[(a, M), (b, D), (40 - a - b, M)] for a in range(1, 21) for b in range(1, 11)]
N_LINE = 3 * 1024 + 500    # windows open at records 1024, 2048 and 3072


def _line(n, ties, first_pos=100):
    """one file of n reads 40M on distinct starts, except that the records at the indices in `ties` (tuples of consecutive indices)
    share the start of the tuple's first record; member j takes SHAPES[(7 j + 3) % 200], so a set's key order is not its output order"""
    recs = [(0, first_pos + 3 * i, 0, 60, "+", 1, [(40, M)]) for i in range(n)]
    for t in ties:
        for j, i in enumerate(t):
            recs[i] = (0, first_pos + 3 * t[0], 0, 60, "+", 1, SHAPES[(7 * j + 3) % len(SHAPES)])
    return recs


def _run(a, n):
    return tuple(range(a, a + n))


TIE_PLACES = {
    "sets-of-2-3-70": [_run(40, 2), _run(300, 3), _run(1024 + 76, 70), _run(2048 + 30, 70)],        # 70: lanes 76 .. 145, 30 .. 99
    "second-member-is-lane-0": [(63, 64), (1024 + 127, 1024 + 128), _run(2048 + 191, 3)],           # the head is the carried lane 63
    "first-and-last-groups-of-a-window": [(0, 1), (1022, 1023), (1024, 1025), _run(2045, 3), _run(2048, 3), (N_LINE - 2, N_LINE - 1)],
    "head-is-lane-0": [(64, 65), (1024 + 128, 1024 + 129)],                                         # the group before it: LONG (below)
    "no-set": [],
}
# The group in lane 63 ahead of a set whose head is lane 0 of the next round: five CIGAR operations on a start of its own, which the
# reference comparator puts BEHIND the set's members (fewer operations first) — were the head's flag taken from lane 63 without a look
# at the carried key, that group would join the set and leave its place
LONG = [(10, M), (5, N), (10, M), (5, N), (10, M)]
LONG_AT = {"head-is-lane-0": [63, 1024 + 127]}


def _pileup_files():
    """2100 reads on one base put three splitters on one key: a window of the pile-up's own, with tie sets of many groups among other
    spans; sets on the last two groups of the window before it and on the first two of the window behind it"""
    pre = _line(1000, [(998, 999)])
    p = 100 + 3 * 1000
    pile = [(0, p, 0, 60, "+", 1, SHAPES[i % 90] if i % 5 else [(20 + 5 * (i % 3), M)]) for i in range(2100)]
    post = _line(500, [(0, 1)], first_pos=p + 1)
    return [pre + pile + post]


def _all_tie_files():
    """every group of the tile in one tie set: one window, 200 groups of three records"""
    return [[(0, 700, 0, 60, "-", 1, c) for c in SHAPES for _ in range(3)]]


@functools.lru_cache(maxsize=None)
def _tie_scene(place, k=1):
    """the tile of a place, its records dealt round-robin to k files, and the oracle's result: built once, shared, never written"""
    if place == "pile-up":
        recs = _pileup_files()[0]
    elif place == "every-group":
        recs = _all_tie_files()[0]
    else:
        recs = _line(N_LINE, TIE_PLACES[place])
        for i in LONG_AT.get(place, []):
            recs[i] = recs[i][:6] + (LONG,)
    tile = _tile([recs[f::k] for f in range(k)])
    return tile, _oracle(tile)


ALL_PLACES = list(TIE_PLACES) + ["pile-up", "every-group"]


@pytest.mark.parametrize("place", ALL_PLACES)
def test_tie_sets(ctx, monkeypatch, place):
    """64 files at most and no record -> group map: the files travel as masks, there is no incidence and no inverse — the fused back end
    runs one scan less than the split one (the scan of the windows' incidence counts, all zero)"""
    tile, want = _tie_scene(place)
    ran = _ab(ctx, monkeypatch, tile, want=want)
    scans = {b: sum(v[1] for k, v in ran[b].items() if k.startswith("scan_")) for b in ran}
    assert scans["split"] > scans["fused"], scans
    assert "col_write" not in ran["fused"]


@pytest.mark.parametrize("place", ALL_PLACES)
def test_tie_sets_with_record_group_map(ctx, monkeypatch, place):
    """the record -> group map goes through ginv: the compaction's identity and the tie kernel's inverse of every set"""
    tile, want = _tie_scene(place)
    _ab(ctx, monkeypatch, tile, rec_group=True, want=want)


@pytest.mark.parametrize("place", ALL_PLACES)
def test_tie_sets_with_65_files(ctx, monkeypatch, place):
    """one file more than a mask holds: incidence lists, pbase is live (the second scan runs in both forms), the YD items are not placed
    by list and read ginv"""
    tile, want = _tie_scene(place, 65)
    ran = _ab(ctx, monkeypatch, tile, want=want)
    scans = {b: sum(v[1] for k, v in ran[b].items() if k.startswith("scan_")) for b in ran}
    assert scans["split"] == scans["fused"], scans


# ---- verification --------------------------------------------------------------------------------------------------------------------
HASHED = [(20, M), (2, I), (20, M)]                                  # an insertion: no exact key word
PAIR_A = [(10, M), (20, N), (10, M), (30, N), (10, M)]               # the pair of window_scenes.py: only the inner exon differs
PAIR_B = [(10, M), (30, N), (10, M), (20, N), (10, M)]
N_VER = 2 * 1024 + 500                                               # three windows: the keys of records 1024 and 2048 open two


def _verify_tile(pair_in=None, cross=False):
    """The plain reads (50M) lie three to a start, so a full window holds some 350 groups and stays in the first group table (573
    groups; a window the LDS sort takes is verified there as well, and would hide what the list's walk misses).  Window 0 holds no
    hashed record; window 1 exactly 64 listed entries (records 1100 .. 1163), window 2 exactly 65 (2101 .. 2165): identical hashed reads
    two to a start, so that half of the entries are compared with another record, and one alone.
    pair_in = 1 | 2: the last two paired entries of that window are PAIR_A and PAIR_B on one start (two groups; one key once the hash
    is masked away).  cross: PAIR_A is an entry of window 1 and PAIR_B one of window 2, each on a start of its own"""
    recs = [(0, 100 + 3 * (i - i % 3), 0, 60, "+", 1, [(50, M)]) for i in range(N_VER)]

    def put(i, cig, at=None):
        recs[i] = (0, 100 + 3 * (i if at is None else at), 0, 60, "+", 1, cig)

    for first, n in ((1100, 64), (2101, 65)):
        for i in range(first, first + n):
            put(i, HASHED, at=first + 2 * ((i - first) // 2))
    if pair_in:
        i = {1: 1162, 2: 2163}[pair_in]
        put(i, PAIR_A)
        put(i + 1, PAIR_B, at=i)
    if cross:
        put(1163, PAIR_A)
        put(2165, PAIR_B)
    pos = [r[1] for r in recs]
    assert pos == sorted(pos)
    return _tile([recs])


@pytest.mark.parametrize("what", ["plain", "cross"])
def test_verification_passes_at_the_round_edge(ctx, monkeypatch, what):
    """0, 64 and 65 listed entries: one round of the wave, and one entry in a second round.  With every hash bit masked away all hashed
    key words are equal, and still nothing is flagged: true repeats compare equal, and a pair whose members lie in different windows
    (different starts) never meets"""
    tile = _verify_tile(cross=what == "cross")
    want = _oracle(tile)
    ran = _ab(ctx, monkeypatch, tile, want=want)
    assert not any(k in ran["fused"] for k in BACK), ran["fused"]
    assert all(k in ran["split"] for k in BACK), ran["split"]
    tbk_debug(monkeypatch, hash_mask="0")
    _ab(ctx, monkeypatch, tile, want=want)


def _refused(ctx, monkeypatch, tile):
    from tiebrush_amd import api
    dev = api.to_device(tile, "cuda:0")
    for back in ("fused", "split"):
        tbk_debug(monkeypatch, wg_back=back, hash_mask="0")
        with pytest.raises(api.TbkError) as e:
            ctx.collapse(dev)
        assert e.value.status == -8, back                              # TBK_ECOLLISION
        r = ctx.collapse_route()
        assert r["form"] == "none" and r["reseeds"] == 4, (back, r)
    tbk_debug(monkeypatch, wg_back=None, hash_mask=None)


@pytest.mark.parametrize("pair_in", [1, 2])
def test_collision_among_64_and_65_entries(ctx, monkeypatch, pair_in):
    """the colliding pair among the 64 entries of one round / the 65 of two: the oracle's result (a tie set of two) with the hash, a
    reseed per seed and TBK_ECOLLISION with the mask on every seed"""
    tile = _verify_tile(pair_in=pair_in)
    _ab(ctx, monkeypatch, tile)
    _refused(ctx, monkeypatch, tile)


@pytest.mark.parametrize("name", ["collision-tier1", "collision-tier2", "collision-lds-sort", "collision-pileup"])
def test_collision_in_one_window_of_each_tier(ctx, monkeypatch, name):
    """window_scenes.py's pair in a window of the first table, the second table, the LDS sort and a pile-up"""
    tile = ws.get(name).tile
    _ab(ctx, monkeypatch, tile, want=ws.oracle(name))
    _refused(ctx, monkeypatch, tile)


# ---- kernels that ran ----------------------------------------------------------------------------------------------------------------
def test_kernels_of_the_back_end(ctx, monkeypatch):
    from tiebrush_amd import api
    tile, want = _tie_scene("sets-of-2-3-70")
    ran = _ab(ctx, monkeypatch, tile, want=want)
    assert "wg_compact" in ran["fused"] and not any(k in ran["fused"] for k in BACK), ran["fused"]
    assert all(k in ran["split"] for k in ("wg_compact",) + BACK), ran["split"]
    tbk_debug(monkeypatch, wg_dense_verify="1")                      # the per-record form keeps its kernel
    ctx.collapse(api.to_device(tile, "cuda:0"))
    dense = ctx.kernel_times()
    assert "wg_finish" in dense and "wg_compact" in dense and "col_tie_sets" in dense, dense
