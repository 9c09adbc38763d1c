"""The window path of the collapse stage (wgroup.hip) on hand-built tiles that sit on its edges (window_scenes.py): the thresholds of
its two group tables and of the LDS sort, pile-ups beyond them, its worklist loops, the shortcuts of its partition, the carries of
its effective-end scan, its collision checks.  Every scene runs under path=window in four forms — raw with the sparse verification
list (what a plain tiebrush run uses), raw with the record -> group map, compacted (raw=0), raw with the per-record verification
marks (wg_dense_verify=1) — and must equal the oracle exactly; the route it took (tbk_last_route under wg_stats=1) must equal what
the CPU model (window_model.py) predicts, so a scene that no longer reaches its edge fails here and in test_window_model_cpu.py."""
import numpy as np
import pytest

import window_model as wm
import window_scenes as ws
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

FORMS = ["raw-sparse", "raw-recgroup", "compacted", "raw-dense-verify"]
KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _set_form(monkeypatch, form, **more):
    tbk_debug(monkeypatch, path="window", wg_stats="1", raw="0" if form == "compacted" else "1", **more)
    if form == "raw-dense-verify":
        tbk_debug(monkeypatch, wg_dense_verify="1")


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    _set_form(monkeypatch, request.param)
    return request.param


def _equal(got, want, rec_group):
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in KEYS + (("rec_group",) if rec_group else ()):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def _collapse(ctx, tile, form, **opts):
    from tiebrush_amd import api
    rec = form in ("raw-recgroup", "compacted")
    return api.to_numpy(ctx.collapse(tile, want_rec_group=rec, **opts)), rec


def _check_route(route, tile, want, form, opts, handed_back=False):
    """the readout against the model: the window attempt whose counts it holds is the compacted one after a hand-back"""
    assert route["reseeds"] == 0 and route["raw_handed_back"] == handed_back
    if tile.n_files > wm.WINDOW_MAX_FILES:
        assert route["form"] == "sort" and "nw" not in route and not route["big_bucket"]
        return None
    raw = form != "compacted" and not handed_back
    p = wm.predict(tile, raw, want["rec_group"], **{k: v for k, v in opts.items() if k != "strategy"})
    assert {k: route[k] for k in ("nw", "nw_live", "ovf1", "ovf2")} == {k: p[k] for k in ("nw", "nw_live", "ovf1", "ovf2")}, (route, form)
    assert route["big_bucket"] == p["big_bucket"]
    assert route["form"] == ("sort" if p["big_bucket"] else "raw" if raw else "compacted"), route
    return p


def _run(ctx, name, form):
    s, want = ws.get(name), ws.oracle(name)
    got, rec = _collapse(ctx, s.tile, form, **s.opts)
    route = ctx.collapse_route()
    _equal(got, want, rec)
    return _check_route(route, s.tile, want, form, s.opts)


@pytest.mark.parametrize("name", ws.TIER_SCENES + ["tier-k1025"])
def test_tiers_one_window(ctx, form, name):
    """exactly thr1, thr1 + 1, thr2, thr2 + 1 groups in one window: first table, second table, second table, LDS sort; k = 32 -> 33 adds a
    word of sample bits, 64 -> 65 leaves the compile-time table, 1024 ranks by the merge sort, 1025 is the sort path"""
    _run(ctx, name, form)


@pytest.mark.parametrize("name", ws.PILEUP_SCENES)
def test_tiers_pile_up(ctx, form, name):
    """the same four counts as distinct CIGARs of one base with more than 4096 records: the last one is TBK_DERR_BIGBUCKET and the sort path"""
    p = _run(ctx, name, form)
    if name.endswith("thr2+1") and (ws.get(name).edge["mode"] == "raw") == (form != "compacted"):
        assert p["big_bucket"]


@pytest.mark.parametrize("name", ["largest-sortable-window", "worklist-tier2", "worklist-sort"])
def test_lds_sort_and_worklists(ctx, form, name):
    """a window of 2977 records in the LDS sort; 577 windows for the 512 blocks of the second tier; 1300 for the 1024 of the sort"""
    _run(ctx, name, form)


PARTITION = ws.RUN_SCENES + ["tid-change-at-chunk-edges", "400-files-of-5", "dense-64-files", "dense-96-files", "unplaced-tail", "extreme-coordinates"]


@pytest.mark.parametrize("name", PARTITION + ws.PILE_SCENES + ["effective-ends"])
def test_partition_and_effective_ends(ctx, form, name):
    _run(ctx, name, form)


@pytest.mark.parametrize("name", PARTITION + ws.PILE_SCENES)
@pytest.mark.parametrize("og_form", ["raw-sparse", "compacted"])
def test_partition_with_eight_chunk_blocks(ctx, monkeypatch, og_form, name):
    """tiles of this size run the offsets pass with one chunk per block; wg_og=8 gives them the blocks of eight chunks that tiles of 32 M
    records get: segments continued from the chunk before, the 256 probes fetched ahead, the search where a chunk spans more"""
    _set_form(monkeypatch, og_form, wg_og="8")
    _run(ctx, name, og_form)


@pytest.mark.parametrize("og", ["1", "8"])
@pytest.mark.parametrize("what", ["tid", "pos-chunk-edge", "pos-block-edge"])
def test_hidden_inversions(ctx, monkeypatch, form, what, og):
    """an inversion the partition's shortcuts do not see (a chunk whose ends agree) or see with the key before the chunk taken from the
    carried state / from memory: with a passing record TBK_EUNSORTED, among filtered ones the oracle's result; the raw form hands the
    tile back either way"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api
    _set_form(monkeypatch, form, wg_og=og)
    make = {"tid": ws.hidden_tid_inversion, "pos-chunk-edge": lambda f: ws.pos_inversion(wm.WG_OC, f),
            "pos-block-edge": lambda f: ws.pos_inversion(wm.WG_OG * wm.WG_OC, f)}[what]
    raw = form != "compacted"
    with pytest.raises(api.TbkError) as e:
        ctx.collapse(make(False))
    assert e.value.status == -6                                     # TBK_EUNSORTED
    r = ctx.collapse_route()
    assert r["form"] == "none" and r["raw_handed_back"] == raw and not r["big_bucket"]
    tile = make(True)
    want = orc.collapse(tile, want_rec_group=True)
    got, rec = _collapse(ctx, tile, form)
    route = ctx.collapse_route()
    _equal(got, want, rec)
    _check_route(route, tile, want, form, {}, handed_back=raw)


@pytest.mark.parametrize("name", list(ws.COLLISION_SCENES))
def test_collisions_are_refused(ctx, monkeypatch, form, name):
    """two alignments that differ only in the inner exon, every seed's hash masked away: TBK_ECOLLISION from every tier's verification,
    never a result; with the mask lifted the same context gives the oracle's result"""
    from tiebrush_amd import api
    s = ws.get(name)
    tbk_debug(monkeypatch, hash_mask="0")
    with pytest.raises(api.TbkError) as e:
        _collapse(ctx, s.tile, form)
    assert e.value.status == -8                                     # TBK_ECOLLISION
    r = ctx.collapse_route()
    assert r["form"] == "none" and r["reseeds"] == 4
    tbk_debug(monkeypatch, hash_mask=None)
    _run(ctx, name, form)


@pytest.mark.parametrize("seed", range(4))
def test_reseeds_are_counted(ctx, monkeypatch, form, seed):
    """twelve hash bits on a few thousand three-exon reads: the oracle's result or TBK_ECOLLISION, and the readout's reseed count is the
    one the message names"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api
    tile = ws.many_hashed_reads(seed)
    want = orc.collapse(tile, want_rec_group=True)
    tbk_debug(monkeypatch, hash_mask="0xFFF")
    before = ctx.last_message()
    try:
        got, rec = _collapse(ctx, tile, form)
    except api.TbkError as e:
        assert e.status == -8 and ctx.collapse_route()["reseeds"] == 4
    else:
        _equal(got, want, rec)
        n = ctx.collapse_route()["reseeds"]
        assert 0 <= n < 4
        assert ctx.last_message() == ("info: key-hash collision, reseeded %d time(s)" % n if n else before)
    tbk_debug(monkeypatch, hash_mask=None)
    got, rec = _collapse(ctx, tile, form)
    _equal(got, want, rec)
    assert ctx.collapse_route()["reseeds"] == 0


def test_readout_costs_nothing_unasked(monkeypatch):
    """without wg_stats the readout holds the host's bookkeeping only, and the collapse runs the same kernels"""
    from tiebrush_amd import api, synth
    tile = synth.make_tile(8, 20000, "c3", n_loci=400)
    c = api.Context(0)
    c.set_profiling(True)
    tbk_debug(monkeypatch, path="window")
    c.collapse(tile)
    plain = {k: v[1] for k, v in c.kernel_times().items()}
    r = c.collapse_route()
    assert r["form"] == "raw" and "nw" not in r
    tbk_debug(monkeypatch, wg_stats="1")
    c.collapse(tile)
    assert {k: v[1] for k, v in c.kernel_times().items()} == plain
    assert c.collapse_route()["nw"] > 1
    tbk_debug(monkeypatch, path="sort", wg_stats=None)
    c.collapse(tile)
    assert c.collapse_route() == dict(form="sort", reseeds=0, raw_handed_back=False, big_bucket=False)
    c.close()
