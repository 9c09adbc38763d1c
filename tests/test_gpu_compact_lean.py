"""The compaction of the raw window form in its lean form (wgroup.hip): the caller's arrays are the only copy of a group's
representative, count and sample count, wg_tie_k takes a set member's values from window space, and the YD stage reads the caller's
representatives.  Every scene of compact_scenes.py (test_compact_scenes_cpu.py proves what each one reaches: groups, windows, tie sets
and listed records around the multiples of 64 and 256 groups) runs on one context and equals the oracle in rep, yc, yx, yd, g_start,
g_end, n_groups, n_passed and the number of reseeds; a sample also runs under wg_back=split, the sequence of separate passes with
every store of old, and under yd_front=split, whose pass of its own reads the representatives the same way.  The forms that are not
lean (a record -> group map, more than 64 files) keep every store; a caller without key and coordinates stays lean."""
import numpy as np
import pytest

import compact_scenes as cs
import test_gpu_window_backend as wb
import window_scenes as ws
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

GROUP_KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end")
FORMS = {"lean": dict(wg_back=None, yd_front=None), "split": dict(wg_back="split", yd_front=None), "yd-split": dict(wg_back=None, yd_front="split")}


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


def _run(ctx, monkeypatch, tile, want, forms=("lean",), keys=GROUP_KEYS, **kw):
    from tiebrush_amd import api
    dev = api.to_device(tile, "cuda:0")
    for form in forms:
        tbk_debug(monkeypatch, **FORMS[form])
        got = api.to_numpy(ctx.collapse(dev, **kw))
        ran, route = ctx.kernel_times(), ctx.collapse_route()
        assert "wg_compact" in ran and ("col_tie_sort" in ran) == (form == "split") and ("col_tie_sets" in ran) == (form != "split"), (form, sorted(ran))
        assert route["form"] == "raw" and route["reseeds"] == 0, (form, route)
        assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"], form
        for k in keys:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (form, k)
    tbk_debug(monkeypatch, **FORMS["lean"])


def _refused(ctx, monkeypatch, tile):
    """with the hash masked away the pair shares a key on every seed: four reseeds and TBK_ECOLLISION, lean and split alike"""
    from tiebrush_amd import api
    dev = api.to_device(tile, "cuda:0")
    for form in ("lean", "split"):
        tbk_debug(monkeypatch, hash_mask="0", **FORMS[form])
        with pytest.raises(api.TbkError) as e:
            ctx.collapse(dev)
        assert e.value.status == -8, form                              # TBK_ECOLLISION
        r = ctx.collapse_route()
        assert r["form"] == "none" and r["reseeds"] == 4, (form, r)
    tbk_debug(monkeypatch, hash_mask=None, **FORMS["lean"])


SPLIT_SAMPLE = ("ng-257", "windows-one-before-blocks", "ties-254-257", "ties-of-far-groups", "head-opens-a-block", "empty-windows-at-the-middle", "listed-records")


@pytest.mark.parametrize("name", list(cs.SCENES))
def test_scene(ctx, monkeypatch, name):
    _run(ctx, monkeypatch, cs.get(name), cs.oracle(name), ("lean", "split", "yd-split") if name in SPLIT_SAMPLE else ("lean",))


@pytest.mark.parametrize("k", [2, 64])
@pytest.mark.parametrize("name", ["ng-513", "ties-254-257", "ties-window-ends", "ties-of-far-groups", "head-opens-a-block", "listed-records", "collision-among-257"])
def test_scene_dealt_to_files(ctx, monkeypatch, name, k):
    """the groups and their places are those of one file; the windows are cut elsewhere (the samples are taken per file)"""
    _run(ctx, monkeypatch, cs.get(name, k), cs.oracle(name, k), ("lean", "split") if k == 64 else ("lean",))


@pytest.mark.parametrize("place", ["pile-up", "every-group"])
def test_scenes_of_the_back_end(ctx, monkeypatch, place):
    """a pile-up window of hundreds of groups in tie sets; one window whose every group is in one set: every member's representative,
    count and sample count come from window space"""
    tile, want = wb._tie_scene(place)
    _run(ctx, monkeypatch, tile, want, ("lean", "split", "yd-split"))


@pytest.mark.parametrize("name", ["collision-among-65", "collision-among-257"])
def test_collision_among_the_listed_records(ctx, monkeypatch, name):
    """the colliding pair among the 65 entries of one window and the 257 of another: the oracle's result (a tie set of two, whose
    members are far groups: the YD stage fetches their representatives) with the hash, refused without"""
    _run(ctx, monkeypatch, cs.get(name), cs.oracle(name))
    _refused(ctx, monkeypatch, cs.get(name))


@pytest.mark.parametrize("name", ["collision-tier1", "collision-tier2", "collision-lds-sort", "collision-pileup"])
def test_collision_in_one_window_of_each_tier(ctx, monkeypatch, name):
    tile = ws.get(name).tile
    _run(ctx, monkeypatch, tile, ws.oracle(name))
    _refused(ctx, monkeypatch, tile)


# ---- the forms that are not lean keep every store -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties-254-257", "listed-records"])
def test_record_group_map_is_not_lean(ctx, monkeypatch, name):
    _run(ctx, monkeypatch, cs.get(name), cs.oracle(name), ("lean", "yd-split"), GROUP_KEYS + ("rec_group",), want_rec_group=True)


@pytest.mark.parametrize("name", ["ties-254-257", "listed-records"])
def test_65_files_are_not_lean(ctx, monkeypatch, name):
    _run(ctx, monkeypatch, cs.get(name, 65), cs.oracle(name, 65))


@pytest.mark.parametrize("name", ["ties-254-257", "ties-window-ends", "ties-of-far-groups", "listed-records"])
def test_caller_without_key_and_coordinates_stays_lean(ctx, monkeypatch, name):
    _run(ctx, monkeypatch, cs.get(name), cs.oracle(name), ("lean", "yd-split"), ("rep", "yc", "yx", "yd"), want_coords=False, want_key=False)
