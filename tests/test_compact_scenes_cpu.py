"""Every scene of compact_scenes.py reaches the edge it is named for — proved from the oracle's result (which output places a tie set
occupies, which group is where) and the CPU model of the partition (window_model.py: the groups of every window, hence its first
group and the blocks of 256 output groups it meets; the listed records of every window).  A scene that misses its edge fails here,
without a GPU.

The claims (compact_scenes.scene(name, **claim)):
  ng                  groups of the tile
  window_starts       the first groups of the windows that hold groups
  blocks_of_a_window  the most blocks of 256 groups one window meets
  tie_sets            (first output place, members) of every tie set of several groups
  long_at             output places of groups whose representative has five CIGAR operations
  empty_run           a run of at least that many empty windows; the scene's name says where it lies among the windows with groups
  windows_in_a_block  windows with groups that blocks 0, 1, .. meet
  listed_windows      some block walks at least that many windows, empty ones included, from its first to its last
  entries             the listed records (hashed key words) of the first windows with groups
  split_listed_window a window with listed records starts inside a block and ends in a later one
  collision           a tie set of two whose representatives are the pair of five operations, both listed"""
import numpy as np
import pytest

import compact_scenes as cs
import window_model as wm

B = cs.BLOCK


def _layout(name, k=1):
    tile, res = cs.get(name, k), cs.oracle(name, k)
    P = wm.predict(tile, True, res["rec_group"])
    grp = np.asarray(P["groups"], np.int64)
    gbase = np.concatenate([[0], np.cumsum(grp)])[:-1]
    listed = wm.hashed_mask(tile) & P["part"].mask
    ent = np.bincount(P["part"].win[listed], minlength=len(grp))
    assert int(grp.sum()) == res["n_groups"]
    return tile, res, grp, gbase, ent


def _nops(tile, rec):
    off = tile.cig_off.astype(np.int64)
    return off[np.asarray(rec) + 1] - off[np.asarray(rec)]


@pytest.mark.parametrize("name", list(cs.SCENES))
def test_scene_reaches_its_edge(name):
    claim = cs.SCENES[name][1]
    tile, res, grp, gbase, ent = _layout(name)
    live = np.flatnonzero(grp > 0)
    first_b, last_b = gbase[live] // B, (gbase[live] + grp[live] - 1) // B
    if "ng" in claim:
        assert res["n_groups"] == claim["ng"]
    if "window_starts" in claim:
        assert list(gbase[live]) == claim["window_starts"]
    if "blocks_of_a_window" in claim:
        assert int((last_b - first_b + 1).max()) == claim["blocks_of_a_window"]
    if "tie_sets" in claim:
        assert cs.output_tie_sets(res) == sorted(claim["tie_sets"])
    if "long_at" in claim:
        assert list(_nops(tile, np.asarray(res["rep"])[claim["long_at"]])) == [5] * len(claim["long_at"])
    if "empty_run" in claim:
        empty = np.concatenate([[0], (grp == 0).astype(np.int64), [0]])
        edges = np.flatnonzero(np.diff(empty))
        runs = sorted((b - a, a) for a, b in zip(edges[0::2], edges[1::2]))
        length, at = runs[-1]
        assert length >= claim["empty_run"]
        before, behind = int((live < at).sum()), int((live >= at).sum())
        where = name.rsplit("-", 1)[1]
        assert grp[0] == 0 if where == "start" else grp[0] > 0                      # the tile begins with an empty window
        assert {"start": before == 1 and behind >= 1, "middle": before >= 1 and behind >= 1, "end": behind == 0}[where], (before, behind)
    if "windows_in_a_block" in claim:
        met = [int(((first_b <= b) & (last_b >= b)).sum()) for b in range(len(claim["windows_in_a_block"]))]
        assert met == claim["windows_in_a_block"]
    if "listed_windows" in claim:
        nb = -(-res["n_groups"] // B)
        met = [live[(first_b <= b) & (last_b >= b)] for b in range(nb)]
        walked = [int(w.max() - w.min() + 1) for w in met]
        assert max(walked) >= claim["listed_windows"]
    if "entries" in claim:
        assert list(ent[live][:len(claim["entries"])]) == claim["entries"]
    if claim.get("split_listed_window"):
        assert np.any((ent[live] > 0) & (gbase[live] % B != 0) & (last_b > first_b))
    if claim.get("collision"):
        (at, n), = cs.output_tie_sets(res)
        assert n == 2 and list(_nops(tile, np.asarray(res["rep"])[at:at + 2])) == [5, 5]
        w = np.flatnonzero((gbase <= at) & (at < gbase + grp))[0]
        assert ent[w] in (65, 257) and gbase[w] % B != 0


@pytest.mark.parametrize("k", [2, 64])
@pytest.mark.parametrize("name", ["ties-254-257", "ties-window-ends", "head-opens-a-block"])
def test_places_do_not_depend_on_the_files(name, k):
    """dealt to k files the records form the same groups at the same output places (the windows are cut elsewhere)"""
    claim = cs.SCENES[name][1]
    tile, res, grp, gbase, ent = _layout(name, k)
    assert res["n_groups"] == claim["ng"] and cs.output_tie_sets(res) == sorted(claim["tie_sets"])
    if "long_at" in claim:
        assert list(_nops(tile, np.asarray(res["rep"])[claim["long_at"]])) == [5] * len(claim["long_at"])
