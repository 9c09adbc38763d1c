"""Every scene of yd_item_scenes.py reaches the edge it is named for — proved on the CPU with the oracle, without a GPU.

The claims (yd_item_scenes.scene(name, **claim)):
  chains       lengths of the chains of the scene's one list (one file, one strand)
  far          the items of that list that are far: several exons, not the exact shape M N M
  probes       at least that many probing reads, and EVERY probing read has a non-zero YD that differs from its YD in the scene's
               other tile, where every read keeps its start and every far read takes the exons of the next variant — the neighbouring
               far group's geometry: exons read at another group's offset move the distances these reads report
  probe_groups groups (scenes of several files) with a non-zero YD that differs in the scene's other tile, as for `probes`
  ng           groups of the tile
  tile_items   items of every tile of 1024 groups
  peaks        groups with a YD of 30 and more among groups with 7 at the most
  far_groups   output places of the far groups
  second_round the tile holds more items than one staging round of yd_lscatter_k"""
import numpy as np
import pytest

import yd_item_scenes as ys

M, N = ys.M, ys.N


def _is_far(cig):
    ex = 1 + sum(1 for _, o in cig if o == N)
    return ex > 2 or (ex == 2 and [o for _, o in cig] != [M, N, M])


@pytest.mark.parametrize("name", list(ys.SCENES))
def test_scene_reaches_its_edge(name):
    claim = ys.SCENES[name][1]
    b, res = ys.build(name), ys.oracle(name)
    files = b["files"]
    yd = np.asarray(res["yd"])
    if "chains" in claim:
        assert len(files) == 1 and ys.chains_of(files[0]) == claim["chains"]
        assert res["n_groups"] == sum(claim["chains"])  # every read a group: the items of the list are the reads
    if "far" in claim:
        assert [i for i, r in enumerate(files[0]) if _is_far(r[6])] == claim["far"]
        assert [i for i, k in enumerate(b["kinds"]) if k.startswith("far")] == claim["far"]
    if "probes" in claim:
        other = np.asarray(ys.oracle(name, 1)["yd"])
        assert len(other) == len(yd)
        probes = [i for i, k in enumerate(b["kinds"]) if "probe" in k]
        assert len(probes) >= claim["probes"]
        for i in probes:
            assert yd[i] != 0 and yd[i] != other[i], (i, yd[i], other[i])
    if "probe_groups" in claim:
        other = np.asarray(ys.oracle(name, 1)["yd"])
        for g in claim["probe_groups"]:
            assert yd[g] != 0 and yd[g] != other[g], (g, yd[g], other[g])
    if "ng" in claim:
        assert res["n_groups"] == claim["ng"]
    if "tile_items" in claim:
        # one group per start in these scenes: a read's group is the rank of its start; an item per read, two where the strand is '.'
        gs = np.asarray(res["g_start"])
        assert np.all(np.diff(gs) > 0)
        items = np.zeros(-(-res["n_groups"] // ys.NT), np.int64)
        for f in files:
            g = np.searchsorted(gs, np.array([r[1] for r in f]))
            np.add.at(items, g // ys.NT, [2 if r[4] == "." else 1 for r in f])
        assert list(items) == claim["tile_items"]
    if "peaks" in claim:
        pk = claim["peaks"]
        assert int(yd[pk].min()) >= 30 and int(np.delete(yd, pk).max()) <= 7
    if "far_groups" in claim:
        gs, rep = np.asarray(res["g_start"]), np.asarray(res["rep"])
        allr = [r for f in files for r in f]  # (rep: index of the representative among the records of all files)
        assert [o for o in range(res["n_groups"]) if _is_far(allr[int(rep[o])][6])] == claim["far_groups"]
        assert np.all(np.diff(gs) > 0)  # one group per start: the output place of a group is its read's place in a file
    if "second_round" in claim:
        assert (claim["tile_items"][0] > ys.CAP) == claim["second_round"]


def test_dense_tiles_straddle_both_staging_sizes():
    n = [ys.SCENES["dense-%d" % f][1]["tile_items"][0] for f in (7, 8, 9)]
    assert n[0] == ys.CAP < ys.CAP_OLD < n[1] < n[2]
    # lists 0 .. 13 of the larger tiles hold 1021 items each (the probing groups are in the later files only) and list 14 all 1024
    # groups: the far item of group 500 in list 14 has the list-major index 14 * 1021 + 500, in list 15 another 1024 more
    assert 14 * 1021 + 500 >= ys.CAP and 14 * 1021 + 1024 + 500 >= ys.CAP_OLD
