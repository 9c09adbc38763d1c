"""The scenes of window_scenes.py through the CPU model of the window path (window_model.py), without a GPU: every scene reaches the
edge it is named for, every window that is not a pile-up on one base stays below 2 * 1024 + k * s records, and the route the device
test will demand of tbk_last_route is shown scene by scene (pytest -s prints it)."""
import os
import re

import numpy as np
import pytest

import window_model as wm
import window_scenes as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = -(2**31)


def _predict(name, raw):
    s = ws.get(name)
    opts = {k: v for k, v in s.opts.items() if k != "strategy"}
    p = wm.predict(s.tile, raw, ws.oracle(name)["rec_group"], **opts)
    P = p["part"]
    light = P.count[~P.heavy]
    assert light.size == 0 or int(light.max()) < P.window_bound, name                   # < 2 T + k s: what the LDS sort can take
    print("%-44s %-9s k=%-4d n=%-8d nw=%-5d live=%-5d ovf1=%-5d ovf2=%-5d big=%d largest window %d" %
          (name, "raw" if raw else "compacted", P.k, P.m, p["nw"], p["nw_live"], p["ovf1"], p["ovf2"], p["big_bucket"], int(P.count.max())))
    return p


def test_constants_are_the_kernel_sources():
    src = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "wgroup.hip")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1).strip()
    assert const("WG_NT") == "512" and const("WG_E") == "8" and const("WG_T") == "1024" and const("WG_KS") == "2048"
    assert const("WG_TC") == "4096" and const("WG_OC") == "2048" and const("WG_OG") == "8"
    assert const("WG_LDS_HASH") == "40448" and const("WG_LDS_HASH2") == "64 * 1024"
    assert "(gcap >> 2) * 3u" in src and "(WG_LDS_HASH - (8u * k + 8u)) / (44u + 4u * nwords)" in src
    csrc = os.path.join(ROOT, "tiebrush_amd", "csrc")
    assert "inline bool tbk_window_supported(uint32_t k) { return collapse_window_supported(k); }" in open(os.path.join(csrc, "wgroup.h")).read()
    plan = open(os.path.join(csrc, "collapse_plan.hpp")).read()
    assert "inline bool collapse_window_supported(uint32_t k) { return k >= 1 && k <= COLP_WINDOW_MAX_FILES; }" in plan
    assert "constexpr uint32_t COLP_WINDOW_MAX_FILES = 1024;" in plan
    assert (wm.WG_GC64, wm.WG_GC64_2) == (767, 1250)
    assert wm.thresholds(1, True) == wm.thresholds(64, True) == (573, 936)
    assert wm.thresholds(1, False) == (630, 1023) and wm.thresholds(64, False) == (573, 936)
    assert wm.gcaps(1024, True) == wm.gcaps(1024, False) == (187, 333) and wm.gcaps(1024, True)[0] * 8 < 2144
    assert [wm.stride(k) for k in (1, 2, 3, 64, 65, 1024)] == [(1024, 1), (1024, 1), (512, 2), (32, 32), (16, 64), (2, 512)]


@pytest.mark.parametrize("name", ws.TIER_SCENES)
def test_tiers_one_window(name):
    s = ws.get(name)
    assert s.tile.n_records <= 1024
    p = _predict(name, s.edge["mode"] == "raw")
    assert p["nw"] == 1 and p["nw_live"] == 1 and int(p["groups"][0]) == s.edge["groups"]
    assert (p["ovf1"], p["ovf2"]) == s.edge["route"] and not p["big_bucket"]
    k = s.tile.n_files
    assert np.all(np.diff(s.tile.file_off.astype(np.int64)) >= 0) and (k < 33 or len(set(s.tile.file_of().tolist())) > 32)


def test_one_file_too_many():
    s = ws.get("tier-k1025")
    assert s.tile.n_files == wm.WINDOW_MAX_FILES + 1


@pytest.mark.parametrize("name", ws.PILEUP_SCENES)
def test_tiers_pile_up(name):
    s = ws.get(name)
    p = _predict(name, s.edge["mode"] == "raw")
    P = p["part"]
    w = int(P.count.argmax())
    assert P.heavy[w] and int(P.count[w]) > wm.WG_CAP and int(p["groups"][w]) == s.edge["groups"]
    assert (p["ovf1"], p["ovf2"], p["big_bucket"]) == s.edge["route"] + (s.edge["big_bucket"],)
    rg = np.asarray(ws.oracle(name)["rec_group"])
    rec = P.rec[P.win == w]
    assert rg[rec[0]] != rg[rec[-1]]                                                  # first and last record of the pile-up: different groups
    assert np.all(P.pieces(w) > 2048)                                                 # ... every file's piece crosses chunks
    # a group's members lie in several files and several 512-record chunks of the window
    g0 = rec[rg[rec] == rg[rec[0]]]
    assert len(set(s.tile.file_of()[g0].tolist())) > 1 and len(set((np.searchsorted(rec, g0) // 512).tolist())) > 1


def test_largest_sortable_window():
    s = ws.get("largest-sortable-window")
    for raw in (True, False):
        p = _predict("largest-sortable-window", raw)
        P = p["part"]
        w = int(P.count.argmax())
        assert (P.s, P.g) == (32, 32) and not P.heavy[w]
        assert int(P.count[w]) == s.edge["window"] > 2048 and int(P.count[w]) > 4 * wm.WG_NT   # more than four of eight records per thread
        assert int(p["groups"][w]) > p["thr2"] and p["ovf2"] >= 1
        assert len(np.unique(P.keys)) == P.m


def test_worklist_scenes_outgrow_the_grids():
    for raw in (True, False):
        p = _predict("worklist-tier2", raw)
        P = p["part"]
        assert P.k == 1 and set(P.count[P.count > 0].tolist()) == {1024}
        assert p["ovf1"] > 512 and p["ovf2"] > 100 and p["ovf1"] - p["ovf2"] > 100 and p["nw_live"] - p["ovf1"] > 20
        p = _predict("worklist-sort", raw)
        P = p["part"]
        assert set(P.count[P.count > 0].tolist()) == {1024} and p["ovf2"] > 1024
        hashed = np.bincount(P.win[wm.hashed_mask(P.tile)[P.rec]], minlength=P.nw)[P.count > 0]
        assert np.all(hashed[0::2] == 0) and np.all(hashed[1::2] > 0)                   # verification entries: none in one window, some in the next


@pytest.mark.parametrize("name", ws.RUN_SCENES)
def test_runs_on_the_chunk_edges(name):
    s = ws.get(name)
    lens = np.diff(s.tile.file_off.astype(np.int64)).tolist()
    ln = s.edge["run"]
    at = [i for i, x in enumerate(lens) if x == ln]
    assert len(at) == 3 and 0 in lens and 1 in lens and lens[-1] == 0
    assert (at[0] == 0) == (not name.endswith("-lead")) and at[-1] == len(lens) - 2
    assert ln in (wm.WG_OC - 1, wm.WG_OC, wm.WG_OC + 1, wm.WG_TC - 1, wm.WG_TC, wm.WG_TC + 1, wm.WG_OG * wm.WG_OC - 1, wm.WG_OG * wm.WG_OC, wm.WG_OG * wm.WG_OC + 1)
    p = _predict(name, True)
    br = p["part"].offsets_branches(wg_og=8)
    assert br["first"] == sum(1 for x in lens if x) and (ln < 4095 or br["probe"] + br["run_end"] > 0)


def test_reference_changes_at_chunk_edges():
    s = ws.get("tid-change-at-chunk-edges")
    ct = wm.tid_chunks(s.tile)
    assert ct.tolist() == [0, 1, MIXED, 1, 0, MIXED, MIXED]
    t = s.tile.tid
    assert t[4095] == 0 and t[4096] == 1 and t[8192 + 4094] == 0 and t[8192 + 4095] == 1 and t[16384 + 4096] == 0 and t[16384 + 4097] == 1
    a, b = 6 * wm.WG_TC, s.tile.n_records - 1
    assert t[a] == t[b] == 1 and int(s.tile.file_off[4]) < b and b - a == wm.WG_TC - 1      # ends agree, but a file ends inside the chunk
    _predict("tid-change-at-chunk-edges", True)


def test_partition_shortcut_scenes():
    p = _predict("400-files-of-5", True)
    assert p["part"].k == 400 and p["part"].m == 2000
    for name, k in (("dense-64-files", 64), ("dense-96-files", 96)):
        s = ws.get(name)
        assert s.tile.n_files == k and int(np.diff(s.tile.file_off.astype(np.int64)).min()) >= 4100
        P = _predict(name, True)["part"]
        assert P.offsets_og() == 1                                                     # (tiles of this size: one chunk per block)
        br = P.offsets_branches(wg_og=8)
        assert br["search"] > 0 and br["probe"] > 0 and br["max_span"] >= 256, br
    p = _predict("unplaced-tail", True)
    P = p["part"]
    w = int(P.win[-1])
    assert int(P.keys[-1]) == wm.UNPLACED and P.heavy[w] and int(P.count[w]) > wm.WG_OC and int(p["groups"][w]) == 0
    tails = [int((s_tid < 0).sum()) for s_tid in np.split(P.tile.tid, P.tile.file_off[1:-1].astype(np.int64))]
    assert 0 in tails and max(tails) > wm.WG_TC
    p = _predict("extreme-coordinates", True)
    t = p["part"].tile
    assert int(t.pos.min()) == 0 and int(t.pos.max()) == 2**31 - 1 and int(t.tid[t.pos == 2**31 - 1].min()) == int(t.tid.max())
    assert int(p["part"].keys[t.tid >= 0].max()) >> 32 > 0


@pytest.mark.parametrize("name", ws.PILE_SCENES)
def test_pile_ups_at_the_partitions_edges(name):
    s = ws.get(name)
    pr, pc = _predict(name, True), _predict(name, False)
    for p in (pr, pc):
        P = p["part"]
        assert np.all(P.count[P.heavy] > 2 * wm.WG_T) and not p["big_bucket"]
    P = pr["part"]
    hw = np.flatnonzero(P.heavy)
    live = np.flatnonzero(P.count > 0)
    if name in ("piles-adjacent-bases", "piles-across-references"):
        assert len(hw) == 2 and P.W[hw[0]] == P.W[hw[1] - 1] and int(P.count[hw[0] + 1: hw[1]].sum()) == 0   # bound v + 1 of the first = bound v of the second
    if name == "piles-across-references":
        assert int(P.W[hw[0]]) == 1 << 31 and int(pr["groups"][hw[0]]) == 0 and int(pc["part"].heavy.sum()) == 1
    if name == "piles-first-and-last-key":
        assert hw[0] == live[0] and hw[1] == live[-1]
    if name == "piles-one-record-between":
        assert len(hw) == 2 and int(P.count[hw[0] + 1: hw[1]].sum()) == 1
    if name == "pile-all-filtered":
        assert len(hw) == 2 and int(pr["groups"][hw[0]]) == 0 and int(P.count[hw[0]]) == 2600     # raw: a live window without a group
        assert int(pc["part"].heavy.sum()) == 1 and pc["nw_live"] < pr["nw_live"]                # compacted: it does not exist


def test_effective_end_scene_shows_every_carry_in_the_representative():
    from oracle import oracle_ffi as orc
    base = ws.get("effective-ends").tile
    want = ws.oracle("effective-ends")
    for raw in (True, False):
        p = _predict("effective-ends", raw)
        assert p["nw_live"] == 1 and p["part"].heavy[int(p["part"].count.argmax())]
    assert ws.EFF_SETTERS == (63, 8 * 64 - 1, 4 * 512 - 1, ws.EFF_LEN0 - 1) and int(base.file_off[1]) == ws.EFF_LEN0
    f1 = int(base.file_off[1])
    for j in range(3):                       # the record behind setter j inherits its end: the representative is file 1's member
        assert rep_in(base, want, 31 + j) == f1 + 2 + 2 * j
        low = ws.effective_ends(("lower", j))
        assert rep_in(low, orc.collapse(low), 31 + j) == ws.EFF_SETTERS[j] + 1     # ... without the maximum it is that record itself
    assert rep_in(base, want, 34) == f1                                              # file 1's first record does not inherit file 0's last
    joined = ws.effective_ends("join")
    assert rep_in(joined, orc.collapse(joined), 34) == int(joined.file_off[2]) + 2  # ... in one file it would, and file 2's member leads
    assert int(base.flag[511]) & 0x100 and int(base.flag[1000]) & 4                  # a filtered setter, an unmapped mate inside the run


def rep_in(tile, res, ln):
    return ws.rep_of(tile, res, ln)


@pytest.mark.parametrize("name", list(ws.COLLISION_SCENES))
def test_collision_scenes(name):
    s = ws.get(name)
    want = ws.oracle(name)
    hm = wm.hashed_mask(s.tile)
    pair = np.flatnonzero(hm)
    assert len(pair) == 2 and want["rec_group"][pair[0]] != want["rec_group"][pair[1]]
    assert s.tile.pos[pair[0]] == s.tile.pos[pair[1]]
    for raw in (True, False):
        p = _predict(name, raw)
        P = p["part"]
        w = int(P.win[pair[0]])
        assert w == int(P.win[pair[1]])
        here = (int(p["groups"][w] > p["thr1"]), int(p["groups"][w] > p["thr2"]))
        if name.startswith("collision-tier1"):
            assert here == (0, 0)
        if name == "collision-tier2":
            assert here == (1, 0)
        if name == "collision-lds-sort":
            assert here == (1, 1)
        if name == "collision-pileup":
            assert P.heavy[w] and pair[1] - pair[0] > wm.WG_CAP and np.searchsorted(P.rec[P.win == w], pair[1]) - np.searchsorted(P.rec[P.win == w], pair[0]) > wm.WG_CAP
        if name == "collision-only-hashed-of-their-window":
            assert p["nw_live"] > 3 and np.bincount(P.win[hm[P.rec]], minlength=P.nw).tolist().count(0) == P.nw - 1 and here == (0, 0)
    fo = s.tile.file_of()
    assert (fo[pair[0]] == fo[pair[1]]) == (name == "collision-tier1-one-file")


def test_hidden_inversion_scenes():
    t = ws.hidden_tid_inversion(False)
    assert wm.tid_chunks(t)[0] == 0 and t.tid[0] == t.tid[4095] == 0 and t.tid[2000] == 1
    assert not wm.filter_mask(ws.hidden_tid_inversion(True))[2000:4096].any() and wm.filter_mask(ws.hidden_tid_inversion(True))[:2000].all()
    for at in (wm.WG_OC, wm.WG_OG * wm.WG_OC):
        t = ws.pos_inversion(at, False)
        assert t.pos[at] < t.pos[at - 1] and np.all(np.diff(t.pos[:at].astype(np.int64)) >= 0) and at % wm.WG_OC == 0
