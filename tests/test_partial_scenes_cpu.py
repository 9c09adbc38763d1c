"""Every scene of partial_scenes.py reaches the edge it is named for — proved on the CPU with the model and the oracle, without a GPU.
The rows come from the oracle's local collapses and dist._partial_pack_np (word 10, the key word, is absent there and not needed).

The claims (partial_scenes.Scene(..., **claim)):
  windows     windows of the partition (2 nsp + 1)
  groups      groups of the oracle's collapse of the received rows;  members: {members per group: groups}
  heavy       rows of the one heavy window [v, v + 1) — all on one place, between equal consecutive splitters, an empty window beside it
  one_window  all rows lie in one window of that many rows (thread t of pr_merge_k owns ceil(n / 256) of its sorted positions)
  group_at    (first sorted position, members) of one group
  splitters   (tid, pos) places that are bounds of the partition
  empty_runs  runs without a row
  ties        the tie sets hold several key classes: exact words only, hashed words only, both; a group whose members differ in their
              CIGAR words where the strategy allows it; the three strands
  rep_run     {pos: runs whose rows tie on the smallest effective end}: the representative is the one received first
  sums        {pos: (YC, YX[, YD])} of the group on that place
What the GPU test relies on when it expects no refusal — no window above PR_CAP — is asserted for every scene that expects status 0."""
import numpy as np
import pytest

import partial_scenes as ps


def _orders(name):
    return (False, True) if ps.SCENES[name].reverse else (False,)


def test_constants_and_stride():
    """the arithmetic the scenes are sized by: for every number of runs the first splitter appears between 512 and 513 rows, and a
    window that is not heavy stays below 2 PR_T + k s <= PR_CAP"""
    assert (ps.PR_T, ps.PR_KS, ps.PR_CAP, ps.PR_MAXRUNS, ps.PR_NT) == (512, 512, 1536, 64, 256)
    assert ps.PR_CAP % ps.PR_NT == 0 and ps.PR_CAP // ps.PR_NT == 6          # PR_E
    assert ps.PR_MAXRUNS <= 64 and ps.PR_MAXRUNS <= 255                       # one wave for the piece table, uint8_t pf[]
    assert ps.PR_CAP <= 65535                                                 # uint16_t srt[]
    for k in range(1, ps.PR_MAXRUNS + 1):
        s, g = ps.stride(k)
        assert s & (s - 1) == 0 and s * k <= ps.PR_KS and s <= ps.PR_T and s * g == ps.PR_T
        assert (2 * s * k > ps.PR_KS or 2 * s > ps.PR_T)                      # the largest such power of two
        assert 2 * ps.PR_T + k * s <= ps.PR_CAP
        nsp = lambda m: ((-(-m // s)) - 1) // g if -(-m // s) > 1 else 0
        assert nsp(512) == 0 and nsp(513) == 1 and nsp(1024) == 1 and nsp(1025) == 2


def test_capacity_by_the_model_alone():
    """PR_CAP rows on one place are one window the kernel takes, PR_CAP + 1 are not — from the places alone"""
    for k, per, extra, fits in ((1, 1536, 0, True), (64, 24, 0, True), (64, 24, 1, False), (4, 384, 1, False)):
        keys = [np.full(per + (extra if r == 0 else 0), (0 << 31) | 1000, np.uint64) for r in range(k)]
        P = ps.partition(keys)
        assert P["count"].max() == k * per + extra and (P["count"].max() <= ps.PR_CAP) == fits
        assert P["heavy"][np.argmax(P["count"])] and (P["count"] > 0).sum() == 1


@pytest.mark.parametrize("name", list(ps.SCENES))
def test_scene_reaches_its_edge(name):
    sc = ps.SCENES[name]
    claim = sc.claim
    for rev in _orders(name):
        rows, run_off, cig = ps.packed(name, rev)
        t2, want = ps.expected_of(name, rev)
        rg = np.asarray(want["rec_group"])
        ng = int(want["n_groups"])
        assert (rg >= 0).all()                                         # every filter open: every row is in a group
        members = np.bincount(rg, minlength=ng)
        first_pos = np.concatenate([[0], np.cumsum(members)])          # sorted position of every group's first member
        if "groups" in claim:
            assert ng == claim["groups"]
        if "members" in claim:
            assert {int(a): int(b) for a, b in zip(*np.unique(members, return_counts=True))} == claim["members"]
        if "empty_runs" in claim:
            assert [r for r in range(sc.k) if not sc.runs[r]] == claim["empty_runs"]
            assert (np.diff(run_off.astype(np.int64)) == 0).sum() == len(claim["empty_runs"])
        if sc.k > ps.PR_MAXRUNS:
            assert sc.expect == ps.EUNSUPPORTED
            continue
        assert sc.k == len(run_off) - 1
        P = ps.partition_of(name, rev)
        cnt = P["count"]
        assert P["m"] == len(rows) and cnt.sum() == P["m"]
        if P["nsp"]:
            assert sorted(P["rank"].tolist()) == list(range(P["ns"]))  # pr_sample_rank_k: every rank taken once
        assert np.all(np.diff(P["W"].astype(np.int64)) >= 0)
        assert P["nw"] == claim["windows"]
        assert np.all(cnt[~P["heavy"]] < P["bound"]) and P["bound"] <= ps.PR_CAP
        pile = sc.expect == ps.E2BIG and claim.get("heavy", 0) > ps.PR_CAP
        assert (cnt.max() > ps.PR_CAP) == pile                         # accepted scenes: no window above PR_CAP
        if "heavy" in claim:
            hw = np.flatnonzero(P["heavy"] & (cnt > 0))
            assert len(hw) == 1 and cnt[hw[0]] == claim["heavy"]
            w = int(hw[0])
            assert P["W"][w - 1] + np.uint64(1) == P["W"][w]           # [v, v + 1): equal consecutive splitters
            assert len(np.unique(ps.place_keys(rows)[P["win"] == w])) == 1
            assert cnt[w - 1] == 0 or cnt[w + 1] == 0 or (cnt == 0).any()
            assert (cnt == 0).any()
        if "one_window" in claim:
            n = claim["one_window"]
            assert cnt.max() == n == P["m"] and (cnt > 0).sum() == 1
            eu = -(-n // ps.PR_NT)
            last = first_pos[1:] - 1
            if name.startswith("seam_") and name[5:].isdigit():
                assert np.any(first_pos[:-1] // eu != last // eu)      # groups whose members cross a thread's range
                assert np.any((members == 3) & (first_pos[:-1] % eu == eu - 1)) or eu == 1
        if "group_at" in claim:
            pos, mem = claim["group_at"]
            g = int(np.searchsorted(first_pos, pos))
            assert first_pos[g] == pos and members[g] == mem
            if name == "seam_last_single":
                n = claim["one_window"]
                assert g == ng - 1 and pos + mem == n and members[g - 1] == 3 and pos % (-(-n // ps.PR_NT)) == 0
        if "splitters" in claim:
            for tid, pos in claim["splitters"]:
                v = np.uint64((tid << 31) | pos)
                assert v in P["W"]
                assert ps.place_keys(rows)[rows[:, 0] == tid].min() == v     # the first place of its reference
        if claim.get("ties"):
            _check_ties(sc, rows, run_off, cig, t2, want, members)
        rep = np.asarray(want["rep"]).astype(np.int64)
        if "rep_run" in claim:
            order = ps.order_of(name, rev)
            for pos, tied in claim["rep_run"].items():
                g = _group_on(want, rows, pos, 150)
                assert rows[rep[g], 4] == min(order.index(r) for r in tied)     # word 4: the global file = the rank that sent the row
                effs = rows[rg == g, 3]
                assert (effs == effs.min()).sum() == len(tied) and rows[rep[g], 3] == effs.min()
        for pos, sums in claim.get("sums", {}).items():
            g = _group_on(want, rows, pos, 150)
            for key, v in zip(("yc", "yx", "yd"), sums):
                if v is not None:
                    assert want[key][g] == v, (key, pos)


def _group_on(want, rows, pos, span):
    g = np.flatnonzero((np.asarray(want["g_start"]) == pos + 1) & (np.asarray(want["g_end"]) == pos + span))
    assert len(g) == 1
    return int(g[0])


def _check_ties(sc, rows, run_off, cig, t2, want, members):
    rep = np.asarray(want["rep"]).astype(np.int64)
    rg = np.asarray(want["rec_group"])
    co = t2.cig_off.astype(np.int64)
    words = lambda i: tuple(int(x) for x in cig[co[i]:co[i + 1]])
    cigar_of = lambda i: [(w >> 4, w & 0xF) for w in words(i)]
    sets = {}
    for g in range(int(want["n_groups"])):
        sets.setdefault((int(want["g_start"][g]), int(want["g_end"][g]), int(t2.strand[rep[g]])), []).append(g)
    kinds = set()
    for gs in sets.values():
        if len(gs) < 2:
            continue
        ex = [ps.exact_key_word(cigar_of(rep[g]), sc.strategy) for g in gs]
        kinds.add("exact" if all(ex) else ("mixed" if any(ex) else "hashed"))
    assert kinds == {"exact", "hashed", "mixed"}
    assert sum(1 for gs in sets.values() if len(gs) == 3) >= 2                 # A < B < C on one key
    # every tie set's groups lie in at least two runs each, in different pairs of runs
    run_of = np.searchsorted(run_off.astype(np.int64), np.arange(len(rows)), side="right") - 1
    for gs in sets.values():
        if len(gs) == 3:
            pairs = {tuple(sorted(run_of[rg == g].tolist())) for g in gs}
            assert pairs == {(0, 1), (0, 2), (1, 2)}
    # a group whose members differ in their CIGAR words: never under cigar, a soft clip under clip, an indel under exon
    differ = [g for g in range(int(want["n_groups"])) if len({words(i) for i in np.flatnonzero(rg == g)}) > 1]
    assert bool(differ) == (sc.strategy != "cigar")
    if sc.strategy == "clip":
        assert any(ps.exact_key_word(cigar_of(rep[g]), "clip") for g in differ) and any(not ps.exact_key_word(cigar_of(rep[g]), "clip") for g in differ)
    # the three strands on one base: three groups of two members
    on = [g for g in range(int(want["n_groups"])) if want["g_start"][g] == 6001]
    assert sorted(chr(t2.strand[rep[g]]) for g in on) == ["+", "-", "."] and all(members[g] == 2 for g in on)
