"""The scenes of cut_scenes.py through the CPU model of the multi-rank cut search (cut_model.py), without a GPU: every scene sits on the
edge it is named for, and on every scene and on seeded random ones the contract of include/tbk.h holds between two independent
statements of it — a cut the gathered lists settle is exactly the smallest clean key at or behind its target (the brute force
cut_model.exact_cut) and what the protocol's rounds walk to; a cut they leave unsettled has that key at or beyond some rank's horizon,
or no clean key at all.  tests/test_gpu_cut_search.py demands the same arrays of the device (pytest -s prints what each scene does)."""
import os
import re

import numpy as np
import pytest

import cut_model as cm
import cut_scenes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, K = cm.INF, cm.K


def test_constants_are_the_kernel_sources():
    src = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "shard.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "tbk.h")).read()
    from tiebrush_amd import _lib, dist
    assert "#define TBK_PARTIAL_BUNDLES %d\n" % cm.BUNDLES in hdr and "#define TBK_PARTIAL_META (%d + 4)" % cm.SAMPLES in hdr
    assert (_lib.PARTIAL_CAND, _lib.PARTIAL_META, dist.KEY_INF, dist.N_SAMPLES) == (cm.CAND, cm.META, INF, cm.SAMPLES)
    assert "constexpr uint32_t LIMIT = 1u << 22;" in src and "base += %d;" % cm.STEP in src and "PM_INF = (int64_t)1 << 62" in src
    assert re.search(r"partial_cands_k, world - 1, %d, 0" % cm.STEP, src)


def _settle_properties(ranks, tg, allc, label):
    """the contract on one scene: per cut, the lists' verdict against the brute force and the rounds; returns (cuts, unsettled ones)"""
    pairs = [(r.key, r.endk) for r in ranks]
    walks = [(r.key, r.emax) for r in ranks]
    n_uns = 0
    for c, t in enumerate(int(v) for v in tg):
        cut, uns = cm.choose(allc[:, c, :], t)
        exact = cm.exact_cut(pairs, t)
        walked, _ = cm.rounds_cut(walks, t)
        assert walked == exact, (label, c, walked, exact)
        if uns:
            n_uns += 1
            hz = int(allc[:, c, 1].min())
            assert cut == INF and (exact == INF or exact >= hz), (label, c, exact, hz)
        else:
            assert cut == exact, (label, c, cut, exact)
            if t < INF and exact < INF:           # a settled cut is clean for every rank: said once more from the groups themselves
                assert all(int(r.endk[r.key < cut].max(initial=-1)) < cut for r in ranks)
    return len(tg), n_uns


def _table_lists(s):
    per = [cm.stage_cands(r.key, r.emax, s.allmeta, s.world) for r in s.ranks]
    return per[0][0], np.stack([p[1] for p in per])


@pytest.mark.parametrize("name", list(cs.TABLE))
def test_table_scene_sits_on_its_edge(name):
    s = cs.table(name)
    tg, allc = _table_lists(s)
    e = s.edge
    r0 = s.ranks[0]
    print("%-34s world %-2d ng %-22s targets %d  %s" % (name, s.world, [r.ng for r in s.ranks][:6], len(tg), s.doc))
    nonempty = [r for r in s.ranks if r.ng]
    assert all(int(r.key.min()) >= 1 << 32 for r in nonempty)                        # tid >= 1: a key cut to 32 bits is another key
    if "empty" in e:
        for r in e["empty"]:
            assert s.ranks[r].ng == 0 and np.all(s.allmeta[r, :cm.SAMPLES] == INF)
            for c in range(s.world - 1):
                assert allc[r, c, 0] == -1 and allc[r, c, 1] == INF and np.all(allc[r, c, 2::2] == INF) and np.all(allc[r, c, 3::2] == -1)
    if e.get("no_targets"):
        assert np.all(tg == INF) and cm.stage_choose(allc, tg)[1] == 0 and np.all(cm.stage_choose(allc, tg)[0] == INF)
    if "ng" in e:
        n = e["ng"]
        idx = (np.arange(64) * n) // 64
        assert all(r.ng == n for r in s.ranks) and np.array_equal(s.allmeta[0, :64], r0.key[idx])
        assert len(set(idx.tolist())) == min(n, 64) and (n != 65 or 64 not in idx.tolist())
    if "idx0" in e:
        idx0 = cm.walk(r0.key, r0.emax, int(tg[0]))[0]
        assert idx0 == e["idx0"] and (idx0 % 256 != 0 or not ("offsets" in e or "head16" in e))
    if name == "target-below-first-key":
        assert allc[0, 0, 0] == -1 and allc[0, 0, 2] == r0.key[0]
    if name == "target-above-last-key":
        assert allc[0, 0, 0] == r0.emax[-1] and allc[0, 0, 2] == INF and cm.heads_behind(r0.key, r0.emax, int(tg[0])) == 0
    if name == "target-on-head":
        assert allc[0, 0, 2] == tg[0] and allc[0, 0, 0] == r0.emax[6]
    if name == "target-on-non-head":
        assert tg[0] == r0.key[2] and allc[0, 0, 2] == r0.key[3] > tg[0] and allc[0, 0, 0] == r0.emax[2]
    if name == "target-on-shared-key":
        assert list(r0.key).count(int(tg[0])) == 3 and allc[0, 0, 2] == tg[0] and allc[0, 0, 0] == r0.emax[2] and allc[0, 0, 3] == r0.emax[6]
    if e.get("tid") == cs.BIG_TID:
        assert int(tg[0]) >> 47
    if "heads" in e:
        n, t = e["heads"], int(tg[0])
        assert cm.heads_behind(r0.key, r0.emax, t) == n and r0.emax[-1] != r0.endk[-2]
        src = cm.horizon_source(r0.key, r0.emax, t)
        hd = cm.walk(r0.key, r0.emax, t)[1]
        last = allc[0, 0, 2 + 2 * (min(n, 15) - 1) + 1]
        if n <= 15:
            assert src == "none" and allc[0, 0, 1] == INF and last == r0.emax[-1] and allc[0, 0, 2 + 2 * n if n < 15 else 30] == (INF if n < 15 else r0.key[hd[14]])
        else:
            assert src == "head16" and allc[0, 0, 1] == r0.key[hd[15]] and last == r0.emax[hd[15] - 1] != r0.emax[-1]
    if "offsets" in e:
        hd = cm.walk(r0.key, r0.emax, int(tg[0]))[1]
        assert [h - e["idx0"] for h in hd] == e["offsets"] and cm.horizon_source(r0.key, r0.emax, int(tg[0])) == "none"
    if "head16" in e:
        idx0, hd, base, hit = cm.walk(r0.key, r0.emax, int(tg[0]))
        assert len(hd) == 16 and hd[15] - idx0 == e["head16"] and base - idx0 == 256 * (e["head16"] // 256) and not hit
        assert allc[0, 0, 1] == r0.key[hd[15]]
    if name == "step-of-256-heads":
        assert cm.heads_behind(r0.key, r0.emax, int(tg[0])) == 256 and not cm.heads_of(r0.key, r0.emax)[100:356].any()
        assert cm.heads_of(r0.key, r0.emax)[356:612].all()
    if name == "reference-change":
        assert tg[0] == 7 << 31 and allc[0, 0, 2] == K(6, 1) and allc[0, 0, 0] == K(5, 2**31 - 1) and allc[0, 0, 4] == K(cs.BIG_TID, 1)
    if "world" in e:
        assert s.world == e["world"] and len(tg) == s.world - 1 and np.all(np.diff(tg) >= 0)
        if s.world == 64:
            assert s.allmeta[:, :64].size == 4096                                       # the whole LDS array of the sort
            cuts, flag = cm.stage_choose(allc, tg)
            where = [1 + r * cm.BUNDLES + b for c in range(63) for r in range(64) for b in range(cm.BUNDLES)
                     if cuts[c] < INF and allc[r, c, 2 + 2 * b] == cuts[c] and cuts[c] != tg[c]]
            assert max(where) >= 256, max(where)               # a winning candidate that only a second pass of the 256 threads reaches
            assert np.array_equal(s.allmeta[9], s.allmeta[8][:64].tolist() + [1, 9, 0, 0]) and (s.allmeta[31, :64] == INF).all()
    _settle_properties(s.ranks, tg, allc, name)


@pytest.mark.parametrize("extra", [0, 1])
def test_give_up_limit_scene(extra):
    """one bundle of 2^22 groups behind the target: with nothing after it the walk runs off the end (no horizon); with one more group it
    gives up ON that group, whose key becomes the horizon — the limit cannot be reached with less"""
    r0 = cs.limit_rank_np(extra)
    t = cs.LIMIT_TARGET
    idx0, hd, base, hit = cm.walk(r0.key, r0.emax, t)
    assert idx0 == 3 and hd == [3] and base - idx0 == cm.LIMIT and hit == bool(extra) and r0.ng == 3 + cm.LIMIT + extra
    got = cm.cands(r0.key, r0.emax, t)
    assert cm.horizon_source(r0.key, r0.emax, t) == ("limit" if extra else "none")
    assert got[1] == (r0.key[3 + cm.LIMIT] if extra else INF) and got[0] == r0.emax[2] and got[2] == t and got[3] == r0.emax[-1] and got[4] == INF
    allc = np.stack([got, cm.cands(cs.LIMIT_OTHER.key, cs.LIMIT_OTHER.emax, t)])[:, None, :]
    # the smallest clean key is rank 1's start beyond the far end of the long bundle: judged without a horizon, skipped behind one
    assert cm.choose(allc[:, 0, :], t) == ((INF, True) if extra else (K(8, cs.LIMIT_BEYOND), False))
    assert cm.exact_cut([(r0.key, r0.endk), (cs.LIMIT_OTHER.key, cs.LIMIT_OTHER.endk)], t) == K(8, cs.LIMIT_BEYOND)
    _settle_properties([r0, cs.LIMIT_OTHER], [t], allc, "limit+%d" % extra)


@pytest.mark.parametrize("name", list(cs.CHOOSE))
def test_choose_scene_sits_on_its_edge(name):
    s = cs.CHOOSE[name]
    raw = [cm.choose(s.allcands[:, c, :], int(s.targets[c])) for c in range(s.world - 1)]
    cuts, flag = cm.stage_choose(s.allcands, s.targets)
    print("%-30s world %d cuts %s flag %d  %s" % (name, s.world, [hex(int(c)) for c in cuts], flag, s.doc))
    assert np.array_equal(cuts, s.cuts) and flag == (2 if s.unsettled else 0)
    if s.raw_cuts is not None:
        assert [r[0] for r in raw] == list(s.raw_cuts) and list(s.raw_cuts) != sorted(s.raw_cuts)
    if name == "target-clean":
        assert cm.judge(s.allcands[1, 0], int(cuts[0])) == int(cuts[0]) - 1 and cuts[0] == s.targets[0]
    if name == "target-reached-by-one":
        assert cm.judge(s.allcands[1, 0], int(s.targets[0])) == int(s.targets[0]) and cuts[0] == s.allcands[1, 0, 2]
    if name == "third-rank-wins":
        assert cuts[0] == s.allcands[2, 0, 2] and all(cm.judge(s.allcands[2, 0], int(x)) < int(x) for x in (s.targets[0], s.allcands[0, 0, 2], s.allcands[1, 0, 2]))
    if name == "candidate-on-horizon":
        assert cuts[0] == s.allcands[1, 0, 1] == s.allcands[0, 0, 2]
    if name == "candidate-beyond-horizon":
        assert s.allcands[0, 0, 2] == s.allcands[1, 0, 1] + 1
        other = cs.CHOOSE["candidate-on-horizon"]
        assert (s.allcands != other.allcands).sum() == 1
    if name == "world-64-winners-beyond-256":
        for c, q in cs.W64_WINNERS.items():
            hits = [1 + r * cm.BUNDLES + b for r in range(64) for b in range(cm.BUNDLES) if s.allcands[r, c, 2 + 2 * b] == cuts[c]]
            assert hits == [q] and q >= 256 and raw[c] == (int(cuts[c]), False)
        assert max(cs.W64_WINNERS.values()) == 1 + 64 * cm.BUNDLES - 1
    if name.startswith("two-targets"):
        d = {3: 0, 5: 1}[s.world]
        assert cuts[d] == cuts[d + 1] and s.targets[d] < s.targets[d + 1]
    key = _choose_tile_keys()
    tab = cm.table(key, cuts, np.ones(len(key), np.int64))
    if name.startswith("two-targets"):
        assert tab[d + 1, 1] == 0 and tab[:, 1].sum() == len(key)
    if name == "two-targets-one-bundle-w5":
        assert cuts[-1] > key[-1] and tab[-1, 1] == 0 and tab[-1, 0] == len(key)
    if name == "earlier-cut-lowered":
        assert list(key).count(int(cuts[0])) == 4 and tab[1, 0] == np.searchsorted(key, cuts[0]) and tab[1, 1] == 0
    if s.unsettled or name == "all-targets-inf":
        assert tab[0, 1] == len(key) and not tab[1:, 1].any()


def _choose_tile_keys():
    """the keys of the tiny tile's groups: one group per distinct (tid, start, CIGAR) — 1-based starts"""
    g = sorted({(t, p + 1, tuple(c)) for f in cs.CHOOSE_FILES for t, p, c in f})
    return np.array([K(t, s) for t, s, _ in g], np.int64)


def test_choose_tile_has_the_keys_the_scenes_cut_at():
    key = _choose_tile_keys()
    assert len(key) == 11 and list(key).count(K(cs.TA, 200)) == 4 and list(key).count(K(cs.TB, 50)) == 2 and key.min() >= 1 << 32


@pytest.mark.parametrize("name", cs.TILE_NAMED)
def test_tile_scene_sits_on_its_edge(name):
    s = cs.tile(name)
    ranks = s.ranks()
    tg, allc, raw, cuts, flag = cs.verdict(name)
    print("%-18s world %d groups %-22s cuts %s flag %d  %s" % (name, s.world, [r.ng for r in ranks], [hex(int(c)) for c in cuts], flag, s.doc))
    _settle_properties(ranks, tg, allc, name)
    if name == "filtered-rank":
        assert ranks[1].ng == 0 and len(s.reads[1]) > 0 and flag == 0
    if name == "two-references":
        assert flag == 0 and cuts[0] == min(int(r.key[r.key >= K(2, 0)][0]) for r in ranks)
        assert max(int(r.endk[r.key < cuts[0]].max()) for r in ranks) < K(1, 0)
    if name == "touching-reads":
        t, c = int(tg[0]), int(cuts[0])
        both = np.concatenate([r.key for r in ranks]), np.concatenate([r.endk for r in ranks])
        assert flag == 0 and (t & 0x7FFFFFFF) % 1000 == 200
        assert t in ranks[0].key and t in both[1]              # the target is a start of rank 0 and the keyed end (end + 1) of a read of rank 1
        nxt = int(both[0][both[0] > t].min())
        assert nxt == t + 50 and nxt in both[1] and nxt in ranks[1].key       # so is the next start, of rank 1, behind the target
        assert c == t + 101 and c - 1 in both[1] and c in ranks[0].key        # the cut: the first start at an end + 2
    if name == "few-groups":
        assert [r.ng for r in ranks] == [1, 63, 64, 65]
    if name == "scan-tiles":
        assert all(r.ng > 2 * 2048 for r in ranks) and ranks[0].emax[4200] == ranks[0].endk[0] > ranks[0].endk[4200] and flag == 2


def test_staircases_find_the_lists_limit():
    """the model decides which staircase the lists still settle: up to some length every cut settles, beyond it none does"""
    flags = [cs.verdict("staircase-%d" % n)[4] for n in cs.STAIR_LENGTHS]
    for n in cs.STAIR_LENGTHS:
        s = cs.tile("staircase-%d" % n)
        tg, allc, _, _, _ = cs.verdict(s.name)
        _settle_properties(s.ranks(), tg, allc, s.name)
    longest, shortest = cs.stair_edge()
    print("staircases %s -> flags %s: the lists settle %d links and give up %d" % (cs.STAIR_LENGTHS, flags, longest, shortest))
    assert flags == sorted(flags) and flags[0] == 0 and flags[-1] == 2
    assert shortest == cs.STAIR_LENGTHS[cs.STAIR_LENGTHS.index(longest) + 1] == longest + 1      # the edge is found to the link


def test_random_scenes_settle_most_cuts_and_not_all():
    """seeded random loci: the contract on every cut, and the share of unsettled cuts — at most a quarter (the lists are worth having),
    at least one in twenty (the GPU test sees the other verdict too)"""
    n_cuts = n_uns = 0
    worlds = set()
    empties = 0
    for name in cs.RANDOM:
        s = cs.tile(name)
        ranks = s.ranks()
        tg, allc, _, _, _ = cs.verdict(name)
        a, b = _settle_properties(ranks, tg, allc, name)
        n_cuts, n_uns = n_cuts + a, n_uns + b
        worlds.add(s.world)
        empties += sum(r.ng == 0 for r in ranks)
    print("random scenes: %d cuts, %d unsettled (%.1f %%), %d empty ranks" % (n_cuts, n_uns, 100.0 * n_uns / n_cuts, empties))
    assert worlds == set(cs.RANDOM_WORLDS) and empties >= 2
    assert 4 * n_uns <= n_cuts and 20 * n_uns >= n_cuts, (n_uns, n_cuts)
