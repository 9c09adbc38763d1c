"""The multi-rank cut search on the device (tiebrush_amd/csrc/shard.hip: tbk_partial_stage_keys / _cands / _pack, tbk_shard_probe_max /
_next) on the hand-built scenes of cut_scenes.py, against the CPU model of cut_model.py: the sampled keys, targets and candidate lists
entry for entry, the verdict and the cuts, the table of the exchange — and every settled cut against the brute force
(cut_model.exact_cut), which knows nothing of lists.  tests/test_cut_model_cpu.py shows without a GPU that each scene sits on the edge
it is named for.  All comparisons are integer equality."""
import time

import numpy as np
import pytest

import cut_model as cm
import cut_scenes as cs
from dist_helpers import check_against_flat, split_tile
from helpers import tbk_debug
from test_gpu_dist import DeviceCompute

pytestmark = pytest.mark.gpu

INF, K = cm.INF, cm.K


@pytest.fixture(scope="module")
def comp():
    c = DeviceCompute()
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def ctx(comp):
    return comp.ctx


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int64))).cuda()


def _host(t):
    return t.cpu().numpy()


# ---- table scenes: tbk_partial_stage_cands on bare arrays ---------------------------------------------------------------------------------
def _check_stage_cands(ctx, ranks, allmeta, world):
    """every rank's targets and lists against the model; then the gathered lists through tbk_partial_stage_pack over the tiny tile of the
    choose scenes (partial_choose_k reads only the lists, partial_table_k only key and cuts): cuts, flag and table against the model,
    settled cuts against the brute force"""
    import torch
    allmeta_d = _dev(allmeta)
    first, cds = None, []
    for r, rank in enumerate(ranks):
        tg, cd = ctx.partial_stage_cands(_dev(rank.key), _dev(rank.emax), allmeta_d, world)
        want_tg, want_cd = cm.stage_cands(rank.key, rank.emax, allmeta, world)
        tg, cd = _host(tg), _host(cd)
        assert np.array_equal(tg, want_tg), (r, tg, want_tg)
        assert np.array_equal(cd, want_cd), (r, np.argwhere(cd != want_cd)[:8], cd[cd != want_cd][:8], want_cd[cd != want_cd][:8])
        first = tg if first is None else first
        assert np.array_equal(tg, first)              # every rank computes the same targets
        cds.append(_dev(cd))
    tile, fin, key, meta, words = _choose_base(ctx)
    _, _, tabx, cuts = ctx.partial_stage_pack(tile, fin, key, meta, torch.stack(cds), _dev(first), world, cs.FIRST_FIDX)
    want_allc = np.stack([cm.stage_cands(r.key, r.emax, allmeta, world)[1] for r in ranks])
    want_cuts, flag = cm.stage_choose(want_allc, first)
    assert np.array_equal(_host(cuts), want_cuts), (_host(cuts), want_cuts)
    assert np.array_equal(_host(tabx), cm.tabx(_host(key), want_cuts, words, flag, cs.N_FILES, cs.FIRST_FIDX, cs.CARRY))
    if not flag:
        pairs = [(r.key, r.endk) for r in ranks]
        assert want_cuts.tolist() == [cm.exact_cut(pairs, int(t)) for t in first]


@pytest.mark.parametrize("name", list(cs.TABLE))
def test_table_scene_lists_equal_the_model(ctx, name):
    s = cs.table(name)
    _check_stage_cands(ctx, s.ranks, s.allmeta, s.world)


@pytest.mark.parametrize("extra", [0, 1])
def test_give_up_limit(ctx, extra):
    """one bundle of 2^22 groups behind the target, built on the device: with nothing after it no horizon, with one more group the key of
    that group; the walk's 16,384 steps of one block are timed (pytest -s prints it)"""
    import torch
    head, first, n, far = cs.limit_scene(extra)
    key = torch.cat([_dev(head.key), first + torch.arange(n, dtype=torch.int64, device="cuda")])
    emax = torch.cat([_dev(head.emax), torch.full((n,), far, dtype=torch.int64, device="cuda")])
    allmeta = cs.rows_for_targets(2, [cs.LIMIT_TARGET])
    allmeta_d = _dev(allmeta)
    ctx.partial_stage_cands(_dev(cs.LIMIT_OTHER.key), _dev(cs.LIMIT_OTHER.emax), allmeta_d, 2)        # (first launch of the kernels: not timed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tg, cd = ctx.partial_stage_cands(key, emax, allmeta_d, 2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("give-up limit, %d groups behind the target: tbk_partial_stage_cands took %.1f ms" % (n, dt * 1e3))
    r0 = cs.limit_rank_np(extra)
    assert np.array_equal(_host(key), r0.key) and np.array_equal(_host(emax), r0.emax)
    want = cm.cands(r0.key, r0.emax, cs.LIMIT_TARGET)
    assert want[1] == (r0.key[3 + cm.LIMIT] if extra else INF)
    assert _host(tg).tolist() == [cs.LIMIT_TARGET] and np.array_equal(_host(cd)[0], want), (_host(cd)[0], want)
    # the verdict on these lists: without the horizon rank 1's start beyond the bundle's far end settles the cut, behind it nothing can
    tile, fin, dkey, meta, _ = _choose_base(ctx)
    _, cd1 = ctx.partial_stage_cands(_dev(cs.LIMIT_OTHER.key), _dev(cs.LIMIT_OTHER.emax), allmeta_d, 2)
    allc = torch.stack([cd, cd1])
    _, _, tabx, cuts = ctx.partial_stage_pack(tile, fin, dkey, meta, allc, tg, 2, cs.FIRST_FIDX)
    assert (_host(cuts).tolist(), int(_host(tabx)[6]) & 2) == (([INF], 2) if extra else ([K(8, cs.LIMIT_BEYOND)], 0))


# ---- choose scenes: tbk_partial_stage_pack on hand-written lists ---------------------------------------------------------------------------
_BASE = {}


def _choose_base(ctx):
    """the tiny tile on the device, collapsed, with its keys: (tile, fin, key, meta row with distinctive words, words per group)"""
    if "v" not in _BASE:
        from tiebrush_amd import api
        tile = cs.choose_tile()
        dt = api.to_device(tile, "cuda:0")
        fin = ctx.collapse(dt, want_coords=True, want_effend=True)
        key, emax, meta = ctx.partial_stage_keys(dt, fin, cs.FIRST_FIDX, cs.CARRY)
        meta = meta.clone()
        assert _host(meta)[64:].tolist() == [tile.n_files, cs.FIRST_FIDX, 0, cs.CARRY]
        meta[64] = cs.N_FILES
        rep = _host(fin["rep"]).astype(np.int64)
        words = (tile.cig_off[rep + 1].astype(np.int64) - tile.cig_off[rep].astype(np.int64))
        want_key, _ = cm.keys(sorted(zip(tile.tid[rep].tolist(), _host(fin["g_start"]).tolist(), _host(fin["g_end"]).tolist()), key=lambda g: g[:2]))
        assert np.array_equal(_host(key), want_key) and len(want_key) == 11 and sorted(set(words.tolist())) == [1, 2, 3]
        _BASE["v"] = (dt, fin, key.clone(), meta, words)
    return _BASE["v"]


@pytest.mark.parametrize("name", list(cs.CHOOSE))
def test_choose_scene_cuts_and_table_equal_the_model(ctx, name):
    s = cs.CHOOSE[name]
    tile, fin, key, meta, words = _choose_base(ctx)
    _, _, tabx, cuts = ctx.partial_stage_pack(tile, fin, key, meta, _dev(s.allcands), _dev(s.targets), s.world, cs.FIRST_FIDX)
    want_cuts, flag = cm.stage_choose(s.allcands, s.targets)
    assert np.array_equal(want_cuts, s.cuts) and flag == (2 if s.unsettled else 0)          # (the scene's own claim, as on the CPU)
    assert np.array_equal(_host(cuts), want_cuts), (_host(cuts), want_cuts)
    want = cm.tabx(_host(key), want_cuts, words, flag, cs.N_FILES, cs.FIRST_FIDX, cs.CARRY)
    got = _host(tabx)
    assert np.array_equal(got[:s.world * 3].reshape(s.world, 3), cm.table(_host(key), want_cuts, words))
    assert got[s.world * 3:].tolist() == [flag, cs.N_FILES, cs.FIRST_FIDX, cs.CARRY] and np.array_equal(got, want)


# ---- tile scenes and random scenes: the three stages as dist.partials_collapse queues them -----------------------------------------------
def _stages(ctx, s, after_keys=None):
    """collapse every rank's tile, run the three stages with the gathers in between; every array against the model.  Returns
    (ranks as the device ordered them, targets, cuts, flag); after_keys() runs behind every tbk_partial_stage_keys"""
    import torch
    from tiebrush_amd import api
    tile = s.tile()
    tiles, first = split_tile(tile, s.world)
    dtiles = [api.to_device(t, "cuda:0") for t in tiles]
    fins = [ctx.collapse(dt, want_coords=True, want_effend=True) for dt in dtiles]
    per, ranks = [], []
    for r in range(s.world):
        key, emax, meta = ctx.partial_stage_keys(dtiles[r], fins[r], first[r], 100 + r)
        if after_keys:
            after_keys()
        rep = _host(fins[r]["rep"]).astype(np.int64)
        got = list(zip(tiles[r].tid[rep].tolist(), _host(fins[r]["g_start"]).tolist(), _host(fins[r]["g_end"]).tolist()))
        assert sorted(got) == [tuple(g) for g in s.groups[r]]             # one group per read that passes
        rank = cs.rank_of(got)
        want_key, want_emax = cm.keys(got)
        assert np.array_equal(_host(key), want_key) and np.array_equal(_host(emax), want_emax), r
        assert np.array_equal(_host(meta), cm.meta_row(want_key, 1, first[r], 0, 100 + r)), r
        per.append((key, emax, meta))
        ranks.append(rank)
    want_tg, want_allc, _, want_cuts, flag = cs.verdict(s.name)
    allmeta = torch.stack([p[2] for p in per])
    cds = []
    for r in range(s.world):
        tg, cd = ctx.partial_stage_cands(per[r][0], per[r][1], allmeta, s.world)
        assert np.array_equal(_host(tg), want_tg) and np.array_equal(_host(cd), want_allc[r]), r
        cds.append(cd)
    allc = torch.stack(cds)
    for r in range(s.world):
        _, _, tabx, cuts = ctx.partial_stage_pack(dtiles[r], fins[r], per[r][0], per[r][2], allc, tg, s.world, first[r])
        assert np.array_equal(_host(cuts), want_cuts), r
        assert np.array_equal(_host(tabx), cm.tabx(ranks[r].key, want_cuts, np.ones(ranks[r].ng, np.int64), flag, 1, first[r], 100 + r)), r
    if not flag:
        pairs = [(k.key, k.endk) for k in ranks]
        assert want_cuts.tolist() == [cm.exact_cut(pairs, int(t)) for t in want_tg]
    return ranks, want_tg, want_cuts, flag


STAGE_SCENES = [n for n in cs.TILE_NAMED if n != "scan-tiles"] + ["staircase-settled", "staircase-given-up"]


def _scene(name):
    """the two staircases are the model's choice, made when the test runs: the longest the lists still settle, the shortest they give up"""
    if name.startswith("staircase-"):
        longest, shortest = cs.stair_edge()
        name = "staircase-%d" % (longest if name == "staircase-settled" else shortest)
    return cs.tile(name)


@pytest.mark.parametrize("name", STAGE_SCENES + cs.RANDOM)
def test_tile_scene_stages_equal_the_model(ctx, name):
    _stages(ctx, _scene(name))


@pytest.mark.parametrize("scan", ["lookback", "3pass"])
def test_running_maximum_across_scan_tiles(scan, monkeypatch):
    """more than 2 x 2,048 groups per rank and one early read that reaches across them, under each form of the scan engine: the look-back
    launches the scan's name once, the three-launch form twice"""
    from tiebrush_amd import api
    tbk_debug(monkeypatch, scan=scan)
    c = api.Context(0)
    c.set_profiling(True)
    try:
        launches = []
        ranks, _, _, flag = _stages(c, cs.tile("scan-tiles"), after_keys=lambda: launches.append(c.kernel_times()["partial_emax_scan"][1]))
        assert all(r.ng > 2 * 2048 for r in ranks) and flag == 2
        assert launches == [1 if scan == "lookback" else 2] * len(ranks), launches
    finally:
        c.close()


# ---- the rounds form: tbk_shard_probe_max / _next with one "file" per rank ---------------------------------------------------------------------
def _files(ranks):
    fo = np.concatenate([[0], np.cumsum([r.ng for r in ranks])]).astype(np.uint32)
    return fo, np.concatenate([r.key for r in ranks]), np.concatenate([r.emax for r in ranks])


def test_probes_equal_the_host_restatement(ctx):
    """an empty file between two full ones; cuts below every key, above every key, on a key three groups hold, 1 << 62; an m equal to a
    key — which _next must pass, all three holders of it —, m = -1, and an m beyond everything"""
    import torch
    from tiebrush_amd import dist
    B = cs.BIG_TID
    fo, key, emax = _files([cs._POS, cs.EMPTY, cs._POS2])
    dkey, demax = _dev(key), _dev(emax)
    cuts = np.array([K(B, 50), K(B, 500), K(B, 200), K(B, 130), K(B, 250), K(B, 251), INF], np.int64)
    m = _host(ctx.shard_probe_max(fo, dkey, demax, _dev(cuts), torch.full((len(cuts),), -1, dtype=torch.int64, device="cuda")))
    want_m = dist._probe_max_np(fo, key, emax, cuts)
    assert np.array_equal(m, want_m) and m[0] == -1 and m[1] == max(cs._POS.emax[-1], cs._POS2.emax[-1]) and m[2] == max(cs._POS.emax[2], cs._POS2.emax[0])
    ms = np.array([-1, K(B, 200), K(B, 150), K(B, 400), K(B, 399), K(B, 100) - 1, INF - 1], np.int64)
    ms = np.concatenate([ms, want_m])
    nxt = _host(ctx.shard_probe_next(fo, dkey, _dev(ms), torch.full((len(ms),), INF, dtype=torch.int64, device="cuda")))
    assert np.array_equal(nxt, dist._probe_next_np(fo, key, ms))
    assert nxt[:7].tolist() == [K(B, 100), K(B, 220), K(B, 200), INF, K(B, 400), K(B, 100), INF]


def _device_rounds(ctx, ranks, t):
    import torch
    fo, key, emax = _files(ranks)
    dkey, demax = _dev(key), _dev(emax)
    p = _dev([t])
    for _ in range(200):
        m = ctx.shard_probe_max(fo, dkey, demax, p, torch.full((1,), -1, dtype=torch.int64, device="cuda"))
        if int(m[0]) < int(p[0]) or int(p[0]) == INF:
            return int(p[0])
        p = ctx.shard_probe_next(fo, dkey, m, torch.full((1,), INF, dtype=torch.int64, device="cuda")).clone()
    raise AssertionError("the walk did not end")


@pytest.mark.parametrize("name", ["touching-reads", "two-references", "filtered-rank", "staircase-given-up", "random-1", "random-3"])
def test_device_rounds_walk_to_the_exact_cut(ctx, name):
    s = _scene(name)
    ranks = s.ranks()
    tg = cs.verdict(s.name)[0]
    pairs = [(r.key, r.endk) for r in ranks]
    for t in tg:
        assert _device_rounds(ctx, ranks, int(t)) == cm.exact_cut(pairs, int(t)) == cm.rounds_cut([(r.key, r.emax) for r in ranks], int(t))[0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAGE_SCENES + ["scan-tiles"] + cs.RANDOM[:8])
def test_loopback_takes_the_rounds_exactly_when_the_model_says_so(comp, name):
    import torch
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, dist
    s = _scene(name)
    tile = s.tile()
    flat = orc.collapse(tile)
    tiles, first = split_tile(tile, s.world)
    dtiles = [api.to_device(t, "cuda:0") for t in tiles]
    sts = [dict() for _ in range(s.world)]
    res = dist.run_loopback(comp, dtiles, first, device_chain=True, cut_search="lists", per_rank=[dict(stats=sts[r]) for r in range(s.world)])
    for r in res:
        for f in ("tid", "start", "end", "rep_fidx", "rep_idx", "yc", "yx", "yd"):
            v = getattr(r, f)
            setattr(r, f, v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
    check_against_flat(res, tile, flat)
    flag = cs.verdict(s.name)[4]
    if flag:
        assert all(st["cut_rounds"] >= 1 for st in sts), sts
    else:
        assert all(st["cut_rounds"] == 0 for st in sts), sts
