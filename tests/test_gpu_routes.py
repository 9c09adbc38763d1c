"""The collapse driver's first route on the device (collapse.hip: tbk_collapse_device, collapse_plan.hpp) against the CPU model of the
decision (route_model.py), on the smallest synthetic tiles at which the decision flips: tbk_last_route names the model's route and the
result is the oracle's.  The thresholds no small tile reaches (8 Mi records, 2^30 records or CIGAR words) are the CPU test's."""
import numpy as np
import pytest

import route_model as rm
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

PATH, SORT = {"sort": 1, "window": 2}, {"radix": 1, "runs": 2}   # TBK_DEBUG's values as TbkDebug holds them


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _plain(n_files, reads):
    from tiebrush_amd import synth
    tile = synth.make_tile(n_files, reads, "c3", n_loci=300)
    assert tile.n_records == n_files * reads
    return tile


def _carried(tile, tbm, prio):
    """flags `tbm` of the files as TieBrush-merged and gives every record carried tags (integral YC) and, prio, an explicit priority"""
    n = tile.n_records
    rng = np.random.default_rng(7)
    tile.tbmerged = np.asarray(tbm, np.uint8)
    tile.yc_in = rng.integers(1, 9, n).astype(np.float64)
    tile.yx_in = rng.integers(1, 4, n).astype(np.int64)
    tile.yd_in = rng.integers(0, 50, n).astype(np.int64)
    if prio:
        tile.prio_hi = rng.integers(0, 1000, n).astype(np.uint64)
        tile.prio_lo = np.arange(n).astype(np.uint64)
    return tile


TILES = {
    "3x2000": lambda: _plain(3, 2000),
    "65x1008": lambda: _plain(65, 1008),                                  # 65 520 records: below the many-files threshold
    "65x1009": lambda: _plain(65, 1009),                                  # 65 585: above it
    "partials-65535": lambda: _carried(_plain(3, 21845), [1, 1, 1], True),
    "partials-65536": lambda: _carried(_plain(4, 16384), [1, 1, 1, 1], True),
    "one-merged-file": lambda: _carried(_plain(3, 2000), [0, 1, 0], False),
}
# (tile, debug keys, the route the case is here for — the model must say the same)
CASES = [("3x2000", {}, "sort"), ("3x2000", dict(path="window"), "raw"), ("3x2000", dict(path="window", raw="0"), "compacted"),
         ("3x2000", dict(path="sort"), "sort"), ("3x2000", dict(sort="radix"), "sort"), ("3x2000", dict(sort="runs"), "sort"),
         ("65x1008", {}, "sort"), ("65x1009", {}, "raw"),
         ("partials-65535", {}, "sort"), ("partials-65536", {}, "raw"),
         ("one-merged-file", dict(path="window"), "sort")]


@pytest.fixture(scope="module")
def scenes():
    """tile name -> (tile, the oracle's result), made once"""
    from dist_helpers import OracleCompute
    made = {}

    def get(name):
        if name not in made:
            tile = TILES[name]()
            made[name] = (tile, OracleCompute().collapse(tile))
        return made[name]
    return get


def _model(tile, keys):
    tb = np.asarray(tile.tbmerged)
    p = rm.plan(n=tile.n_records, cig=len(tile.cig), k=tile.n_files, tbm=rm.TBM_ALL if tb.all() else rm.TBM_SOME if tb.any() else rm.TBM_NONE,
                prio=tile.prio_hi is not None, carried=tile.yc_in is not None and tile.yx_in is not None and tile.yd_in is not None,
                path=PATH.get(keys.get("path"), 0), raw=int(keys.get("raw", -1)), sort=SORT.get(keys.get("sort"), 0))
    return p


@pytest.mark.parametrize("name,keys,route", CASES, ids=["%s-%s" % (n, ",".join("%s=%s" % kv for kv in k.items()) or "no-key") for n, k, _ in CASES])
def test_first_route_and_result(ctx, monkeypatch, scenes, name, keys, route):
    from tiebrush_amd import api
    tile, want = scenes(name)
    p = _model(tile, keys)
    assert rm.FORM[int(p["route"])] == route
    assert bool(p["part"]) == (name == "partials-65536")                       # the PART form: from 65 536 group partials on
    tbk_debug(monkeypatch, **keys)
    got = api.to_numpy(ctx.collapse(tile))
    r = ctx.collapse_route()
    assert r == dict(form=route, reseeds=0, raw_handed_back=False, big_bucket=False)
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in ("rep", "yc", "yx", "yd", "g_start", "g_end"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
