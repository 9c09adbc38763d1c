"""The coverage kernels (tiebrush_amd/csrc/cov.hip) on hand-placed reads: every scene of tests/cov_scenes.py — a feature on the first or
last base of a tile, a bundle decision on a thread, wave, row or block seam of the record passes, a junction table or home exactly
full, the accumulator switch — through every interval chain and junction route, against the oracle, bit for bit.  No tolerances.
What each scene is, and that it is what it says, is tests/test_cov_scenes_cpu.py's business; here every run also asserts, through the
labels of the kernels it launched, that it took the path it is there for."""
import numpy as np
import pytest

import cov_scenes as cs
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

IV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val")
J_KEYS = ("j_tid", "j_start", "j_end", "j_strand", "j_val")
S_KEYS = ("s_tid", "s_start", "s_end", "s_count", "s_heat")
CHAINS = ("lean", "legacy", "scan", "refused")
HOOKS = ("cov_legacy", "cov_bundle_scan", "cov_tile_cap", "junc_radix", "no_junc_agg", "jh_cap")
NS = 5


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


def _hooks(monkeypatch, **kw):
    """exactly these hooks, every other one of this file off"""
    tbk_debug(monkeypatch, **{k: kw.get(k) for k in HOOKS})


_CASES = {}


def _case(group, name, value, variant="int"):
    """one scene as the GPU gets it — host arrays with flags and unmapped records between the reads (the compaction is no identity),
    and the mapped records alone without flags for the device (the IDENT instances) — with the oracle's answer; the integral form,
    which every chain runs, is built once"""
    key = (group, name, value, variant)
    case = _CASES.get(key)
    if case is None:
        from oracle import oracle_ffi as orc
        if group == "order":
            cin = cs.order(value)[0]
        elif group == "side":
            cin = cs.j2(value)[0]
        else:
            cin = cs.build(group, name, value)[0]
        if variant == "frac":
            cin = cs.with_yc(cin, lambda y: y + 0.25)
        if variant == "sample":
            cin = cs.mk(cs.records(cin), cs.sample_yx(cin.n_records, NS))
        host = cs.with_unmapped(cin) if cin.n_records < 20000 else cin
        dev = cs.mk(cs.records(cin), cin.yx)
        dev.flag = None
        lay = cs.layout(cin)
        spilling = np.flatnonzero(lay["cs"] % cs.W + (lay["end"] - lay["start"] + 1) > cs.W)
        want = orc.coverage(host, num_samples=NS) if variant == "sample" else orc.coverage(host)
        case = dict(host=host, dev=dev, want=want, ntiles=lay["ntiles"], n_spilling=len(spilling),
                    n_pieces=sum(len(cs.spill_pieces(cin, lay, int(j))) for j in spilling),
                    ordered=bool(np.any(cin.yc != np.floor(cin.yc)) or np.any(np.abs(cin.yc) >= 2.0**30)))
        if variant == "int":
            _CASES[key] = case
    return case


def _inputs(case):
    from tiebrush_amd import api
    yield "host", case["host"]
    yield "device", api.to_device(case["dev"], "cuda:0")


def _compare(got, want, keys, counts, what):
    for k in counts:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


def _coverage(ctx, case, what, **kw):
    """both inputs through ctx.coverage against the oracle; yields the labels of the kernels each run launched"""
    from tiebrush_amd import api
    keys = (IV_KEYS if kw.get("want_cov", True) else ()) + (J_KEYS if kw.get("want_junc", True) else ())
    counts = (("n_bases", "span_bases", "n_intervals") if kw.get("want_cov", True) else ()) + (("n_junctions",) if kw.get("want_junc", True) else ())
    for where, cin in _inputs(case):
        got = api.to_numpy(ctx.coverage(cin, **kw))
        ran = set(ctx.kernel_times())
        _compare(got, case["want"], keys, counts, what + (where,))
        yield where, ran


def _assert_chain(case, chain, ran, what):
    """the labels of the TBK_LAUNCH calls: cov_place = the lean chain's numbering pass, cov_cp_gather = the general chain's gather of
    the change points, cov_spill_fill = the spill pieces' bins (lean: launched for any record whose span leaves its home tile; general:
    for any piece), cov_tile_ordered = the per-base kernel"""
    if case["ordered"]:       # fractional YC, or one of 2^30 and more: the general chain with the ordered tile kernel, whatever the hooks
        assert "cov_tile_ordered" in ran and "cov_cp_gather" in ran and "cov_place" not in ran and "cov_tile" not in ran, (what, ran)
        assert ("cov_spill_fill" in ran) == (case["n_pieces"] > 0), (what, ran)
        return
    assert "cov_tile" in ran and "cov_tile_ordered" not in ran, (what, ran)
    if chain in ("lean", "not-refused"):
        assert "cov_place" in ran and "cov_cp_gather" not in ran, (what, ran)
        assert ("cov_spill_fill" in ran) == (case["n_spilling"] > 0), (what, ran)
    elif chain == "refused":      # the lean chain started, refused, and the general chain took over
        assert "cov_place" in ran and "cov_cp_gather" in ran, (what, ran)
        assert ("cov_spill_fill" in ran) == (case["n_pieces"] > 0), (what, ran)
    else:
        assert "cov_cp_gather" in ran and "cov_place" not in ran, (what, ran)
        assert ("cov_spill_fill" in ran) == (case["n_pieces"] > 0), (what, ran)


def _set_chain(monkeypatch, chain, case):
    if chain == "lean":
        _hooks(monkeypatch)
    elif chain == "legacy":
        _hooks(monkeypatch, cov_legacy="1")
    elif chain == "scan":
        _hooks(monkeypatch, cov_bundle_scan="1")
    elif chain == "refused":            # tile tables of exactly ntiles entries do not hold the input ...
        _hooks(monkeypatch, cov_tile_cap=case["ntiles"])
    elif chain == "not-refused":        # ... of ntiles + 1 they do
        _hooks(monkeypatch, cov_tile_cap=case["ntiles"] + 1)


INTERVAL = list(cs.INTERVAL_SCENES)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name", INTERVAL)
def test_interval_scenes(ctx, monkeypatch, name, chain):
    """tile, record-seam, accumulator and top-of-range scenes on the lean chain, the general chain, the general chain with the bundles
    of the look-back scan, and the lean chain refusing the input for its tile tables (ntiles entries; ntiles + 1 must not refuse)"""
    for value in cs.INTERVAL_SCENES[name]:
        case = _case("interval", name, value)
        for ch in ((chain, "not-refused") if chain == "refused" else (chain,)):
            _set_chain(monkeypatch, ch, case)
            for where, ran in _coverage(ctx, case, (name, value, ch)):
                _assert_chain(case, ch, ran, (name, value, ch, where))


@pytest.mark.parametrize("name", INTERVAL)
def test_interval_scenes_fractional(ctx, monkeypatch, name):
    """the same scenes with YC + 0.25: the ordered per-base kernel, the junction sums in record order"""
    _hooks(monkeypatch)
    for value in cs.INTERVAL_SCENES[name]:
        case = _case("interval", name, value, "frac")
        assert case["ordered"]
        for where, ran in _coverage(ctx, case, (name, value, "frac")):
            _assert_chain(case, "lean", ran, (name, value, "frac", where))
            assert ("junc_fill" in ran) == (case["want"]["n_junctions"] > 0), (name, value, ran)


@pytest.mark.parametrize("name", INTERVAL)
def test_interval_scenes_sample_track(ctx, monkeypatch, name):
    """the same scenes through the sample track: YX = 1 + (7 i mod ns) and one YX that is present and 0"""
    from tiebrush_amd import api
    _hooks(monkeypatch)
    for value in cs.INTERVAL_SCENES[name]:
        case = _case("interval", name, value, "sample")
        want = case["want"]
        for where, cin in _inputs(case):
            got = api.to_numpy(ctx.sample(cin, NS, cap_intervals=want["n_sample"] + 1000))
            ran = set(ctx.kernel_times())
            _compare(got, want, S_KEYS, ("n_sample",), (name, value, "sample", where))
            assert "sample_tile" in ran and "cov_tile" not in ran and "cov_tile_ordered" not in ran, (name, value, ran)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_order_scene(ctx, monkeypatch, reverse):
    """300 fractional reads across one seam, one intron in all of them: per-base sums and the junction sum in record order, for the
    record order and for its reverse (the two answers differ in their last bits: test_cov_scenes_cpu.py)"""
    _hooks(monkeypatch)
    case = _case("order", "order", reverse)
    for where, ran in _coverage(ctx, case, ("order", reverse)):
        assert "cov_tile_ordered" in ran and "junc_fill" in ran and "cov_spill_fill" in ran, ran
        assert "junc_agg" not in ran and "junc_sum" not in ran, ran
    for where, ran in _coverage(ctx, case, ("order", reverse, "junctions only"), want_cov=False):
        assert "junc_fill" in ran and "cov_tile_ordered" not in ran, ran


ROUTES = ("default", "junc_radix", "no_junc_agg", "jh_cap", "junctions-only", "intervals-only")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(cs.JUNC))
def test_junction_scenes(ctx, monkeypatch, name, route):
    """block tables, homes and their wave / block sorts (default), the radix sort (junc_radix; and behind a home that is too full:
    J1 at 1025 and 1100, or any home of more than 64 items with jh_cap=2), plain items without block sums (no_junc_agg); each branch
    alone"""
    _hooks(monkeypatch, **{"junc_radix": {"junc_radix": "1"}, "no_junc_agg": {"no_junc_agg": "1"}, "jh_cap": {"jh_cap": "2"}}.get(route, {}))
    kw = {"junctions-only": dict(want_cov=False), "intervals-only": dict(want_junc=False)}.get(route, {})
    for value in cs.JUNC[name]:
        cin, claims = cs.build("junction", name, value)
        case = _case("junction", name, value)
        most = max(cs.junction_items(cin, cs.layout(cin)).values())        # items in the fullest home
        for where, ran in _coverage(ctx, case, (name, value, route), **kw):
            what = (name, value, route, where, ran)
            if route == "intervals-only":
                assert not [k for k in ran if k.startswith("junc_")], what
                continue
            if route == "no_junc_agg":
                assert "junc_fill" in ran and "junc_agg" not in ran, what
                continue
            assert "junc_agg" in ran and "junc_fill" not in ran, what
            if route == "junc_radix":
                assert "junc_iota" in ran and "junc_sort" not in ran, what
            else:                      # the homes, and the radix sort behind them only when one is too full
                assert "junc_sort" in ran, what
                assert ("junc_iota" in ran) == (most > (64 if route == "jh_cap" else cs.JH_REC)), what
        if name == "j1":
            assert most == value


def test_j2_on_the_side_context(ctx, monkeypatch):
    """66000 records and both tracks wanted: the junction branch runs on the side context while the intervals are built; alone it
    runs inline — the same six sums"""
    _hooks(monkeypatch)
    case = _case("side", "j2", cs.J2_SIDE)
    assert case["host"].n_records >= 2**16
    for where, ran in _coverage(ctx, case, ("j2", cs.J2_SIDE)):
        assert "junc_agg" in ran and "junc_sort" in ran and "junc_iota" not in ran and "cov_place" in ran, ran
    for where, ran in _coverage(ctx, case, ("j2", cs.J2_SIDE, "junctions only"), want_cov=False):
        assert "junc_agg" in ran and "cov_place" not in ran, ran
