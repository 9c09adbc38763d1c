"""The comparator of the full-size GPU tests (`tests/scale_helpers.py`), on the CPU: single planted faults that the
size-independent properties of `test_gpu_scale._properties` let through and the array comparison must name; the oracle's
tiecov split by reference against the single call; the host memory formula against the bytes really allocated."""
import copy

import numpy as np
import pytest

import scale_helpers as sh


@pytest.fixture(scope="module")
def case():
    from oracle import oracle_ffi as orc
    from tiebrush_amd import synth, synth_dev
    tile = synth_dev.tile_to_host(synth_dev.make_tile_device(6, 30_000, "c3", device="cpu", n_loci=300))
    want = orc.collapse(tile, want_rec_group=True, strategy=sh.STRATEGY["clip"])
    cin = synth.collapsed_to_cov_input(tile, want)
    return tile, want, cin, orc.coverage(cin)


def _properties_numpy(tile, res, cov):
    """what `_properties` asserts of YD, of the representative and of tiecov, in numpy"""
    g = res["n_groups"]
    rep = res["rep"].astype(np.int64)
    assert int(res["yd"].min()) >= 0
    rg = res["rec_group"].astype(np.int64)
    assert np.array_equal(np.bincount(rg[rg >= 0], minlength=g).astype(np.float64), res["yc"])
    assert np.array_equal(rg[rep], np.arange(g))                       # the representative is a member of its group
    co = tile.cig_off.astype(np.int64)
    mlen = np.where((tile.cig & 0xF) == 0, tile.cig >> 4, 0).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(mlen)])
    mb = csum[co[rep + 1]] - csum[co[rep]]
    area = ((cov["iv_end"] - cov["iv_start"]).astype(np.float64) * cov["iv_val"]).sum()
    assert float(area) == float((mb.astype(np.float64) * res["yc"].astype(np.float32).astype(np.float64)).sum())
    assert cov["n_bases"] == int(mb.sum())


def _fails(tile, got, want, cov_got, cov_want):
    with pytest.raises(AssertionError) as e:
        sh.compare_results(tile, got, want, cov_got, cov_want, desc='synth_dev.make_tile_device(6, 30_000, "c3", n_loci=300)')
    return str(e.value)


def test_equal_results_compare_equal(case):
    tile, want, cin, cov = case
    assert len(np.unique(cov["iv_tid"])) == 3 and cov["n_junctions"] > 0 and int(want["yd"].max()) > 0
    _properties_numpy(tile, want, cov)
    sh.compare_results(tile, copy.deepcopy(want), want, copy.deepcopy(cov), cov)


def test_yd_off_by_one_passes_the_properties_and_fails_the_comparison(case):
    tile, want, cin, cov = case
    got = copy.deepcopy(want)
    i = int(np.flatnonzero(want["yd"] > 0)[len(want["yd"]) // 7 % int((want["yd"] > 0).sum())])
    got["yd"][i] += 1
    _properties_numpy(tile, got, cov)
    msg = _fails(tile, got, want, cov, cov)
    assert msg.startswith("yd: 1 of %d entries differ, first at index %d\n" % (want["n_groups"], i))
    r = int(want["rep"][i])
    assert "got %d, oracle %d" % (want["yd"][i] + 1, want["yd"][i]) in msg
    assert "oracle: group %d = (tid %d, g_start %d, g_end %d, strand %s), rep %d in file %d" % (
        i, tile.tid[r], want["g_start"][i], want["g_end"][i], chr(tile.strand[r]), r, r // 30_000) in msg
    assert "tile_to_host(tile, window=(%d, 0, %d))" % (tile.tid[r], want["g_start"][i] + sh.WINDOW_MARGIN) in msg
    assert "make_tile_device(6, 30_000" in msg


def test_second_member_as_representative_passes_the_properties_and_fails_the_comparison(case):
    tile, want, cin, cov = case
    got = copy.deepcopy(want)
    rg = want["rec_group"]
    i = int(np.flatnonzero(want["yc"] >= 3)[5])
    members = np.flatnonzero(rg == i)
    other = int(members[members != want["rep"][i]][0])
    assert other // 30_000 != int(want["rep"][i]) // 30_000 or other > int(want["rep"][i])
    got["rep"][i] = other
    _properties_numpy(tile, got, cov)
    msg = _fails(tile, got, want, cov, cov)
    assert msg.startswith("rep: 1 of %d entries differ, first at index %d\n" % (want["n_groups"], i))
    assert "got %d, oracle %d" % (other, want["rep"][i]) in msg
    assert "got: group %d" % i in msg and "rep %d in file %d" % (other, other // 30_000) in msg
    assert "rep %d in file %d" % (want["rep"][i], want["rep"][i] // 30_000) in msg


def test_changed_junction_value_fails_the_comparison(case):
    tile, want, cin, cov = case
    cg = copy.deepcopy(cov)
    j = cov["n_junctions"] // 2
    cg["j_val"][j] += 1.0
    msg = _fails(tile, want, want, cg, cov)
    assert msg.startswith("j_val: 1 of %d entries differ, first at index %d\n" % (cov["n_junctions"], j))
    assert "row %d = (tid %d, start %d, end %d)" % (j, cov["j_tid"][j], cov["j_start"][j], cov["j_end"][j]) in msg
    assert "window=(%d, 0, %d)" % (cov["j_tid"][j], cov["j_start"][j] + sh.WINDOW_MARGIN) in msg


def test_length_and_record_differences_are_named(case):
    tile, want, cin, cov = case
    got = copy.deepcopy(want)
    got["yx"] = got["yx"][:-2]
    msg = _fails(tile, got, want, cov, cov)
    assert msg.startswith("yx: 2 of %d entries differ, first at index %d " % (want["n_groups"], want["n_groups"] - 2))
    got = copy.deepcopy(want)
    r = tile.n_records // 3
    got["rec_group"][r] += 1
    msg = _fails(tile, got, want, cov, cov)
    assert msg.startswith("rec_group: 1 of %d entries differ, first at index %d\n" % (tile.n_records, r))
    assert "record %d = (tid %d, pos %d, file %d)" % (r, tile.tid[r], tile.pos[r], r // 30_000) in msg
    got = copy.deepcopy(want)
    got["n_passed"] += 1
    assert _fails(tile, got, want, cov, cov).startswith("n_passed: got")


def test_coverage_per_reference_equals_the_single_call(case):
    tile, want, cin, cov = case
    assert len(np.unique(cin.tid)) == 3
    parts = sh.oracle_coverage(cin, split=True)
    for k in sh.COV_KEYS:
        assert parts[k].dtype == cov[k].dtype and np.array_equal(parts[k], cov[k]), k
    for k in ("n_intervals", "n_junctions", "n_bases", "span_bases"):
        assert parts[k] == cov[k], k
    whole = sh.oracle_coverage(cin)                      # far below 2^32 entries: one call
    assert all(np.array_equal(whole[k], cov[k]) for k in sh.COV_KEYS)
    assert sh.cov_capacity(2**30, 2**30)[0] >= 2**32 > sh.cov_capacity(2**29, 2**29)[0]


def test_memory_formula_equals_the_bytes_allocated(case):
    tile, want, cin, cov = case
    n, ncig, g, gcig = tile.n_records, len(tile.cig), want["n_groups"], len(cin.cig)
    ni, nj = cov["n_intervals"], cov["n_junctions"]
    assert sh.tile_bytes(n, ncig, tile.n_files) == sh.nbytes_of(tile)
    assert sh.groups_bytes(n, g) == sh.nbytes_of(want)
    assert sh.cov_input_bytes(g, gcig) == sh.nbytes_of(cin)
    assert sh.cov_bytes(ni, nj) == sh.nbytes_of({k: cov[k] for k in sh.COV_KEYS})
    # the oracle binding's own allocations: the capacity arrays it hands to the C side
    from oracle import oracle_ffi as orc
    seen = []
    real = np.zeros

    def spy(shape, dtype=float, **kw):
        a = real(shape, dtype, **kw)
        seen.append(a.nbytes)
        return a

    orc.np.zeros = spy
    try:
        orc.collapse(tile, want_rec_group=True, strategy=sh.STRATEGY["clip"])
        assert sum(seen) == sh.collapse_work_bytes(n) - 16 * (n + 1)        # (the 16 B per record are malloc'ed inside tbo_collapse)
        del seen[:]
        orc.coverage(cin)
        assert sum(seen) == sh.cov_work_bytes(g, gcig)
    finally:
        orc.np.zeros = real
    need = sh.memory_need(n, ncig, tile.n_files, g, gcig, ni, nj)
    held = sh.nbytes_of(tile) + 2 * sh.nbytes_of(want) + sh.nbytes_of({k: cov[k] for k in sh.COV_KEYS})
    assert need >= held + max(sh.collapse_work_bytes(n), sh.nbytes_of(cin) + sh.cov_work_bytes(g, gcig))
    assert sh.memory_need(n, ncig, tile.n_files, g, gcig, ni, nj, cov_share=0.5) <= need
    assert sh.host_memory_budget() > 0


def test_chain_stats_on_a_hand_made_tile():
    """Two files on one reference, strand '.': file 0 holds reads at 100, 150 (overlapping: one chain of 2) and 1000 (beyond
    every end + 1: a new chain); file 1 holds 100 and 1000.  Both strand lists of a file carry a '.' item."""
    from oracle import oracle_ffi as orc
    from helpers import tile_from_records
    M = 0
    recs = [[(0, 100, 0, 60, ".", 1, [(100, M)]), (0, 150, 0, 60, ".", 1, [(100, M)]), (0, 1000, 0, 60, ".", 1, [(50, M)])],
            [(0, 100, 0, 60, ".", 1, [(100, M)]), (0, 1000, 0, 60, ".", 1, [(50, M)])]]
    tile = tile_from_records(recs)
    want = orc.collapse(tile, want_rec_group=True)
    assert want["n_groups"] == 3
    st = sh.chain_stats(tile, want)
    assert st == dict(items=2 * (3 + 2), chains=2 * (2 + 2), longest=2)


def test_prefix_window_holds_the_asked_share():
    from tiebrush_amd import synth_dev
    tile = synth_dev.make_tile_device(4, 20_000, "c2", device="cpu", n_loci=300)
    w = sh.prefix_window(tile, 0.2)
    small = synth_dev.tile_to_host(tile, window=w)
    assert w[0] == 0 and w[1] == 0 and 0.15 * tile.n_records < small.n_records <= 0.2 * tile.n_records
    assert sh.prefix_window(tile, 0.99)[2] == int(tile.pos[tile.tid == 0].max()) + 1
