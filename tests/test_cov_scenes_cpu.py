"""The scenes of tests/cov_scenes.py before the GPU sees them: the per-base model and the oracle agree on every one, bit for bit, and every
scene is what it claims to be (a later change of a builder cannot hollow a scene out: the claims and the realised offsets are
asserted here, on the CPU)."""
import numpy as np
import pytest

import cov_scenes as cs

KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
SAMPLE_KEYS = ("s_tid", "s_start", "s_end", "s_count", "s_heat")
COUNTS = ("n_bases", "span_bases", "n_intervals", "n_junctions", "n_sample")
NS = 5


def _agree(cin):
    """model == oracle on every key, the sample track (YX = 1 + (7 i mod NS), one present 0) included"""
    from oracle import oracle_ffi as orc
    c = cs.mk(cs.records(cin), cs.sample_yx(cin.n_records, NS))
    want = orc.coverage(c, num_samples=NS)
    got = cs.model(c, NS)
    for k in COUNTS:
        assert got[k] == want[k], k
    for k in KEYS + SAMPLE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return got


ALL = [("interval", n) for n in cs.INTERVAL_SCENES] + [("junction", n) for n in cs.JUNC]


@pytest.mark.parametrize("group,name", ALL, ids=[n for _, n in ALL])
def test_model_equals_oracle_and_claims_hold(group, name):
    table = cs.INTERVAL_SCENES if group == "interval" else cs.JUNC
    for value in table[name]:
        cin, claims = cs.build(group, name, value)
        assert cs.check_claims(claims) == [], (name, value)
        _agree(cin)
        if cin.n_records < 3000 or value in (1, 4096):
            _agree(cs.with_unmapped(cin))       # the unmapped records change nothing
        if group == "interval" and name in cs.TILE:
            _agree(cs.with_yc(cin, lambda y: y + 0.25))


@pytest.mark.parametrize("name", list(cs.SWEPT))
def test_sweeps_reach_the_seam_and_both_neighbours(name):
    """over a scene's sweep the feature sits on a tile's last base, on the next tile's first base and on the base behind it, for
    k = 1 and for k = 2"""
    for k in cs.SWEEP_K:
        offs = set()
        for value, thunk in cs.SWEPT[name].items():
            if value[0] == k:
                claims = cs.build("interval", name, value)[1]
                assert claims["offset"] == claims["want_offset"]
                offs.add(claims["offset"] - k * cs.W)
        assert {-1, 0, 1} <= offs, (name, k, offs)


def test_seam_records_are_the_seams_of_the_bundle_passes():
    """thread seams (4 records), wave seams (256), row seams (1024), block seams (4096), each with both neighbours, and the input's
    last record"""
    ks = set(cs.SEAM_K)
    for seam_ in (4, 256, 1024, 4096):
        assert {seam_ - 1, seam_, seam_ + 1} <= ks, seam_
    assert {1, 8191, 8192, cs.SEAM_N - 1} <= ks and cs.SEAM_N == 2 * cs.CB_TILE + 5
    for event in cs.SEAM_EVENTS:
        assert set(cs.SEAM[event]) == ks


def test_t8_reaches_both_sides_of_the_spill_window():
    tiles = set()
    for value in cs.TILE["t8"]:
        claims = cs.build("interval", "t8", value)[1]
        tiles.update(t - claims["tbase"] for t in claims["spill_tiles"])
    assert {cs.SW - 1, cs.SW, cs.SW + 1} <= tiles


def test_order_scene_sums_depend_on_the_order():
    """the two record orders give depths and a junction sum that differ — in the last bits: a kernel that adds in another order than the
    records' cannot pass both"""
    (a, ca), (b, cb) = cs.order(False), cs.order(True)
    assert cs.check_claims(ca) == [] and cs.check_claims(cb) == []
    ra, rb = _agree(a), _agree(b)
    assert ra["n_junctions"] == rb["n_junctions"] == 1
    va, vb = float(ra["j_val"][0]), float(rb["j_val"][0])
    assert va != vb and abs(va - vb) <= 8 * np.spacing(va)
    # the depths behind the seam (reference position F_POS + 150), where the 300 reads arrive as spill pieces
    fa, fb = (r["iv_val"][(r["iv_tid"] == cs.F_TID) & (r["iv_start"] >= cs.F_POS + 150)] for r in (ra, rb))
    assert len(fa) and (len(fa) != len(fb) or np.any(fa != fb))
    assert abs(fa.max() - fb.max()) <= 8 * np.spacing(fa.max())
    assert np.any(a.yc != np.floor(a.yc))


def test_j2_side_variant_is_large_enough_for_the_fork():
    assert cs.J2_SIDE >= 2**16
    cin, claims = cs.j2(cs.J2_SIDE)
    assert cs.check_claims(claims) == [] and cin.n_records == cs.J2_SIDE
    _agree(cin)


def test_layout_of_a_known_input():
    """layout() itself, on numbers worked out by hand: two bundles on one reference (the second adjacent), an unmapped record, a
    record without a reference base, a second reference"""
    M, N, S, I = cs.M, cs.N, cs.S, cs.I
    cin = cs.mk([(0, 10, 0, [(50, M)], 1.0, "."), (0, 20, 4, [(50, M)], 1.0, "."), (0, 30, 0, [(10, M), (100, N), (10, M)], 1.0, "+"),
                 (0, 150, 0, [(5, M)], 1.0, "."), (0, 155, 0, [(3, S), (2, I)], 1.0, "."), (1, 0, 0, [(8192, M)], 1.0, ".")])
    lay = cs.layout(cin)
    assert lay["idx"].tolist() == [0, 2, 3, 4, 5]
    assert lay["head"].tolist() == [True, False, True, True, True]
    assert lay["span"].tolist() == [140, 5, 0, 8192] and lay["b_off"].tolist() == [0, 140, 145, 145, 8337]
    assert lay["cs"].tolist() == [0, 20, 140, 145, 145] and lay["S"] == 8337 and lay["ntiles"] == 2
    assert cs.pieces(cin, lay, 4) == [(0, 145, 8047), (1, 0, 145)] and cs.spill_pieces(cin, lay, 4) == [(1, 0, 145)]
    assert cs.is_spilling(lay, 4) and not cs.is_spilling(lay, 1)
    assert cs.exons(30, [(10, M), (100, N), (10, M)]) == [(31, 40), (141, 150)]
    assert cs.exons(9, [(24, M), (7, N), (2, S)]) == [(10, 33), (41, 40)]
