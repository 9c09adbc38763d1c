"""The scenes of stream_scenes.py are what they claim, on the CPU: the model of tbk_cov_stream_push (stream_model.py) reports, push by
push, what each scene states by hand; the views, one after the other, give the rows of the uncut stream in cov_scenes' per-base model of
tiecov (the seam argument of DESIGN.md 4k, checked rather than believed); and the scenes sit on the edges the kernels cut their work by."""
import os
import re

import numpy as np
import pytest

import cov_scenes as cs
import stream_model as sm
import stream_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ss.scenes()
ROW_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val", "s_tid", "s_start", "s_end", "s_count", "s_heat")


def test_block_size_is_the_kernels():
    txt = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "cb_tiles.hpp")).read()
    m = re.search(r"CB_NT = (\d+), CB_ROWS = (\d+), CB_TILE = CB_NT \* 4 \* CB_ROWS;", txt)
    assert m and int(m.group(1)) * 4 * int(m.group(2)) == ss.T
    assert {1, 63, 64, 65, ss.T - 1, ss.T + 1, 3 * ss.T + 1} <= set(ss.SIZES)


def test_names_are_unique():
    assert len({s.name for s in SCENES}) == len(SCENES)


@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_model_reports_what_the_scene_states(scene):
    got, left = sm.run(scene.pushes)
    assert [i for _, i in got] == scene.expect
    nc = 0
    s = sm.Stream()
    for (cin, final, seen), (view, inf) in zip(scene.pushes, got):
        before = list(s.carry)
        s.push(cin, final, seen)
        mapped = [r for r in sm.tile_records(cin, seen) if not (r[0][2] & 4)]
        assert view + s.carry == before + mapped                     # nothing lost, nothing reordered, no unmapped record
        assert inf["n_view"] + inf["n_carry"] == len(before) + len(mapped)
        if s.carry:                                                   # the carry is an open bundle: it starts with a head and holds no other
            hd = sm.heads([r for r, _ in before + mapped])
            k = len(view)
            assert hd[k] and not any(hd[k + 1:])
        assert inf["cut"] <= cin.n_records
        nc = len(s.carry)
    assert nc == len(left)
    if scene.pushes[-1][1]:
        assert left == []


@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_views_add_up_to_the_uncut_rows(scene):
    got, left = sm.run(scene.pushes)
    parts = [cs.model(sm.to_cin(v), scene.num_samples) for v, _ in got if v]
    if left:                                                          # (a scene that ends with an open bundle: flushed here)
        parts.append(cs.model(sm.to_cin(left), scene.num_samples))
    want = cs.model(sm.uncut(scene.pushes), scene.num_samples)
    for k in ROW_KEYS:
        g = np.concatenate([p[k] for p in parts]) if parts else want[k][:0]
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), k
    assert sum(p["n_bases"] for p in parts) == want["n_bases"] and sum(p["span_bases"] for p in parts) == want["span_bases"]


def _neighbour_heads(recs):
    """the WRONG rule: a head when the start lies beyond the end of the record just before"""
    return [j == 0 or recs[j][0] != recs[j - 1][0] or recs[j][1] + 1 > sm.end_of(recs[j - 1]) for j in range(len(recs))]


def test_the_running_maximum_decides_where_it_should():
    by = ss.by_name()
    for name in ("long_covers", "spliced_spans_gap", "spine/%d/gap/whole" % ss.T, "spine/%d/touch/6" % (2 * ss.T), "size/%d" % (3 * ss.T + 1)):
        recs = [r for r, _ in sm.tile_records(sm.uncut(by[name].pushes))]
        right, wrong = sm.heads(recs), _neighbour_heads(recs)
        assert right != wrong and sum(wrong) > sum(right) + 3, name
    # the touching read is no head, the one a base further is
    recs = [r for r, _ in sm.tile_records(by["touch_then_gap"].pushes[0][0])]
    assert sm.heads(recs) == [True, False, True] and recs[1][1] + 1 == sm.end_of(recs[0]) and recs[2][1] + 1 == sm.end_of(recs[1]) + 1


@pytest.mark.parametrize("d", [ss.T, 2 * ss.T])
def test_the_long_read_and_its_head_lie_in_different_blocks(d):
    by = ss.by_name()
    whole = by["spine/%d/gap/whole" % d]
    recs = [r for r, _ in sm.tile_records(whole.pushes[0][0])]
    hd = sm.heads(recs)
    assert [j for j, h in enumerate(hd) if h] == [0, 5, 5 + d] and (5 + d) // ss.T - 5 // ss.T == d // ss.T
    touch = [r for r, _ in sm.tile_records(by["spine/%d/touch/whole" % d].pushes[0][0])]
    assert [j for j, h in enumerate(sm.heads(touch)) if h] == [0, 5]
    # cut behind LONG: the carry holds it alone and the tile's blocks see it only through the spine
    got, _ = sm.run(by["spine/%d/gap/6" % d].pushes)
    assert got[0][1] == ss.info(5, 1, 5, 5) and got[1][1]["cut"] == d - 1 and got[1][1]["n_view"] == d
    # the carry fills whole blocks exactly and X is the next tile's first record
    got, _ = sm.run(by["spine/%d/gap/%d" % (d, 5 + d)].pushes)
    assert [i for _, i in got] == [ss.info(5, d, 5, 5), ss.info(d, 4, 0, 0), ss.info(4, 0, 0, 0)] and d % ss.T == 0
    got, _ = sm.run(by["spine/%d/touch/%d" % (d, 5 + d)].pushes)
    assert [i for _, i in got] == [ss.info(5, d, 5, 5), ss.info(0, d + 4, 0, 0), ss.info(d + 4, 0, 0, 0)]
    # cut among the covered reads: the carry (for d = 2 T: two blocks of it) decides a tile of one wave
    c = 9 + d // 2
    got, _ = sm.run(by["spine/%d/gap/%d-%d" % (d, c, c + 64)].pushes)
    assert got[0][1] == ss.info(5, c - 5, 5, 5) and got[1][1] == ss.info(0, c - 5 + 64, 0, 0) and (d < 2 * ss.T or c - 5 > ss.T)
    assert got[2][1]["cut"] == 5 + d - (c + 64)


def test_sized_tiles_put_the_head_where_they_say():
    by = ss.by_name()
    for s in ss.SIZES[1:]:
        sc = by["size/%d" % s]
        t1 = [r for r, _ in sm.tile_records(sc.pushes[0][0])]
        t2 = [r for r, _ in sm.tile_records(sc.pushes[1][0])]
        assert len(t1) == len(t2) == s
        assert [j for j, h in enumerate(sm.heads(t1)) if h] == ([0, s - 1] if s > 1 else [0])
        assert [j for j, h in enumerate(sm.heads(t2)) if h] == [0] and sum(_neighbour_heads(t2)) == max(s - 1, 1)
