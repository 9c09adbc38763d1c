"""The numpy model of the offsets pass (offsets_model.py) against a record-by-record count, and the hand-built scenes against what
their names promise — a scene that no longer sits on its edge fails here, without a GPU."""
import numpy as np
import pytest

import offsets_model as om


def _brute(tid, pos, run_off, W):
    key = [int(x) for x in om.raw_key(tid, pos)]
    k, nW = len(run_off) - 1, len(W)
    off = np.zeros((nW + 2, k), np.uint32)
    for f in range(k):
        a, b = int(run_off[f]), int(run_off[f + 1])
        off[0, f], off[nW + 1, f] = a, b
        for r in range(nW):
            off[r + 1, f] = next((i for i in range(a, b) if key[i] >= int(W[r])), b)
    return off


@pytest.mark.parametrize("name", ["size-1", "size-17", "empty-runs", "files-inside-a-lane", "unplaced-tail", "pos-2^31-1", "bounds-all-equal"])
def test_model_is_the_first_record_at_or_beyond_each_bound(name):
    tid, pos, run_off, W, _ = om.SCENES[name]
    W = W[::max(1, len(W) // 12)]
    off, wbase = om.offsets(tid, pos, run_off, W)
    assert np.array_equal(off, _brute(tid, pos, run_off, W))
    assert wbase[0] == 0 and wbase[-1] == len(pos) and np.all(np.diff(wbase.astype(np.int64)) >= 0)


def test_raw_key():
    assert [int(x) for x in om.raw_key([0, 0, 2, -1, 7], [0, 2 ** 31 - 1, 5, -1, -3])] == \
        [0, 2 ** 31 - 1, (2 << 31) | 5, 1 << 62, (7 << 31) | (2 ** 31 - 3)]


@pytest.mark.parametrize("name", list(om.SCENES))
def test_scene_is_well_formed(name):
    tid, pos, run_off, W, flagged = om.SCENES[name]
    assert tid.dtype == np.int32 and pos.dtype == np.int32 and run_off.dtype == np.uint32 and W.dtype == np.uint64
    assert len(tid) == len(pos) == run_off[-1] >= 1 and run_off[0] == 0 and np.all(np.diff(run_off.astype(np.int64)) >= 0)
    assert np.all(W[1:] >= W[:-1])
    assert om.runs_sorted(tid, pos, run_off) == (not flagged)
    assert len(pos) <= 20000 and len(W) * (len(run_off) - 1) <= 200000


def test_scenes_sit_on_their_edges():
    S = om.SCENES
    assert [len(S["size-%d" % n][1]) for n in (1, 15, 16, 17, 1023, 1024, 1025, 2049, 16385)] == [1, 15, 16, 17, 1023, 1024, 1025, 2049, 16385]
    assert [len(S["runs-k%d" % k][2]) - 1 for k in (1, 2, 64)] == [1, 2, 64]
    assert S["boundary-at-16j"][2][1] % 16 == 0 and S["boundary-at-16j-1"][2][1] % 16 == 15 and S["boundary-at-16j+1"][2][1] % 16 == 1
    ro = S["files-inside-a-lane"][2]
    assert np.count_nonzero((ro >= 992) & (ro < 1008)) >= 5              # several files inside sixteen consecutive records
    assert S["run-ends-at-step-end"][2][1] == om.ST and S["run-ends-at-chunk-end"][2][1] == 2 * om.ST
    sizes = np.diff(S["empty-runs"][2].astype(np.int64))
    assert sizes[0] == 0 and sizes[-1] == 0 and sizes[3] == 0 and list(sizes[5:8]) == [0, 0, 0]
    tid, pos, ro, W, _ = S["second-file-below-first"]
    key = om.raw_key(tid, pos)
    assert key[ro[1]] < key[ro[1] - 1]
    assert len(S["bounds-none"][3]) == 0 and len(set(S["bounds-all-equal"][3].tolist())) == 1
    W = S["bounds-equal-pairs"][3]
    assert np.all(W[0::2] == W[1::2])
    W = S["size-1025"][3]
    assert np.any(np.diff(W.astype(np.int64)) == 0) and np.any(np.diff(W.astype(np.int64)) == 1)
    tid, pos, ro, W, _ = S["bounds-below-second-run"]
    assert W.max() < om.raw_key(tid, pos)[ro[1]]
    tid, pos, ro, W, _ = S["bounds-above-first-run"]
    assert W.min() > om.raw_key(tid, pos)[ro[1] - 1]
    for c in (63, 64, 65, 300):
        s = S["bounds-%d-in-one-step" % c]
        assert [om.bounds_in_step(*s[:4], step) for step in range(3)] == [0, c, 0]
    tid, pos, ro, W, _ = S["pile-up-three-steps"]
    assert np.all(pos[om.ST:4 * om.ST] == 700) and 700 in W.tolist()
    assert S["tid-change-in-step"][0][1499] != S["tid-change-in-step"][0][1500]
    t = S["tid-change-in-lane"][0]
    assert len(set(t[1500:1504].tolist())) == 3                          # records 1500 .. 1503: one lane's four
    t = S["mixed-chunk"][0]
    assert t[0] != t[om.TC - 1]
    assert np.all(S["unplaced-tail"][0][-300:] < 0)
    assert S["pos-2^31-1"][1].max() == 2 ** 31 - 1


def test_inversions_lie_where_their_names_say():
    for name, at in (("inversion-in-lane", 1002), ("inversion-between-lanes", 1004), ("inversion-between-quads", 1280),
                     ("inversion-between-steps", 1024), ("inversion-between-chunks", 2048), ("inversion-between-ranges", 16384),
                     ("inversion-last-record", 2999)):
        tid, pos, ro, W, flagged = om.SCENES[name]
        key = om.raw_key(tid, pos)[:ro[1]]
        assert flagged and list(np.flatnonzero(key[1:] < key[:-1]) + 1) == [at]
