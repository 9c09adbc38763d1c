"""tbk_cov_summary (tiebrush_amd/csrc/featsum.hip) through Context.cov_summary against feature_model, on the hand-placed
scenes of feature_scenes, a seeded random case and the golden BAMs' own rows; rows from host and from device memory.

The numeric contract: covered, max and junc are exact; sum is exact where every row value on the feature is a multiple of 2^-3 and the
sum stays below 2^50 (feature_model.exact), else within gamma(m + 1) x the sum of |val x bases| (feature_model.check_sum)."""
import os

import numpy as np
import pytest

import feature_model as fm
import feature_scenes as fs
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

COLS = ("covered", "sum", "max", "junc")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _device(rows):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in rows.items()}


def _check(got, rows, feats):
    model = fm.mark_dyadic(rows, fm.per_row(rows, feats))
    assert got["covered"].dtype == np.uint64 and all(got[k].dtype == np.float64 for k in COLS[1:])
    for k, m in enumerate(model):
        assert int(got["covered"][k]) == m["covered"], (k, got["covered"][k], m["covered"])
        assert float(got["max"][k]) == m["max"], (k, got["max"][k], m["max"])
        assert float(got["junc"][k]) == m["junc"], (k, got["junc"][k], m["junc"])
        fm.check_sum(got["sum"][k], m)
    return model


@pytest.fixture(scope="module")
def scenes():
    return {name: f() for name, f in fs.SCENES.items()}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", sorted(fs.SCENES))
def test_scenes(ctx, scenes, name, mem):
    rows, feats, _ = scenes[name]
    got = ctx.cov_summary(_device(rows) if mem == "device" else rows, feats)
    model = _check(got, rows, feats)
    if name == "thirds":
        assert not any(fm.exact(m) for m in model if m["m"])      # this scene is the one held to the bound
    again = ctx.cov_summary(_device(rows) if mem == "device" else rows, feats)
    for k in COLS:
        assert got[k].tobytes() == again[k].tobytes(), k           # the same inputs, the same bits


def test_random_case(ctx):
    rows, feats = fs.random_case()
    got = ctx.cov_summary(rows, feats)
    model = _check(got, rows, feats)
    assert all(fm.exact(m) for m in model)
    dev = ctx.cov_summary(_device(rows), feats)
    for k in COLS:
        assert got[k].tobytes() == dev[k].tobytes(), k


def test_feature_forms_and_missing_tracks(ctx, scenes):
    """features as tuples (with and without strands); rows without the interval or the junction columns leave those out"""
    rows, feats, _ = scenes["junctions"]
    tup = [(int(t), int(b), int(e), chr(int(s))) for t, b, e, s in zip(feats["tid"], feats["beg"], feats["end"], feats["strand"])]
    a, b = ctx.cov_summary(rows, feats), ctx.cov_summary(rows, tup)
    for k in COLS:
        assert np.array_equal(a[k], b[k])
    dots = ctx.cov_summary(rows, [f[:3] for f in tup])
    want = fm.per_row(rows, dict(feats, strand=np.full(len(tup), ord("."), np.uint8)))
    assert dots["junc"].tolist() == [m["junc"] for m in want]
    only_j = ctx.cov_summary({k: v for k, v in rows.items() if k[:2] == "j_"}, feats)
    assert sorted(only_j) == ["junc"] and np.array_equal(only_j["junc"], a["junc"])
    rows2, feats2, _ = scenes["edges"]
    only_c = ctx.cov_summary({k: v for k, v in rows2.items() if k[:3] == "iv_"}, feats2)
    assert sorted(only_c) == ["covered", "max", "sum"]
    _check(dict(only_c, junc=np.zeros(len(feats2["tid"]))), rows2, feats2)
    # no row at all: zeros, status 0
    empty = ctx.cov_summary(fs.rows_of(), feats2)
    assert all(not empty[k].any() for k in COLS)


def _good(ctx, scenes):
    rows, feats, _ = scenes["edges"]
    _check(ctx.cov_summary(rows, feats), rows, feats)


REFUSED_FEATURES = {"no feature": [], "tid < 0": [(-1, 0, 5)], "beg < 0": [(1, -1, 5)], "end == beg": [(1, 7, 7)], "end < beg": [(1, 9, 7)],
                    "strand": [(1, 0, 5, "+"), (1, 0, 5, "*")]}


@pytest.mark.parametrize("what", sorted(REFUSED_FEATURES))
def test_refused_features(ctx, scenes, what):
    from tiebrush_amd._lib import TbkError
    rows = scenes["edges"][0]
    with pytest.raises(TbkError) as e:
        ctx.cov_summary(rows, REFUSED_FEATURES[what])
    assert e.value.status == -1
    _good(ctx, scenes)


def _swap(rows, key, i, j):
    out = {k: v.copy() for k, v in rows.items()}
    for k in out:
        if k.startswith(key):
            out[k][[i, j]] = out[k][[j, i]]
    return out


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("what", ["iv order", "iv overlap", "iv tid order", "iv end < start", "j start", "j end", "j strand", "j tid"])
def test_refused_rows(ctx, scenes, what, mem):
    from tiebrush_amd._lib import TbkError
    rows, feats, _ = scenes["runs"]
    jrows = scenes["junctions"][0]
    rows = dict(rows, **{k: v for k, v in jrows.items() if k[:2] == "j_"})
    n = len(rows["iv_tid"])
    if what == "iv order":
        bad = _swap(rows, "iv_", 600, 601)
    elif what == "iv overlap":
        bad = {k: v.copy() for k, v in rows.items()}
        bad["iv_end"][n - 3] += 5                                     # (in the last partial wave of the check)
    elif what == "iv tid order":
        bad = {k: v.copy() for k, v in rows.items()}
        bad["iv_tid"][0] = 1
    elif what == "iv end < start":
        bad = {k: v.copy() for k, v in rows.items()}
        bad["iv_end"][300] = bad["iv_start"][300] - 1
    elif what == "j start":
        bad = _swap(rows, "j_", 3, 4)
    elif what == "j end":
        bad = _swap(rows, "j_", 2, 3)
    elif what == "j strand":
        bad = _swap(rows, "j_", 0, 1)
    else:
        bad = _swap(rows, "j_", 4, 5)
    with pytest.raises(TbkError) as e:
        ctx.cov_summary(_device(bad) if mem == "device" else bad, feats)
    assert e.value.status == -1 and "sorted" in str(e.value)
    _check(ctx.cov_summary(_device(rows) if mem == "device" else rows, feats), rows, feats)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", ["t1", "t2"])
def test_golden_rows_as_features(ctx, name, mem, bam_loader):
    """every junction row of the golden as a feature gets its own value, every coverage row covered == size and sum == val x size"""
    from tiebrush_amd import api, soa
    cin = soa.cov_input_from_bam(bam_loader(os.path.join(GOLDEN, name, name + ".bam")))
    res = ctx.coverage(api.to_device(cin, "cuda:0") if mem == "device" else cin)
    rows = {k: v for k, v in api.to_numpy(res).items() if k[:3] == "iv_" or k[:2] == "j_"}
    given = {k: res[k] for k in rows}
    nj, ni = len(rows["j_tid"]), len(rows["iv_tid"])
    assert nj >= 1 and ni > 100
    jf = dict(tid=rows["j_tid"], beg=rows["j_start"].astype(np.int64), end=rows["j_end"].astype(np.int64), strand=rows["j_strand"])
    got = ctx.cov_summary(given, jf)
    assert np.array_equal(got["junc"], rows["j_val"])
    _check(got, rows, jf)
    cf = dict(tid=rows["iv_tid"], beg=rows["iv_start"].astype(np.int64), end=rows["iv_end"].astype(np.int64), strand=np.full(ni, ord("."), np.uint8))
    got = ctx.cov_summary(given, cf)
    size = (rows["iv_end"].astype(np.int64) - rows["iv_start"]).astype(np.uint64)
    assert np.array_equal(got["covered"], size) and np.array_equal(got["sum"], rows["iv_val"] * size.astype(np.float64))
    assert np.array_equal(got["max"], rows["iv_val"])
    _check(got, rows, cf)
