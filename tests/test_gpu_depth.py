"""tbk_cov_thresholds (tiebrush_amd/csrc/depththr.hip) through Context.cov_thresholds against depth_model on the scenes of
depth_scenes: rows and outputs in host memory, and again in device memory.  The counts are integers: equality with the model is
demanded bit for bit."""
import numpy as np
import pytest

import depth_model as dm
import depth_scenes as ds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    """every scene with the model's counts, computed once"""
    out = {}
    for name, f in ds.SCENES.items():
        rows, feats, thr, _ = f()
        out[name] = (rows, feats, thr) + dm.per_row(rows, feats, thr)
    return out


def _device(rows):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in rows.items()}


def _call(ctx, rows, feats, thr, mem):
    """covered, ge as uint64 numpy arrays; with mem == "device" the rows and the outputs live in device memory"""
    got = ctx.cov_thresholds(_device(rows) if mem == "device" else rows, feats, thr)
    if mem == "device":
        import torch
        assert all(torch.is_tensor(got[k]) and got[k].is_cuda and got[k].dtype == torch.int64 for k in ("covered", "ge"))
        got = {k: v.cpu().numpy().view(np.uint64) for k, v in got.items()}
    assert got["covered"].dtype == np.uint64 and got["ge"].dtype == np.uint64 and got["ge"].shape == (len(feats["tid"]), len(thr))
    return got


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", sorted(ds.SCENES))
def test_scenes(ctx, scenes, name, mem):
    rows, feats, thr, cov, ge = scenes[name]
    got = _call(ctx, rows, feats, thr, mem)
    assert np.array_equal(got["covered"], cov), np.flatnonzero(got["covered"] != cov)[:5]
    assert np.array_equal(got["ge"], ge), np.argwhere(got["ge"] != ge)[:5]
    again = _call(ctx, rows, feats, thr, mem)
    assert got["covered"].tobytes() == again["covered"].tobytes() and got["ge"].tobytes() == again["ge"].tobytes()


def test_features_as_tuples_and_no_rows(ctx, scenes):
    import feature_scenes as fs
    rows, feats, thr, cov, ge = scenes["equal"]
    tup = [(int(t), int(b), int(e), "+") for t, b, e in zip(feats["tid"], feats["beg"], feats["end"])]      # strands are ignored
    got = ctx.cov_thresholds(rows, tup, thr)
    assert np.array_equal(got["covered"], cov) and np.array_equal(got["ge"], ge)
    # n_intervals == 0: zeros, status 0
    for empty in (fs.rows_of(), {}):
        z = ctx.cov_thresholds(empty, feats, thr)
        assert z["ge"].shape == ge.shape and not z["ge"].any() and not z["covered"].any()


def _good(ctx, scenes, mem="host"):
    rows, feats, thr, cov, ge = scenes["runs13"]
    got = _call(ctx, rows, feats, thr, mem)
    assert np.array_equal(got["covered"], cov) and np.array_equal(got["ge"], ge)


REFUSED_THR = {"17 thresholds": [float(k) for k in range(1, 18)], "0 thresholds": [], "descending": [2.0, 1.0], "equal": [1.0, 1.0], "NaN": [1.0, float("nan")],
               "infinite": [1.0, float("inf")], "zero": [0.0, 1.0], "negative": [-1.0]}


@pytest.mark.parametrize("what", sorted(REFUSED_THR))
def test_refused_thresholds(ctx, scenes, what):
    from tiebrush_amd._lib import TbkError
    rows, feats = scenes["runs13"][:2]
    with pytest.raises(TbkError) as e:
        ctx.cov_thresholds(rows, feats, REFUSED_THR[what])
    assert e.value.status == -1
    _good(ctx, scenes)


@pytest.mark.parametrize("features", [[], [(-1, 0, 5)], [(1, 7, 7)]], ids=["n == 0", "tid < 0", "empty"])
def test_refused_features(ctx, scenes, features):
    from tiebrush_amd._lib import TbkError
    rows, _, thr = scenes["runs13"][:3]
    with pytest.raises(TbkError) as e:
        ctx.cov_thresholds(rows, features, thr)
    assert e.value.status == -1
    _good(ctx, scenes)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("what", ["unsorted", "overlapping", "tid order"])
def test_refused_rows(ctx, scenes, what, mem):
    from tiebrush_amd._lib import TbkError
    rows, feats, thr = scenes["runs13"][:3]
    bad = {k: v.copy() for k, v in rows.items()}
    n = len(bad["iv_tid"])
    if what == "unsorted":
        for k in bad:
            bad[k][[600, 601]] = bad[k][[601, 600]]
    elif what == "overlapping":
        bad["iv_end"][n - 3] += 5                                     # (in the last partial wave of the check)
    else:
        bad["iv_tid"][0] = 1
    with pytest.raises(TbkError) as e:
        ctx.cov_thresholds(_device(bad) if mem == "device" else bad, feats, thr)
    assert e.value.status == -1 and "sorted" in str(e.value)
    _good(ctx, scenes, mem)
