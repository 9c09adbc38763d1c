"""The offsets pass of the window path's raw form on its own (tests/support/offsets_probe.hip) on hand-built records, runs and bounds
(offsets_model.py): both kernels — the wave kernel, which is the default, and the block kernel (wg_offsets=block) — each with wg_og 1
and 8, must give the numpy model's matrix and row sums word for word, raise TBK_DERR_RAWORDER exactly on the scenes that hold an
inversion inside a file, and keep every entry inside its run whatever the records are."""
import numpy as np
import pytest

import offsets_model as om

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = om.offsets(*om.SCENES[name][:4])
        return memo[name]
    return get


@pytest.fixture(params=["wave-og1", "wave-og8", "block-og1", "block-og8"])
def form(request):
    kernel, og = request.param.split("-og")
    return kernel, int(og)


def _run(ctx, name, form):
    import offsets_probe as op
    tid, pos, run_off, W, _ = om.SCENES[name]
    off, wbase, err = op.offsets(ctx, tid, pos, run_off, W, kernel=form[0], og=form[1])
    return off, wbase, err & op.DERR_RAWORDER, err & ~op.DERR_RAWORDER


@pytest.mark.parametrize("name", om.CLEAN)
def test_matrix_equals_the_model(ctx, want, form, name):
    off, wbase, raworder, other = _run(ctx, name, form)
    w_off, w_wbase = want(name)
    assert not raworder and not other
    bad = np.argwhere(off != w_off)
    assert len(bad) == 0, "first of %d differing words at (row, run) %s: %d, model %d" % (len(bad), bad[0], off[tuple(bad[0])], w_off[tuple(bad[0])])
    assert np.array_equal(wbase, w_wbase)


@pytest.mark.parametrize("name", om.FLAGGED)
def test_inversions_are_flagged_and_entries_stay_inside_their_runs(ctx, form, name):
    off, wbase, raworder, other = _run(ctx, name, form)
    run_off = om.SCENES[name][2]
    assert raworder and not other
    assert np.all(off >= run_off[None, :-1]) and np.all(off <= run_off[None, 1:])
    assert np.array_equal(off[0], run_off[:-1]) and np.array_equal(off[-1], run_off[1:])


def test_hostile_records_stay_inside_their_runs(ctx, form):
    """records in no order at all, reference ids included: flagged, and nothing outside [run start, run end]"""
    import offsets_probe as op
    rng = np.random.default_rng(3)
    n = 7000
    tid = rng.integers(-1, 4, n).astype(np.int32)
    tid[[0, om.TC - 1, om.TC, n - 1]] = [0, 1, 0, 1]     # (both chunks of reference ids are mixed: every key is the record's own)
    pos = rng.integers(-5, 2 ** 31 - 1, n).astype(np.int32)
    run_off = np.array([0, 0, 1000, 1003, 4100, 4100, n], np.uint32)
    W = np.sort(om.raw_key(rng.integers(0, 4, 900), rng.integers(0, 2 ** 31 - 1, 900)))
    off, wbase, err = op.offsets(ctx, tid, pos, run_off, W, kernel=form[0], og=form[1])
    assert err == op.DERR_RAWORDER
    assert np.all(off >= run_off[None, :-1]) and np.all(off <= run_off[None, 1:])
