"""The items of the YD stage where they are placed by list, on the scenes of yd_item_scenes.py (test_yd_item_scenes_cpu.py proves that
each reaches its edge): a far item carries the offset of its exon list, yd_wave_k fetches two batches deep, no list machine looks a group up,
the item -> group word is a 16-bit index inside its tile, and a dense tile is staged in rounds.  Every scene is compared with the
oracle, array for array, and run in the four forms of the list machines, which must agree with the default form: every chain in
yd_wave_k, every chain in yd_lane_k (chains whose list outgrows the machine go on to yd_run_k in both), every chain in yd_run_k.  The
scenes about exon offsets also run with yd_front=split, where an earlier pass makes the offsets the placement hands to the items."""
import numpy as np
import pytest

import yd_item_scenes as ys
from helpers import tbk_debug
from test_gpu_fuzz import _cmp

pytestmark = pytest.mark.gpu

KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end", "rec_group")
FORMS = {"wave": dict(yd_wave_min="1"), "lane": dict(yd_wave_min=str(1 << 30)), "literal": dict(yd_literal="1")}
CLEAR = dict(yd_wave_min=None, yd_literal=None, yd_front=None)


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _got(ctx, tile):
    from tiebrush_amd import api
    return api.to_numpy(ctx.collapse(tile, want_rec_group=True))


@pytest.mark.parametrize("name", list(ys.SCENES))
def test_scene_in_every_form(ctx, monkeypatch, name):
    tile = ys.get(name)
    tbk_debug(monkeypatch, path="window", **CLEAR)
    want = _cmp(ctx, tile)
    assert want["n_groups"] == ys.oracle(name)["n_groups"]
    forms = dict(FORMS)
    if name in ys.FAR_OFFSET_SCENES:
        forms["split"] = dict(yd_front="split")
    for form, kw in forms.items():
        tbk_debug(monkeypatch, **dict(CLEAR, **kw))
        got = _got(ctx, tile)
        assert got["n_groups"] == want["n_groups"], form
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (form, k)
