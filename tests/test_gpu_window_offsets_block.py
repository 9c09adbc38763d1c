"""The raw window path with the block kernel of the offsets pass (wg_offsets=block; the default is the wave kernel, which
test_gpu_window_edges.py runs): the partition scenes of window_scenes.py once more, against the oracle and the model's route, with
one chunk per block and with eight."""
import numpy as np
import pytest

import window_model as wm
import window_scenes as ws
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end")
PARTITION = ws.RUN_SCENES + ["tid-change-at-chunk-edges", "400-files-of-5", "dense-64-files", "dense-96-files", "unplaced-tail", "extreme-coordinates"]


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("og", [None, "8"])
@pytest.mark.parametrize("name", PARTITION + ws.PILE_SCENES)
def test_partition_with_the_block_kernel(ctx, monkeypatch, name, og):
    from tiebrush_amd import api
    tbk_debug(monkeypatch, path="window", wg_stats="1", raw="1", wg_offsets="block", wg_og=og)
    s, want = ws.get(name), ws.oracle(name)
    got = api.to_numpy(ctx.collapse(s.tile, **s.opts))
    route = ctx.collapse_route()
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert route["reseeds"] == 0 and not route["raw_handed_back"]
    if s.tile.n_files > wm.WINDOW_MAX_FILES:
        assert route["form"] == "sort"
        return
    p = wm.predict(s.tile, True, want["rec_group"], **{k: v for k, v in s.opts.items() if k != "strategy"})
    assert {k: route[k] for k in ("nw", "nw_live", "ovf1", "ovf2")} == {k: p[k] for k in ("nw", "nw_live", "ovf1", "ovf2")}
    assert route["form"] == ("sort" if p["big_bucket"] else "raw")


@pytest.mark.parametrize("og", ["1", "8"])
@pytest.mark.parametrize("at", [wm.WG_OC, wm.WG_OG * wm.WG_OC])
def test_block_kernel_hands_an_inversion_back(ctx, monkeypatch, at, og):
    from tiebrush_amd import api
    tbk_debug(monkeypatch, path="window", wg_stats="1", raw="1", wg_offsets="block", wg_og=og)
    with pytest.raises(api.TbkError) as e:
        ctx.collapse(ws.pos_inversion(at, False))
    assert e.value.status == -6                                     # TBK_EUNSORTED
    r = ctx.collapse_route()
    assert r["form"] == "none" and r["raw_handed_back"]
