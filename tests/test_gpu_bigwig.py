"""tbk_bigwig_build (bigwig.hip) against the host writer, scene by scene (tests/bigwig_scenes.py): the same levels and reductions, per
level the same sections in the same order with identical payload bytes — the zoom floats bit for bit —, every stream readable by
plain zlib.decompress; with HOST and with DEVICE rows.  Then every class of invalid rows: TBK_EINVAL before anything is delivered,
and the same context takes a good call afterwards."""
import numpy as np
import pytest

import bigwig_model
import bigwig_payloads as bp
import bigwig_scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bw_host")


def _build(ctx, scene, device):
    tid, start, end, val = scene.tid, scene.start, scene.end, scene.val.astype(np.float64)
    if device:
        import torch
        tid, start, end, val = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (tid, start, end, val))
    return ctx.bigwig_build(tid, start, end, val, scene.ref_len())


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", bigwig_scenes.names())
def test_scene_equals_host_writer(ctx, host_dir, name, mem):
    scene = bigwig_scenes.by_name(name)
    want = bp.host_file(scene, host_dir)
    levels = _build(ctx, scene, mem == "device")
    got = bp.build_view(levels)
    bp.same_levels(got, want["levels"])
    bp.same_levels(got, bigwig_model.model(scene)["levels"])
    assert max([lv["max_payload"] for lv in levels]) == want["ubuf"]
    assert len(levels[0]["sections"]) == want["n_sections"]
    # the tables are the R-tree's leaves: the host file's leaf keys in order
    for lv, w in zip(levels, want["levels"]):
        keys = [k for leaf, ks in w["rtree"][1] if leaf for k in ks]
        assert [(c, s, c, e) for c, s, e, _o, _z in lv["sections"]] == keys


def test_slices_of_whole_sections(host_dir):
    """a slice size below one level's bytes: the sink gets several slices, each of whole sections, and the bytes are the same"""
    from tiebrush_amd import api
    scene = bigwig_scenes.by_name("chrom_change_mid_section")
    c = api.Context(0)
    try:
        want = _build(c, scene, False)
        c.set_debug("fmt_slice=4096")
        got = _build(c, scene, False)
    finally:
        c.close()
    assert [lv["bytes"] for lv in got] == [lv["bytes"] for lv in want] and [lv["sections"] for lv in got] == [lv["sections"] for lv in want]
    assert len(want[0]["bytes"]) > 4096


def _bad_rows():
    t = np.array([0, 0, 1, 1], dtype=np.int32)
    s = np.array([5, 20, 3, 30], dtype=np.int32)
    e = np.array([10, 25, 9, 40], dtype=np.int32)

    def edit(**kw):
        a = dict(tid=t.copy(), start=s.copy(), end=e.copy())
        for k, (i, v) in kw.items():
            a[k][i] = v
        return a
    return {
        "unsorted_tid": edit(tid=(3, 0)),
        "unsorted_start": dict(tid=t.copy(), start=np.array([20, 5, 3, 30], dtype=np.int32), end=np.array([25, 10, 9, 40], dtype=np.int32)),
        "overlap": edit(end=(0, 21)),
        "equal_starts": edit(start=(1, 5), end=(1, 7)),
        "end_equals_start": edit(end=(2, 3)),
        "end_below_start": edit(end=(1, 19)),
        "negative_start": edit(start=(0, -1)),
        "tid_negative": edit(tid=(0, -1)),
        "tid_beyond_n_ref": edit(tid=(3, 2)),
    }


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", list(_bad_rows()))
def test_invalid_rows_are_refused(ctx, host_dir, name, mem):
    from tiebrush_amd import _lib
    rows = _bad_rows()[name]
    arrs = [rows["tid"], rows["start"], rows["end"], np.ones(4, dtype=np.float64)]
    if mem == "device":
        import torch
        arrs = [torch.from_numpy(a).to("cuda:0") for a in arrs]
    with pytest.raises(_lib.TbkError) as e:
        ctx.bigwig_build(*arrs, np.array([1000, 1000], dtype=np.uint32))
    assert e.value.status == -1, name
    # ... and the context takes the next call
    scene = bigwig_scenes.by_name("two_chroms_same_bin_number")
    bp.same_levels(bp.build_view(_build(ctx, scene, mem == "device")), bp.host_file(scene, host_dir)["levels"])
