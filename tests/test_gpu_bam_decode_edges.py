"""The BAM decode on the device (the second half of bamdev.hip: bam_header_k, the member walks, the chain bam_index_k, bam_fields_k,
bam_fill_k, bam_compact_k, bam_recsize_k / bam_reccopy_k) on the hand-built files of tests/bam_craft.py.  The reference of every
array is the expectation written beside each record, which test_bam_craft_cpu.py has held against the host loaders."""
import ctypes

import numpy as np
import pytest

import bam_craft as bc
from helpers import tbk_debug

pytestmark = pytest.mark.gpu

FIELDS = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig", "yc_in", "yx_in", "yd_in", "md_off", "md_has", "qname_hash", "qname_off")
CORE = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")
MESSAGE = {"chain": "record chain", "header": "header", "fields": "malformed BAM record"}


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.bam_release()
    c.close()


def _compare(ctx, scene, s, fo, want, md=True, names=True):
    assert np.array_equal(fo, want["file_off"]) and s.n_records == len(want["tid"]) and s.n_cigar_ops == len(want["cig"])
    got = ctx.soa_to_numpy(s, fields=FIELDS)
    for a in CORE:
        assert got[a].dtype == want[a].dtype and np.array_equal(got[a], want[a]), (scene.name, a)
    if scene.tbmerged.any():
        assert s.yc_in and s.yx_in and s.yd_in
        tb = scene.tb_mask()
        for a in bc.CARRIED:
            assert np.array_equal(got[a][tb], want[a][tb]), (scene.name, a)
    if md:
        for a in ("md_off", "md", "md_has"):
            assert np.array_equal(got[a], want[a]), (scene.name, a)
    else:
        assert not s.md_off and not s.md and not s.md_has
    if names:
        for a in ("qname_off", "qname", "qname_hash"):
            assert np.array_equal(got[a], want[a]), (scene.name, a)
    else:
        assert not s.qname_off and not s.qname and not s.qname_hash


def _decode(ctx, scene, md=True, names=True):
    return ctx.bam_decode(scene.files, tbmerged=scene.tbmerged, want_md=md, want_names=names)


@pytest.mark.parametrize("name", list(bc.well_formed()))
def test_scene_decodes_to_its_expectation(ctx, monkeypatch, name):
    """every array of the tile, as built (and the record index that ran is the one the scene's members call for), through the chain
    kernel whatever the members look like, and without MD and names (those pointers null, every other array the same)"""
    scene = bc.well_formed()[name]
    want = scene.expect()
    ctx.set_profiling(True)
    try:
        s, fo = _decode(ctx, scene)
        kt = ctx.kernel_times()
    finally:
        ctx.set_profiling(False)
    assert "bam_index" in kt and ("bam_index_chain" in kt) == (scene.index == "chain"), (scene.index, sorted(kt))
    _compare(ctx, scene, s, fo, want)
    tbk_debug(monkeypatch, index_chain=1)
    ctx.set_profiling(True)
    try:
        s, fo = _decode(ctx, scene)
        kt = ctx.kernel_times()
    finally:
        ctx.set_profiling(False)
        tbk_debug(monkeypatch, index_chain=None)
    assert "bam_index_chain" in kt and "bam_index" not in kt
    _compare(ctx, scene, s, fo, want)
    s, fo = _decode(ctx, scene, md=False, names=False)
    _compare(ctx, scene, s, fo, want, md=False, names=False)
    s, fo = _decode(ctx, scene, md=True, names=False)
    _compare(ctx, scene, s, fo, want, md=True, names=False)


def test_files_without_records(ctx):
    """no file has a record: an empty tile, and the context decodes the next scene"""
    scene = bc.scene_all_empty()
    s, fo = _decode(ctx, scene)
    assert s.n_records == 0 and s.n_cigar_ops == 0 and fo.tolist() == [0, 0, 0]
    good = bc.good_scene()
    s, fo = _decode(ctx, good)
    _compare(ctx, good, s, fo, good.expect())


@pytest.mark.parametrize("name", ["sizes", "huge_record/a", "cigar_max", "min3000", "long_record/hand"])
def test_bam_records_hands_back_the_builders_bytes(ctx, name):
    """tbk_bam_records over the record-size scenes: indices out of order and repeated, the 37-byte record, the 100 KB and the 256 KB
    one, lengths that are no multiple of the wave copy's 64 bytes; an index of n_records is refused"""
    from tiebrush_amd import api
    scene = bc.well_formed()[name]
    recs = [r for f in scene.recs for r in f]
    n = len(recs)
    s, fo = _decode(ctx, scene)
    assert s.n_records == n
    big = int(np.argmax([len(r.raw) for r in recs])), int(np.argmin([len(r.raw) for r in recs]))
    idx = [n - 1, 0, big[0], big[1], n // 2, 0, big[0], n - 1, 1, n - 2] + list(range(n - 1, -1, -max(1, n // 40)))
    blob, off = ctx.bam_records(np.array(idx, np.uint32))
    assert len(off) == len(idx) + 1 and int(off[0]) == 0 and int(off[-1]) == len(blob)
    for j, i in enumerate(idx):
        assert blob[int(off[j]):int(off[j + 1])] == recs[i].raw, (j, i)
    assert any(len(recs[i].raw) % 64 for i in idx)
    for bad in ([n], [0, n, 1], [2**32 - 1]):
        with pytest.raises(api.TbkError) as e:
            ctx.bam_records(np.array(bad, np.uint32))
        assert e.value.status == -1
    blob, off = ctx.bam_records(np.array([0], np.uint32))          # and the tile is still there
    assert blob == recs[0].raw


def _seen(ptr, n):
    a = np.empty(n, np.uint8)
    if n:
        assert ptr
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(n), 2) == 0
    return a


@pytest.mark.parametrize("fn", bc.TAG_SCENES, ids=[f.__name__[6:] for f in bc.TAG_SCENES])
def test_tag_scenes_through_spans(ctx, fn):
    """tbk_bam_decode_spans: one span from the first record to the end of its members, one that ends at a record's end inside its
    last member — the same arrays for the records in the spans, every record read as a TieBrush-merged file's, and the tag_seen bits"""
    scene = fn()
    for data, recs in zip(scene.files, scene.recs):
        lay = bc.layout(data)
        assert len(lay.msize) == 2 and lay.msize[1] == 0          # (one member and the EOF member, which a span does not take)
        body = data[:-28]
        j = len(recs) // 2
        spans = bc.Scene("spans", [], [recs, recs[:j + 1]], [1, 1])
        want = spans.expect()
        s, so, seen = ctx.bam_decode_spans([(body, lay.first, 0), (body, lay.first, lay.ends[j])], scene.n_ref)
        assert np.array_equal(so, want["file_off"]) and s.n_records == len(want["tid"])
        got = ctx.soa_to_numpy(s, fields=CORE + bc.CARRIED)
        for a in CORE + bc.CARRIED:
            assert np.array_equal(got[a], want[a]), (scene.name, a)
        assert np.array_equal(_seen(seen, s.n_records), want["seen"])
        assert not s.md_off and not s.qname_off


def test_tag_seen_tells_a_zero_from_an_absent_tag(ctx):
    scene = bc.scene_carried()
    cases = bc._carried_cases()
    i_yc0 = [i for i, (aux, _) in enumerate(cases) if aux == bc.tag("YC", "f", 0.0)][0]
    i_yx1 = [i for i, (aux, _) in enumerate(cases) if aux == bc.tag("YX", "C", 1)][0]
    i_none = [i for i, (aux, _) in enumerate(cases) if aux == b""][0]
    lay = bc.layout(scene.files[1])
    s, so, seen = ctx.bam_decode_spans([(scene.files[1][:-28], lay.first, 0)], 3)
    got = ctx.soa_to_numpy(s, fields=bc.CARRIED)
    bits = _seen(seen, s.n_records)
    assert got["yc_in"][i_yc0] == got["yc_in"][i_none] == 0.0 and bits[i_yc0] & 1 and not bits[i_none] & 1
    assert got["yx_in"][i_yx1] == got["yx_in"][i_none] == 1 and bits[i_yx1] & 2 and not bits[i_none] & 2


@pytest.mark.parametrize("kind", bc.MALFORMED_KINDS)
def test_malformed_scenes_are_refused_and_the_context_goes_on(ctx, kind):
    """ordinary bad input, in the tile's first record, its last, and one in the middle of the second file: TBK_EINVAL with the
    message of the stage that found it, and the same context decodes a good scene afterwards"""
    from tiebrush_amd import api
    good = bc.good_scene()
    want = good.expect()
    stage = bc.MALFORMED_STAGE.get(kind, "fields")
    for position in bc.POSITIONS:
        scene = bc.malformed()["bad/%s/%s" % (kind, position)]
        with pytest.raises(api.TbkError) as e:
            _decode(ctx, scene)
        assert e.value.status == -1, (kind, position)
        assert MESSAGE[stage] in ctx.last_message(), (kind, position, ctx.last_message())
        s, fo = _decode(ctx, good)
        _compare(ctx, good, s, fo, want)


@pytest.mark.parametrize("tb", [False, True], ids=["plain", "first_file_tbmerged"])
def test_mixed_scene_collapses_to_the_oracles_groups(ctx, tb):
    """compressed bytes -> device tile -> collapse, against the oracle's collapse of the expected tile; the carried tags of a file
    that is not flagged tbmerged count for nothing"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, soa
    scene = bc.well_formed()["mixed_tb" if tb else "mixed"]
    w = scene.expect(oracle_defaults=True)
    tile = soa.SoATile(n_files=len(scene.files), file_off=w["file_off"], tbmerged=scene.tbmerged, tid=w["tid"], pos=w["pos"], flag=w["flag"],
                       mapq=w["mapq"], strand=w["strand"], nh=w["nh"], cig_off=w["cig_off"], cig=w["cig"],
                       yc_in=w["yc_in"] if tb else None, yx_in=w["yx_in"] if tb else None, yd_in=w["yd_in"] if tb else None)
    want = orc.collapse(tile)
    assert 0 < want["n_groups"] < tile.n_records
    if tb:
        assert float(np.max(want["yc"])) > 2.0                      # (the carried counts did reach the oracle's groups)
    s, fo = ctx.bam_decode(scene.files, tbmerged=scene.tbmerged)
    got = api.to_numpy(ctx.collapse_struct(s, len(scene.files)))
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in ("rep", "yc", "yx", "yd", "g_start", "g_end"):
        assert np.array_equal(np.asarray(got[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), k
    ctx.bam_release()
