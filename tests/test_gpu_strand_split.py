"""tbk_cov_split_strand on the device: every scene of strand_scenes.py, as a HOST input and as device tensors, against the
model (strand_model.py) array by array; the rows of every part against the oracle on the model's part; and the lifetimes the command
lines rest on: the views survive the coverage, sample and clip calls, the context's other views (region view, stream view and carry)
survive the split."""
import numpy as np
import pytest

import region_fixtures as rf
import strand_model as stm
import strand_scenes as sts
import stream_scenes as ss
import stream_model as sm

pytestmark = pytest.mark.gpu

SCENES = sts.scenes()
COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
SAMP_KEYS = ("s_tid", "s_start", "s_end", "s_count", "s_heat")
NS = 7


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """per scene, computed once: the model's parts and, where tiecov takes the scene, the oracle's rows of each part"""
    from oracle import oracle_ffi as orc
    out = {}
    for sc in SCENES:
        parts = stm.split(sc.cin)
        rows = [orc.coverage(stm.for_oracle(p), num_samples=NS if sc.sample_ok else 0) if sc.cov_ok and p.n_records else None for p in parts]
        out[sc.name] = (parts, rows)
    return out


def _assert_rows(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(w), (what, k, len(g), len(w))
        if len(w):
            assert g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes(), (what, k)


def _assert_views(views, parts, what):
    from tiebrush_amd import api
    assert len(views) == 3
    for s, (v, p) in enumerate(zip(views, parts)):
        assert v.n_records == p.n_records and v.n_cigar_ops == len(p.cig), (what, s, v.n_records, p.n_records)
        assert not v.struct.flag, (what, s)
        if p.n_records == 0:
            continue
        assert stm.same(api.cov_view_to_numpy(v), p) is None, (what, s, stm.same(api.cov_view_to_numpy(v), p))


def _copy(cin):
    from tiebrush_amd import soa
    return soa.CovInput(*[None if a is None else np.array(a, copy=True) for a in (cin.tid, cin.pos, cin.flag, cin.cig_off, cin.cig, cin.yc, cin.strand, cin.yx)])


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_scene(ctx, want, scene, mem):
    from tiebrush_amd import api
    parts, rows = want[scene.name]
    before = _copy(scene.cin)
    cin = scene.cin if mem == "host" else api.to_device(scene.cin)
    whole = api.to_numpy(ctx.coverage(cin)) if scene.cov_ok and scene.cin.n_records else None
    views = ctx.cov_split_strand(cin)
    _assert_views(views, parts, scene.name)
    assert sum(v.n_records for v in views) == int(((scene.cin.flag & 4) == 0).sum())
    back = scene.cin if mem == "host" else api.CovInput(*[None if a is None else a.cpu().numpy() for a in
                                                          (cin.tid, cin.pos, cin.flag, cin.cig_off, cin.cig, cin.yc, cin.strand, cin.yx)])
    assert stm.same(back, before) is None                              # the input is untouched
    if not scene.cov_ok:
        return
    for s, (v, p, w) in enumerate(zip(views, parts, rows)):
        got = api.to_numpy(ctx.coverage(v))
        if w is None:                                                   # an empty class: tbk_coverage_tile accepts the view and gives no rows
            assert got["n_intervals"] == 0 and got["n_junctions"] == 0 and got["n_bases"] == 0
            continue
        _assert_rows(got, w, COV_KEYS, (scene.name, s))
        assert got["n_bases"] == w["n_bases"], (scene.name, s)
        if scene.sample_ok:
            _assert_rows(api.to_numpy(ctx.sample(v, NS)), w, SAMP_KEYS, (scene.name, s, "sample"))
        else:                                                           # (YX beyond 2^31: strand_scenes.py says why the oracle has no say)
            cap = 2 * len(p.cig) + 2 * p.n_records + 16
            _assert_rows(api.to_numpy(ctx.sample(v, NS)), api.to_numpy(ctx.sample(api.to_device(p), NS, cap_intervals=cap)), SAMP_KEYS, (scene.name, s, "sample"))
    _assert_views(views, parts, (scene.name, "after the coverage and sample calls"))
    if whole is not None:                                               # the whole input after the split: what it was before
        again = api.to_numpy(ctx.coverage(cin))
        _assert_rows(again, whole, COV_KEYS, (scene.name, "whole"))
        assert again["n_bases"] == whole["n_bases"] and again["span_bases"] == whole["span_bases"]


def test_one_context_three_calls(want):
    """10007 records, then 1, then 4097 on one context: the workspace and the views' storage are reused"""
    from tiebrush_amd import api
    c = api.Context(0)
    try:
        for n in (10007, 1, 4097):
            name = "size/%d/mod3" % n
            sc = sts.by_name()[name]
            views = c.cov_split_strand(api.to_device(sc.cin))
            _assert_views(views, want[name][0], name)
    finally:
        c.close()


def test_strand_none_is_refused_and_the_context_goes_on(ctx, want):
    from tiebrush_amd import api, soa
    sc = sts.by_name()["size/257/mod3"]
    c = sc.cin
    bad = soa.CovInput(c.tid, c.pos, c.flag, c.cig_off, c.cig, c.yc, None, c.yx)
    with pytest.raises(api.TbkError) as e:
        ctx.cov_split_strand(bad)
    assert e.value.status == -1
    _assert_views(ctx.cov_split_strand(c), want[sc.name][0], "after the refusal")


def test_empty_input_whatever_the_pointers(ctx):
    """n_records == 0 with every column NULL — what a command line hands over for a file or a region without reads —, as a HOST and as
    a DEVICE input: three empty views, status 0"""
    from tiebrush_amd import _lib, api
    for mem in (_lib.TBK_MEM_HOST, _lib.TBK_MEM_DEVICE):
        s = _lib.CovIn()
        s.mem = mem
        views = ctx.cov_split_strand(api.DeviceCovView(s, 0, 0))
        assert [v.n_records for v in views] == [0, 0, 0]
        assert api.to_numpy(ctx.coverage(views[2]))["n_intervals"] == 0


def test_a_view_of_the_last_split_is_no_input(ctx, want):
    """the views die with the next split, so one of them cannot be its input: refused on the host, the views stay, the context goes on"""
    from tiebrush_amd import api
    sc = sts.by_name()["size/2049/mod3"]
    views = ctx.cov_split_strand(sc.cin)
    with pytest.raises(api.TbkError) as e:
        ctx.cov_split_strand(views[1])
    assert e.value.status == -1 and "previous split" in str(e.value)
    _assert_views(views, want[sc.name][0], "after the refusal")
    _assert_views(ctx.cov_split_strand(api.to_device(sc.cin)), want[sc.name][0], "the next call")


def test_no_yx_and_no_flag(ctx):
    """yx None: views without yx; flag None: every record is mapped"""
    from tiebrush_amd import api, soa
    c = sts.by_name()["unmapped/u_seventh"].cin
    for cin in (soa.CovInput(c.tid, c.pos, c.flag, c.cig_off, c.cig, c.yc, c.strand, None), soa.CovInput(c.tid, c.pos, None, c.cig_off, c.cig, c.yc, c.strand, c.yx)):
        parts = stm.split(cin)
        for inp in (cin, api.to_device(cin)):
            views = ctx.cov_split_strand(inp)
            _assert_views(views, parts, "columns left out")
            assert all(bool(v.struct.yx) == (cin.yx is not None) for v in views if v.n_records)


def test_region_view_split_and_clipped(ctx, tmp_path):
    """a region view of t1 (all three classes) split, every part's rows cut to the region: the filtered file's whole rows on the region"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, bamio, soa
    fx = rf.Fixture(rf.golden_copy(tmp_path, "t1/t1.bam"), kinds=("bai",))
    whole = soa.cov_input_from_bam(bamio.read_bam(fx.path, keep_names=False))
    parts = stm.split(whole)
    assert [p.n_records for p in parts] == [2504, 58, 917]
    rows = [orc.coverage(stm.for_oracle(p)) for p in parts]
    first = min(r[1] for r in fx.recs if r[0] == fx.recs[0][0])
    empty = [(0, 0, 1000), (fx.recs[0][0], 0, min(1000, first))]           # a reference without a record; before the first record of one that has some
    assert all(fx.brute(*r) == [] for r in empty)
    n_held = 0
    for tid, beg, end in empty + rf.random_regions(fx, 5, 6):
        tile, _, seen = ctx.bam_decode_spans(fx.spans(api.index_query(fx.path, tid, beg, end, fx.indexes["bai"])), len(fx.lens))
        view = ctx.region_view(tile, seen, tid, beg, end)
        assert view.n_records == len(fx.brute(tid, beg, end))
        if view.n_records == 0:
            # the zeroed view of a region without reads (every pointer NULL, the strand column too): three empty views that the
            # coverage call takes, as `tiecov -r` hands it over
            assert not view.struct.strand and not view.struct.tid
            views = ctx.cov_split_strand(view)
            assert [v.n_records for v in views] == [0, 0, 0] and [v.n_cigar_ops for v in views] == [0, 0, 0]
            for v in views:
                got = api.to_numpy(ctx.coverage(v))
                assert got["n_intervals"] == 0 and got["n_junctions"] == 0 and got["n_bases"] == 0
            continue
        n_held += 1
        before = api.to_numpy(ctx.coverage(view))
        views = ctx.cov_split_strand(view)
        assert sum(v.n_records for v in views) == view.n_records
        for s, v in enumerate(views):
            got = api.to_numpy(ctx.cov_clip(ctx.coverage(v), tid, beg, end)) if v.n_records else {k: np.zeros(0) for k in COV_KEYS}
            _assert_rows(got, rf.clip_cov(rows[s], tid, beg, end), COV_KEYS, (tid, beg, end, s))
        _assert_rows(api.to_numpy(ctx.coverage(view)), before, COV_KEYS, "the region view after the split")
    assert n_held >= 3                                                  # (the drawn regions are not all no-ops)


def _push(ctx, cin, final):
    """the next tile of a stream: a device tile of one TieBrush-written file from a CovInput"""
    from tiebrush_amd import api, soa
    n = cin.n_records
    tile = soa.SoATile(n_files=1, file_off=np.array([0, n], np.uint32), tbmerged=np.ones(1, np.uint8), tid=cin.tid, pos=cin.pos, flag=cin.flag,
                       mapq=np.full(n, 60, np.uint8), strand=cin.strand, nh=np.full(n, soa.NH_ABSENT, np.int32), cig_off=cin.cig_off, cig=cin.cig,
                       yc_in=cin.yc, yx_in=cin.yx if cin.yx is not None else np.ones(n, np.int64), yd_in=np.zeros(n, np.int64))
    keep = []
    s, _dev, _n = ctx._soa_struct(api.to_device(tile), keep)
    return ctx.cov_stream_push(s, None, final)


@pytest.mark.parametrize("name", ["long_covers/cut", "spliced_spans_gap", "size/1025", "unmapped_around"])
def test_stream_views_split(ctx, name):
    """a stream of several tiles: every view split, the parts' rows one after the other are the rows of the uncut stream's parts, and the
    carry (which the split must leave alone) still gives the model's next view"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api
    sc = ss.by_name()[name]
    strands = np.array([ord(c) for c in "+-.+"], np.uint8)

    def stranded(cin):                                                  # (the scenes are mostly unstranded: give them all three classes)
        c = _copy(cin)
        c.strand = strands[(np.asarray(c.pos, np.int64) // 3) % 4]
        return c
    pushes = [(stranded(cin), final, seen) for cin, final, seen in sc.pushes if seen is None]
    assert len(pushes) == len(sc.pushes) and pushes[-1][1]
    wviews, _ = sm.run(pushes)
    ctx.cov_stream_reset()
    got = [[], [], []]
    for k, ((cin, final, _), (wview, winfo)) in enumerate(zip(pushes, wviews)):
        view, info = _push(ctx, cin, final)
        assert info == winfo, (k, info, winfo)                          # (the push before left the right carry, split or not)
        if view.n_records == 0:
            continue
        parts = stm.split(sm.to_cin(wview))
        views = ctx.cov_split_strand(view)
        _assert_views(views, parts, (name, k))
        for s, v in enumerate(views):
            if v.n_records:
                got[s].append(api.to_numpy(ctx.coverage(v)))
    uncut = stm.split(sm.uncut(pushes))
    for s in range(3):
        if uncut[s].n_records == 0:
            assert not got[s]
            continue
        w = orc.coverage(stm.for_oracle(uncut[s]))
        _assert_rows({k: np.concatenate([c[k] for c in got[s]]) for k in COV_KEYS}, w, COV_KEYS, (name, s))
        assert sum(c["n_bases"] for c in got[s]) == w["n_bases"]
    ctx.cov_stream_reset()
