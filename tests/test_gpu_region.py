"""`tiecov -r REGION`: the tracks of one region through the file's index, on the device.  The contract is an identity: the
rows equal the whole-file run's rows on the region — intervals trimmed to it, junctions that overlap it kept whole, the sample rows
trimmed — element for element, iv_val bit-equal.  The library (tbk_bam_decode_spans, tbk_region_view, tbk_cov_clip, tbk_sample_clip)
is held against the ORACLE's whole-file result clipped in numpy, many regions in one process; the command line against the whole-file
run's files clipped line by line, a handful of regions, one process each."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bai_reader as br
import csi_reader as cr
import region_fixtures as rf
from helpers import GOLDEN, read_lines

pytestmark = pytest.mark.gpu

BIN = rf.BIN
COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
SAMP_KEYS = ("s_tid", "s_start", "s_end", "s_count", "s_heat")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


class Whole:
    """a fixture file and the oracle's whole-file result, computed once"""

    def __init__(self, fx, num_samples):
        from oracle import oracle_ffi as orc
        from tiebrush_amd import bamio, soa
        self.fx, self.ns = fx, num_samples
        self.rows = orc.coverage(soa.cov_input_from_bam(bamio.read_bam(fx.path, keep_names=False)), num_samples=num_samples)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_region")
    out = {}
    for al in (0, 1):
        out["syn%d" % al] = Whole(rf.Fixture(rf.write_syn(str(d / ("syn%d.bam" % al)), br.SYN_NAMES, br.SYN_LENS, br.synthetic_records(), al)), rf.SYN_SAMPLES)
    out["t2"] = Whole(rf.Fixture(rf.golden_copy(d, "t2/t2.bam")), 10)             # carries YC and YX
    out["t1s0"] = Whole(rf.Fixture(rf.golden_copy(d, "t1/t1s0.bam")), 1)          # a plain input: no YC, no YX
    return out


def _region_rows(ctx, fx, index, tid, beg, end, ns):
    """the region path of the library: (n_kept, coverage rows, sample rows) as numpy"""
    from tiebrush_amd import api
    chunks = api.index_query(fx.path, tid, beg, end, index)
    tile, span_off, seen = ctx.bam_decode_spans(fx.spans(chunks), len(fx.lens))
    assert int(span_off[-1]) == int(tile.n_records) == len(fx.in_chunks(chunks))
    view = ctx.region_view(tile, seen, tid, beg, end)
    if view.n_records == 0:
        return 0, {k: np.zeros(0) for k in COV_KEYS}, {k: np.zeros(0) for k in SAMP_KEYS}
    cov = ctx.cov_clip(ctx.coverage(view), tid, beg, end)             # device rows, cut on the device
    samp = ctx.sample_clip(ctx.sample(view, ns), tid, beg, end)
    return view.n_records, api.to_numpy(cov), api.to_numpy(samp)


def _assert_rows(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(w), (what, k, len(g), len(w))
        if len(w):
            assert g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes(), (what, k)   # (bit-equal, the values included)


def _check_regions(ctx, wh, kind, regions):
    fx = wh.fx
    for tid, beg, end in regions:
        n_kept, cov, samp = _region_rows(ctx, fx, fx.indexes[kind], tid, beg, end, wh.ns)
        assert n_kept == len(fx.brute(tid, beg, end)), (tid, beg, end)
        _assert_rows(cov, rf.clip_cov(wh.rows, tid, beg, end), COV_KEYS, (kind, tid, beg, end))
        _assert_rows(samp, rf.clip_sample(wh.rows, tid, beg, end), SAMP_KEYS, (kind, tid, beg, end))


@pytest.mark.parametrize("kind", ["bai", "csi"])
@pytest.mark.parametrize("name", ["syn0", "syn1"])
def test_synthetic_regions(ctx, files, name, kind):
    """every hand-picked edge and 40 random regions, on members that records straddle (syn0: the chain indexer) and on record-aligned
    members (syn1: a lane per member)"""
    wh = files[name]
    _check_regions(ctx, wh, kind, rf.syn_regions() + rf.random_regions(wh.fx, 21, 40))


def test_the_picked_edges_are_what_they_claim(files):
    """the hand-picked regions hit the shapes they are there for (so that a change of the synthetic file cannot hollow them out)"""
    wh = files["syn1"]
    fx, W = wh.fx, rf.W
    iso = 50 * W - 20
    assert fx.brute(0, iso, iso + 50) == [r for r in fx.recs if r[1] == iso and r[0] == 0] and len(fx.brute(0, iso, iso + 50)) == 1
    assert fx.brute(0, iso + 50, iso + 120) == [] and fx.brute(0, iso - 100, iso) == []
    intron = rf.clip_cov(wh.rows, 0, 70 * W + 1060, 70 * W + 2060)
    assert len(intron["iv_tid"]) == 0 and len(intron["j_tid"]) == 1
    assert len(fx.brute(0, 60 * W + 5, 60 * W + 6)) == 1 and fx.brute(0, 60 * W + 5, 60 * W + 6)[0][2] == 60 * W + 6   # reference length 0
    cut = rf.clip_cov(wh.rows, 0, 30 * W + 1005, 30 * W + 1015)
    whole = wh.rows
    first = np.flatnonzero((whole["iv_tid"] == 0) & (whole["iv_end"] > 30 * W + 1005))[0]
    assert whole["iv_start"][first] < 30 * W + 1005 and cut["iv_start"][0] == 30 * W + 1005 and cut["iv_end"][-1] == 30 * W + 1015
    assert fx.brute(1, 0, 100000) == [] and len(fx.brute(2, 0, 1000000)) == 1
    # a region whose first chunk starts and ends inside members
    from tiebrush_amd import api
    ch = api.index_query(fx.path, 0, 30 * W + 5000, 30 * W + 5100, fx.indexes["bai"])
    assert any(cb & 0xffff and ce & 0xffff for cb, ce in ch)


@pytest.mark.parametrize("name", ["t2", "t1s0"])
def test_golden_regions(ctx, files, name):
    """YC / YX present (t2: a YC of a collapsed record weighs it) and absent (t1s0: 1.0 / 1)"""
    wh = files[name]
    fx = wh.fx
    whole = [(t, 0, fx.lens[t]) for t in sorted(set(r[0] for r in fx.recs))[:2]]
    for kind in ("bai", "csi"):
        _check_regions(ctx, wh, kind, whole + rf.random_regions(fx, 3, 40 if kind == "bai" else 6))


def test_clip_of_host_rows_over_several_references(ctx, files):
    """tbk_cov_clip / tbk_sample_clip on HOST rows: the whole-file rows of t2 (several references) cut to regions on each of them"""
    wh = files["t2"]
    fx = wh.fx
    rows = {k: wh.rows[k] for k in COV_KEYS}
    srows = {k: wh.rows[k] for k in SAMP_KEYS}
    tids = sorted(set(int(t) for t in wh.rows["iv_tid"]))
    assert len(tids) >= 2
    regions = rf.random_regions(fx, 8, 30) + [(t, 0, fx.lens[t]) for t in tids] + [(tids[0], 0, 1), (len(fx.lens) - 1, 0, 5)]
    for tid, beg, end in regions:
        _assert_rows(ctx.cov_clip(rows, tid, beg, end), rf.clip_cov(wh.rows, tid, beg, end), COV_KEYS, (tid, beg, end))
        _assert_rows(ctx.sample_clip(srows, tid, beg, end), rf.clip_sample(wh.rows, tid, beg, end), SAMP_KEYS, (tid, beg, end))
    assert np.array_equal(rows["iv_start"], wh.rows["iv_start"])      # (the caller's rows were copied, not cut)


def test_tag_presence(ctx, tmp_path):
    """a present YC:f:0 stays 0, an absent YC is 1.0; the same for YX"""
    from tiebrush_amd import api, bamio
    aux = [b"", b"YCf" + struct.pack("<f", 0.0), b"YXC\x00", b"YCf" + struct.pack("<f", 3.0) + b"YXC\x07", b"NHC\x01"]
    recs = [bamio.encode_record(0, 100 + 10 * i, 0, 60, [50 << 4], b"r%d" % i, aux=a) for i, a in enumerate(aux)]
    path = str(tmp_path / "tags.bam")
    cr.write_bam(path, ["chrS"], [10000], recs)
    fx = rf.Fixture(path)
    tile, _, seen = ctx.bam_decode_spans(fx.spans(api.index_query(path, 0, 0, 10000)), 1)
    view = ctx.region_view(tile, seen, 0, 0, 10000)
    assert view.n_records == 5
    res = api.to_numpy(ctx.coverage(view))                            # the values the rows carry tell the weights: depth steps by yc
    # records start 10 apart, each 50 long: row k (k < 5) covers [100 + 10 k, 110 + 10 k) with the sum of the first k + 1 weights
    yc = [1.0, 0.0, 1.0, 3.0, 1.0]
    want = np.cumsum(yc)
    got = {int(s): v for s, v in zip(res["iv_start"], res["iv_val"])}
    assert got[100] == want[0] and got[120] == want[2] and got[130] == want[3] and got[140] == want[4]
    assert 110 not in got                                             # (the YC:f:0 record changes nothing: its row merges with the one before)
    samp = api.to_numpy(ctx.sample(view, 10))
    assert len(samp["s_tid"]) > 0


def _bgzf(payload):
    from tiebrush_amd import bamio
    return bamio.bgzf_compress(payload, 6)[:-28]                      # (without the EOF member)


def test_broken_spans_are_refused_and_the_context_goes_on(ctx, files):
    from tiebrush_amd import api, _lib
    fx = files["syn1"].fx
    region = (0, 30 * rf.W + 5000, 30 * rf.W + 5100)
    chunks = api.index_query(fx.path, *region, fx.indexes["bai"])
    spans = fx.spans(chunks)
    k = [i for i, (z, fu, lu) in enumerate(spans) if fu and lu][0]   # a span that starts and ends inside members
    good = len(fx.brute(*region))

    def run(sp):
        tile, _, seen = ctx.bam_decode_spans(sp, len(fx.lens))
        return ctx.region_view(tile, seen, *region).n_records

    assert run(spans) == good
    z, fu, lu = spans[k]
    for bad in ((z, fu + 1, lu),                                       # a first_uoff inside a record
                (z, fu, lu + 1),                                       # a last_uoff that is not a record start
                (z, 70000, lu), (z, fu, 70000)):                       # offsets outside their members
        with pytest.raises(_lib.TbkError) as e:
            ctx.bam_decode_spans(spans[:k] + [bad] + spans[k + 1:], len(fx.lens))
        assert e.value.status == -1
        assert run(spans) == good                                     # the context takes the next call
    rec = br.synthetic_records()[0]
    short = struct.pack("<I", 31) + rec[4:4 + 31]                     # a block_size of 31
    for payload in (short, rec + short, rec[:-1]):                     # ... first, behind a good record; a record cut short
        with pytest.raises(_lib.TbkError) as e:
            ctx.bam_decode_spans([(_bgzf(payload), 0, 0)], len(fx.lens))
        assert e.value.status == -1
        assert run(spans) == good
    with pytest.raises(_lib.TbkError):                                 # a refID outside the header's references
        ctx.bam_decode_spans([(_bgzf(rec), 0, 0)], 0)
    assert run(spans) == good
    tile, so, _ = ctx.bam_decode_spans([(_bgzf(rec), 0, 0), (_bgzf(rec + rec), 0, len(rec))], len(fx.lens))   # (and good hand-made spans decode)
    assert list(so) == [0, 1, 2]


def test_zero_spans_and_zero_kept_records(ctx, files):
    from tiebrush_amd import api
    fx = files["syn1"].fx
    tile, so, seen = ctx.bam_decode_spans([], len(fx.lens))
    assert int(tile.n_records) == 0 and list(so) == [0] and seen is None
    assert ctx.region_view(tile, seen, 1, 0, 100000).n_records == 0
    assert api.index_query(fx.path, 1, 0, 100000, fx.indexes["bai"]) == []        # chrEmpty: no chunk at all
    chunks = api.index_query(fx.path, 0, 50 * rf.W + 30, 50 * rf.W + 100, fx.indexes["bai"])   # chunks, but no record overlaps
    assert chunks
    tile, so, seen = ctx.bam_decode_spans(fx.spans(chunks), len(fx.lens))
    assert int(tile.n_records) > 0 and ctx.region_view(tile, seen, 0, 50 * rf.W + 30, 50 * rf.W + 100).n_records == 0
    empty = {k: np.zeros(0, dtype=np.float64 if k.endswith("val") else np.uint8 if k == "j_strand" else np.int32) for k in COV_KEYS}
    out = ctx.cov_clip(empty, 0, 0, 100)
    assert out["n_intervals"] == 0 and out["n_junctions"] == 0


def test_long_reference_view(ctx, tmp_path):
    """a 2^31 - 1 reference through its CSI (depth 6): the kept records are the brute-force scan's, up to the last base"""
    from tiebrush_amd import api
    path = str(tmp_path / "long.bam")
    cr.write_bam(path, cr.LONG_NAMES, cr.LONG_LENS, cr.long_records())
    fx = rf.Fixture(path, kinds=("csi",))
    top = (1 << 31) - 1
    regions = [(0, top - 1, top), (0, top - 200, top), (0, (3 << 29) - 50, (3 << 29) + 50), (0, 0, top), (2, 1 << 29, (1 << 29) + 1),
               (2, (1 << 29) - 20, (1 << 29) + 1), (1, 0, 100000)] + rf.random_regions(fx, 4, 20)
    for tid, beg, end in regions:
        tile, _, seen = ctx.bam_decode_spans(fx.spans(api.index_query(path, tid, beg, end)), len(fx.lens))
        assert ctx.region_view(tile, seen, tid, beg, end).n_records == len(fx.brute(tid, beg, end)), (tid, beg, end)


def test_abi_versions_unchanged():
    from tiebrush_amd import _lib
    assert _lib.load().tbk_abi_version() == 9 and _lib.load_host().tbh_abi_version() == 1


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _tiecov(args, **kw):
    return subprocess.run([os.path.join(BIN, "tiecov")] + [str(a) for a in args], capture_output=True, text=True, **kw)


@pytest.fixture(scope="module")
def cli(files, tmp_path_factory):
    """the whole-file run's three tracks of the synthetic file and of t2, once"""
    d = tmp_path_factory.mktemp("gpu_region_cli")
    out = {}
    for name in ("syn0", "syn1", "t2"):
        pre = str(d / name)
        r = _tiecov(["-c", pre + ".c", "-j", pre + ".j", "-s", pre + ".s", files[name].fx.path])
        assert r.returncode == 0, r.stderr
        out[name] = {"c": read_lines(pre + ".c.bedgraph"), "j": read_lines(pre + ".j.bed"), "s": read_lines(pre + ".s.bedgraph")}
    return out


def _cli_regions(name, fx):
    if name == "t2":
        t = fx.recs[len(fx.recs) // 2][0]
        mid = fx.recs[len(fx.recs) // 2][1]
        return [(t, 0, fx.lens[t]), (t, mid, mid + 1), (t, max(0, mid - 5000), mid + 5000), (t, mid + 10, mid + 60)]
    W = rf.W
    return [(0, 30 * W + 1005, 30 * W + 1015), (0, 70 * W + 1060, 70 * W + 2060), (0, W + 150, W + 250), (0, 50 * W - 50, 50 * W + 10),
            (1, 0, 100000), (2, 0, 1000000), (0, 4 * W - 1, 4 * W), (0, (1 << 26) - 30, (1 << 26) + 40)]


@pytest.mark.parametrize("name,via", [("syn0", "bai"), ("syn1", "csi"), ("t2", "bai"), ("t2", "index-file")])
def test_cli_tracks_equal_the_clipped_whole_file_run(files, cli, tmp_path, name, via):
    fx = files[name].fx
    bam = str(tmp_path / "in.bam")
    os.symlink(fx.path, bam)
    extra = []
    if via == "index-file":
        extra = ["--index-file", fx.indexes["csi"]]
    else:
        os.symlink(fx.indexes[via], bam + "." + via)
    junc_seen = 0
    for k, (tid, beg, end) in enumerate(_cli_regions(name, fx)):
        pre = str(tmp_path / ("r%d" % k))
        region = "%s:%s-%d" % (fx.names[tid], format(beg + 1, ","), end)      # (commas in BEG)
        r = _tiecov(["-r" if k % 2 else "--region", region, "-c", pre + ".c", "-j", pre + ".j", "-s", pre + ".s"] + extra + [bam])
        assert r.returncode == 0, r.stderr
        chrom = fx.names[tid]
        assert read_lines(pre + ".c.bedgraph") == rf.clip_track_lines(cli[name]["c"], chrom, beg, end), region
        assert read_lines(pre + ".s.bedgraph") == rf.clip_track_lines(cli[name]["s"], chrom, beg, end), region
        jl = read_lines(pre + ".j.bed")
        assert jl == rf.clip_track_lines(cli[name]["j"], chrom, beg, end, junc=True), region
        assert [l.split("\t")[3] for l in jl[1:]] == ["JUNC%08d" % (i + 1) for i in range(len(jl) - 1)]   # renumbered from 1
        junc_seen += len(jl) - 1
    assert junc_seen > 0


def test_cli_bigwig(files, cli, tmp_path):
    from bigwig_reader import BigWig
    fx = files["t2"].fx
    tid, beg, end = _cli_regions("t2", fx)[2]
    pre = str(tmp_path / "w")
    r = _tiecov(["-W", "-c", pre, "-r", "%s:%d-%d" % (fx.names[tid], beg + 1, end), "--index-file", fx.indexes["bai"], fx.path])
    assert r.returncode == 0, r.stderr
    want = []
    for ln in rf.clip_track_lines(cli["t2"]["c"], fx.names[tid], beg, end)[1:]:
        c, a, b, v = ln.split("\t")
        want.append((c, int(a), int(b), float(np.float32(float(v)))))
    assert want and BigWig(pre + ".bigwig").intervals() == want


def test_cli_errors_leave_no_output(files, tmp_path):
    fx = files["syn1"].fx
    out = tmp_path / "out"
    out.mkdir()
    pre = str(out / "x")
    three = ["-c", pre, "-j", pre, "-s", pre + "s"]
    bam = str(tmp_path / "in.bam")
    os.symlink(fx.path, bam)
    half = str(tmp_path / "half.bam")
    open(half, "wb").write(fx.data[:sorted(fx.msize)[len(fx.msize) // 2]] + cr.EOF_MEMBER)   # (cut at a member that begins with a record)
    other = rf.Fixture(rf.golden_copy(tmp_path, "t2/t2.bam"))
    cases = [(["-r", "chrA:5-10", bam], "no index found"),                                              # no index: the paths tried
             (["-r", "chrA:5-10", "--index-file", other.indexes["bai"], bam], "references"),           # an index of another header
             (["-r", "chrZ", "--index-file", fx.indexes["bai"], bam], "unknown reference name"),
             (["-r", "chrA:x-y", "--index-file", fx.indexes["bai"], bam], "malformed region"),
             (["-r", "chrA:10-5", "--index-file", fx.indexes["bai"], bam], "BEG > END"),
             (["-r", "chrA", "--index-file", fx.indexes["bai"], half], "outside"),                       # a chunk behind the end of the file
             (["-r", "chrA:5-10", "-r", "chrA:7-9", "--index-file", fx.indexes["bai"], bam], "more than once"),
             (["-r", "chrA:5-10", "--region=chrA:7-9", "--index-file", fx.indexes["bai"], bam], "more than once")]
    for args, msg in cases:
        r = _tiecov(three + args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert os.listdir(str(out)) == [], args
    assert bam + ".csi" in _tiecov(three + cases[0][0]).stderr and bam + ".bai" in _tiecov(three + cases[0][0]).stderr


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_cli_without_region_writes_what_it_wrote(tmp_path, name):
    """tiecov without -r: the golden tracks, compared as test_gpu_cli.test_tiecov_cli compares them"""
    pre = str(tmp_path / name)
    r = _tiecov(["-s", pre + ".sample", "-c", pre + ".coverage", "-j", pre + ".junctions", os.path.join(GOLDEN, name, name + ".bam")])
    assert r.returncode == 0, r.stderr

    def norm(lines, col):
        out = []
        for l in lines:
            f = l.split("\t")
            if len(f) > col:
                assert f[col].endswith(".000"), l
                f[col] = f[col][:-4]
            out.append("\t".join(f))
        return out

    assert norm(read_lines(pre + ".coverage.bedgraph"), 3) == read_lines(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"))
    assert norm(read_lines(pre + ".junctions.bed"), 4) == read_lines(os.path.join(GOLDEN, name, name + ".junctions.bed"))
    ours, gold = read_lines(pre + ".sample.bedgraph"), read_lines(os.path.join(GOLDEN, name, name + ".sample.bedgraph"))
    assert ours[0] == gold[0] and ["\t".join(l.split("\t")[:4]) for l in ours[1:]] == ["\t".join(l.split("\t")[:4]) for l in gold[1:]]
