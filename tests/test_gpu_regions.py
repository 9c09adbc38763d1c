"""`tiecov -R BED`: the tracks of several regions in one run, on the device.  The contract is an identity: the interval
rows equal the whole-file run's rows intersected with the table U (a row trimmed to each interval it meets), the junction rows are the
whole-file run's that overlap any interval, once.  Expected rows are the ORACLE's whole-file rows clipped by multi_region.py; kept counts
are the brute-force filter's.  Every test fails on a build without the feature (the entries and the option do not exist there)."""
import os

import numpy as np
import pytest

import csi_reader as cr
import multi_region as mr
import region_fixtures as rf
from helpers import read_lines
from test_gpu_region import COV_KEYS, SAMP_KEYS, _assert_rows, _tiecov, cli, ctx, files  # noqa: F401  (fixtures and helpers of `tiecov -r`)

pytestmark = pytest.mark.gpu

W = rf.W
IV_KEYS = COV_KEYS[:4]
VIEW_FIELDS = ("tid", "pos", "flag", "strand", "cig_off", "cig", "yc_in", "yx_in")


def _view_arrays(ctx, view):
    """the arrays of a device view (they live until the context's next view) as numpy"""
    from tiebrush_amd import _lib
    v, s = view.struct, _lib.SoaIn()
    s.n_records, s.n_cigar_ops = v.n_records, v.n_cigar_ops
    s.tid, s.pos, s.flag, s.strand, s.cig_off, s.cig, s.yc_in, s.yx_in = v.tid, v.pos, v.flag, v.strand, v.cig_off, v.cig, v.yc, v.yx
    return ctx.soa_to_numpy(s, fields=VIEW_FIELDS) if view.n_records else {}


def _decode(ctx, fx, index, table):
    from tiebrush_amd import api
    chunks = api.index_query_regions(fx.path, table, index)
    tile, span_off, seen = ctx.bam_decode_spans(fx.spans(chunks), len(fx.lens))
    assert int(span_off[-1]) == int(tile.n_records) == len(fx.in_chunks(chunks))
    return tile, seen


def _table_rows(ctx, fx, index, table, ns):
    """the table path of the library: (n_kept, coverage rows, sample rows) as numpy"""
    from tiebrush_amd import api
    tile, seen = _decode(ctx, fx, index, table)
    view = ctx.regions_view(tile, seen, table)
    if view.n_records == 0:
        return 0, {k: np.zeros(0) for k in COV_KEYS}, {k: np.zeros(0) for k in SAMP_KEYS}
    cov = ctx.cov_clip_regions(ctx.coverage(view), table)              # device rows, cut on the device
    samp = ctx.sample_clip_regions(ctx.sample(view, ns), table)
    return view.n_records, api.to_numpy(cov), api.to_numpy(samp)


def _check_table(ctx, wh, kind, table):
    assert mr.is_normalised(table), table
    fx = wh.fx
    n_kept, cov, samp = _table_rows(ctx, fx, fx.indexes[kind], table, wh.ns)
    assert n_kept == len(mr.brute(fx.recs, table)), (kind, table)
    want = mr.clip_cov_union(wh.rows, table)
    _assert_rows(cov, want, COV_KEYS, (kind, table))
    _assert_rows(samp, mr.clip_sample_union(wh.rows, table), SAMP_KEYS, (kind, table))
    return n_kept, want


# ---- R = 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_one_interval_equals_the_one_region_entries(ctx, files, kind):
    """for every hand-picked region: the view, the coverage clip and the sample clip of the table of one equal their one-region siblings,
    array for array (the tile is decoded once: neither view consumes it)"""
    from tiebrush_amd import api
    wh = files["syn1"]
    fx = wh.fx
    seen_rows = 0
    for tid, beg, end in rf.syn_regions():
        table = [(tid, beg, end)]
        tile, seen = _decode(ctx, fx, fx.indexes[kind], table)
        one = ctx.region_view(tile, seen, tid, beg, end)
        a = _view_arrays(ctx, one)
        many = ctx.regions_view(tile, seen, table)
        b = _view_arrays(ctx, many)
        assert one.n_records == many.n_records and one.n_cigar_ops == many.n_cigar_ops, table
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (table, k)
        if many.n_records == 0:
            continue
        cov, samp = ctx.coverage(many), ctx.sample(many, wh.ns)
        _assert_rows(api.to_numpy(ctx.cov_clip_regions(cov, table)), api.to_numpy(ctx.cov_clip(cov, tid, beg, end)), COV_KEYS, table)
        _assert_rows(api.to_numpy(ctx.sample_clip_regions(samp, table)), api.to_numpy(ctx.sample_clip(samp, tid, beg, end)), SAMP_KEYS, table)
        seen_rows += many.n_records
    assert seen_rows > 0


# ---- hand-built tables -----------------------------------------------------------------------------------------------------------------------
def _long_row(rows, tid=0, least=12):
    k = int(np.flatnonzero((rows["iv_tid"] == tid) & (rows["iv_end"] - rows["iv_start"] >= least))[0])
    return k, int(rows["iv_start"][k]), int(rows["iv_end"][k])


@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_hand_built_tables(ctx, files, kind):
    wh = files["syn1"]
    fx, rows = wh.fx, wh.rows
    # two intervals inside one interval row: the row comes out twice, trimmed differently
    k, s, e = _long_row(rows)
    table = [(0, s + 2, s + 5), (0, s + 7, s + 10)]
    n, want = _check_table(ctx, wh, kind, table)
    assert list(want["iv_start"]) == [s + 2, s + 7] and list(want["iv_end"]) == [s + 5, s + 10] and want["iv_val"][0] == want["iv_val"][1] == rows["iv_val"][k]
    # the second interval one base after the first ends: two intervals, two rows; at its end: one interval, one row
    apart = mr.normalise([(0, s + 2, s + 5), (0, s + 6, s + 9)], fx.lens)
    n, want = _check_table(ctx, wh, kind, apart)
    assert len(apart) == 2 and list(want["iv_start"]) == [s + 2, s + 6]
    joined = mr.normalise([(0, s + 2, s + 5), (0, s + 5, s + 9)], fx.lens)
    n, want = _check_table(ctx, wh, kind, joined)
    assert joined == [(0, s + 2, s + 9)] and list(want["iv_start"]) == [s + 2] and list(want["iv_end"]) == [s + 9]
    # a record that overlaps two intervals is kept once
    iso = 50 * W - 20
    table = [(0, iso + 5, iso + 10), (0, iso + 20, iso + 30)]
    assert fx.brute(*table[0]) == fx.brute(*table[1]) and len(fx.brute(*table[0])) == 1
    n, want = _check_table(ctx, wh, kind, table)
    assert n == 1 and len(want["iv_tid"]) == 2
    # a junction whose intron contains both intervals: no coverage row, the junction once
    intron = 70 * W + 10 + 50
    table = [(0, intron + 1000, intron + 2000), (0, intron + 5000, intron + 6000)]
    n, want = _check_table(ctx, wh, kind, table)
    assert n == 1 and len(want["iv_tid"]) == 0 and len(want["j_tid"]) == 1
    assert want["j_start"][0] < table[0][1] and want["j_end"][0] > table[1][2]
    # ... and one that overlaps two intervals at its two ends
    table = [(0, intron - 10, intron + 5), (0, intron + 700000 - 5, intron + 700000 + 10)]
    n, want = _check_table(ctx, wh, kind, table)
    assert len(want["j_tid"]) == 1 and len(want["iv_tid"]) == 2
    # the record of reference length 0 at 60 W + 5, one base either side of an interval edge
    z = 60 * W + 5
    far = (0, z + 1000, z + 1001)
    for table, kept in (([(0, z - 1, z), far], 0), ([(0, z, z + 1), far], 1), ([(0, z + 1, z + 2), far], 0), ([(0, z - 5, z + 1), far], 1)):
        assert len(mr.brute(fx.recs, table)) == kept
        assert _check_table(ctx, wh, kind, table)[0] == kept
    # intervals before the first record, behind the last, on a reference without records, beyond the linear index
    nothing = [(0, 100, 200), (1, 0, 1000), (2, 6000, 7000), (2, 500000, 600000)]
    assert _check_table(ctx, wh, kind, nothing)[0] == 0
    # a table whose only hits are its first and its last entry
    table = [(0, W + 100, W + 110), (0, 50 * W + 30, 50 * W + 100), (1, 0, 100), (2, 4000, 4100), (2, 5000, 5050)]
    hits = [len(fx.brute(*iv)) for iv in table]
    assert hits[0] > 0 and hits[-1] > 0 and hits[1:-1] == [0, 0, 0]
    assert _check_table(ctx, wh, kind, table)[0] == hits[0] + hits[-1]


# ---- block edges of the new kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [255, 256, 257])
def test_tables_and_clip_outputs_at_block_edges(ctx, files, R):
    """one-base intervals over the bulk's covered ground: a table of R intervals, and a clip whose output is R rows (one per interval)"""
    wh = files["syn0"]
    table = [(0, 30 * W + 100 + 41 * i, 30 * W + 101 + 41 * i) for i in range(R)]
    n, want = _check_table(ctx, wh, "bai", table)
    assert n > R and len(want["iv_tid"]) == R and len(mr.clip_sample_union(wh.rows, table)["s_tid"]) == R


def _count_file(path, n):
    """n records of 40 bases, two at every position from 1000 on, on one reference: all of them in the first 16 kb window (one bin, so
    any query of the window decodes them all)"""
    from tiebrush_amd import bamio
    assert 1000 + n // 2 + 40 < W
    recs = [bamio.encode_record(0, 1000 + i // 2, 0, 60, [40 << 4], b"c%d" % i, aux=b"NHC\x01") for i in range(n)]
    cr.write_bam(path, ["chrC"], [1000000], recs)
    return rf.Fixture(path, kinds=("bai",))


@pytest.mark.parametrize("n", [254, 255, 256, 257, 16383, 16384, 16385])
def test_tile_lengths_at_block_and_scan_edges(ctx, tmp_path, n):
    """the flag kernel and the scans run over n + 1 elements: n + 1 around 256 (one block), and around 16384 (the scans' switch)"""
    fx = _count_file(str(tmp_path / "c.bam"), n)
    last = 1000 + (n - 1) // 2
    table = [(0, 0, 1001), (0, 1100, 1103), (0, last + 38, last + 39), (0, last + 40, last + 500)]
    tile, seen = _decode(ctx, fx, fx.indexes["bai"], table)
    assert int(tile.n_records) == n
    view = ctx.regions_view(tile, seen, table)
    want = mr.brute(fx.recs, table)
    assert view.n_records == len(want) and 0 < len(want) < n
    got = _view_arrays(ctx, view)
    assert list(got["pos"]) == [r[1] for r in want] and got["cig_off"][-1] == len(want) == len(got["cig"])


# ---- capacity and refusals ----------------------------------------------------------------------------------------------------------------------
def _three_rows(rows, keys, prefix):
    """a row of reference 0 at least 12 bases long with a neighbour on either side, and those two: (the three rows, the middle one's start)"""
    tid, start, end = rows[prefix + "tid"], rows[prefix + "start"], rows[prefix + "end"]
    ok = (tid[1:-1] == 0) & (end[1:-1] - start[1:-1] >= 12) & (tid[:-2] == 0) & (tid[2:] == 0)
    k = int(np.flatnonzero(ok)[0]) + 1
    return {key: np.array(rows[key][k - 1:k + 2], copy=True) for key in keys}, int(start[k])


@pytest.mark.parametrize("where", ["host", "device"])
def test_rows_that_grow_beyond_their_capacity(ctx, files, where):
    """three rows, a table that cuts the middle one in two: four rows are needed.  With room for three the call is TBK_E2BIG, no row is
    touched, the count needed is reported, and the context takes the next call"""
    import torch
    from tiebrush_amd import _lib, api
    wh = files["syn1"]
    for keys, prefix, clip in ((IV_KEYS, "iv_", ctx.cov_clip_regions), (SAMP_KEYS, "s_", ctx.sample_clip_regions)):
        rows, s = _three_rows(wh.rows, keys, prefix)
        assert rows[prefix + "tid"][0] == rows[prefix + "tid"][2] == 0
        table = [(0, int(rows[prefix + "start"][0]), s + 5), (0, s + 7, int(rows[prefix + "end"][2]))]
        give = {k: (torch.from_numpy(v).cuda() if where == "device" else v) for k, v in rows.items()}
        with pytest.raises(_lib.TbkError) as e:
            clip(give, table, cap_intervals=3)
        assert e.value.status == -4 and e.value.needed == 4
        for k in keys:
            assert api.to_numpy(e.value.rows)[k].tobytes() == rows[k].tobytes(), k          # untouched
        want = (mr.clip_cov_union if prefix == "iv_" else mr.clip_sample_union)(
            dict(rows, **{k: np.zeros(0, np.int32) for k in COV_KEYS[4:]}) if prefix == "iv_" else rows, table)
        for cap in (4, None):
            got = api.to_numpy(clip(give, table, cap_intervals=cap))
            _assert_rows(got, want, keys, (where, prefix, cap))
            assert len(got[prefix + "tid"]) == 4
        swapped = {k: (v.flip(0) if where == "device" else v[::-1].copy()) for k, v in give.items()}   # rows that are not sorted
        with pytest.raises(_lib.TbkError) as e:
            clip(swapped, table)
        assert e.value.status == -1
        assert len(api.to_numpy(clip(give, table))[prefix + "tid"]) == 4                  # the context takes the next call


def test_tables_that_are_not_normalised_are_refused(ctx, files):
    from tiebrush_amd import _lib
    wh = files["syn1"]
    fx = wh.fx
    good = [(0, 30 * W + 100, 30 * W + 200), (0, 30 * W + 300, 30 * W + 400)]
    tile, seen = _decode(ctx, fx, fx.indexes["bai"], good)
    n = ctx.regions_view(tile, seen, good).n_records
    rows = {k: wh.rows[k] for k in COV_KEYS}
    for bad in ([], [(0, 100, 200), (0, 200, 300)], [(0, 100, 200), (0, 150, 300)], [(0, 300, 400), (0, 100, 200)], [(1, 0, 5), (0, 0, 5)],
                [(0, 100, 100)], [(-1, 0, 5)], [(0, -3, 5)]):
        for call in (lambda: ctx.regions_view(tile, seen, bad), lambda: ctx.cov_clip_regions(rows, bad),
                     lambda: ctx.sample_clip_regions({k: wh.rows[k] for k in SAMP_KEYS}, bad)):
            with pytest.raises(_lib.TbkError) as e:
                call()
            assert e.value.status == -1, bad
    assert ctx.regions_view(tile, seen, good).n_records == n > 0          # nothing was changed: the tile is still there


# ---- random and golden tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bai", "csi"])
@pytest.mark.parametrize("name", ["syn0", "syn1"])
def test_random_tables_on_the_synthetic_files(ctx, files, name, kind):
    wh = files[name]
    kept = 0
    for seed in range(20):
        table = mr.random_table(wh.fx, 31 * seed + (kind == "csi"))
        kept += _check_table(ctx, wh, kind, table)[0]
    assert kept > 0


@pytest.mark.parametrize("name", ["t2", "t1s0"])
def test_random_tables_on_the_goldens(ctx, files, name):
    """YC / YX present (t2) and absent (t1s0)"""
    wh = files[name]
    fx = wh.fx
    tids = sorted(set(r[0] for r in fx.recs))
    _check_table(ctx, wh, "bai", [(t, 0, fx.lens[t]) for t in tids[:3]])                 # whole references
    for kind in ("bai", "csi"):
        for seed in range(20 if kind == "bai" else 4):
            _check_table(ctx, wh, kind, mr.random_table(fx, seed))


def test_clip_of_host_rows_over_several_references(ctx, files):
    wh = files["t2"]
    rows = {k: wh.rows[k] for k in COV_KEYS}
    srows = {k: wh.rows[k] for k in SAMP_KEYS}
    for seed in range(10):
        table = mr.random_table(wh.fx, 50 + seed, lo=2, hi=60)
        _assert_rows(ctx.cov_clip_regions(rows, table), mr.clip_cov_union(wh.rows, table), COV_KEYS, table)
        _assert_rows(ctx.sample_clip_regions(srows, table), mr.clip_sample_union(wh.rows, table), SAMP_KEYS, table)
    assert np.array_equal(rows["iv_start"], wh.rows["iv_start"])


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def _cli_intervals(name, fx):
    """as a user writes them: unsorted, with overlaps, a nested one, two that abut and an empty one"""
    if name == "t2":
        t, mid = fx.recs[len(fx.recs) // 2][0], fx.recs[len(fx.recs) // 2][1]
        other = sorted(set(r[0] for r in fx.recs) - {t})[0]            # (a second reference, whole)
        return [(t, mid + 10, mid + 60), (t, max(0, mid - 5000), mid), (t, mid - 100, mid + 20), (other, 0, fx.lens[other]), (t, mid + 60, mid + 90), (t, 7, 7)]
    return [(2, 0, 1000000), (0, 70 * W + 1060, 70 * W + 2060), (0, 30 * W + 1005, 30 * W + 1015), (0, 30 * W + 1010, 30 * W + 1100), (0, W + 150, W + 250),
            (0, 30 * W + 1100, 30 * W + 1200), (1, 0, 100000), (0, 50 * W - 50, 50 * W + 10), (0, (1 << 26) - 30, (1 << 26) + 40), (0, 30 * W + 1020, 30 * W + 1030)]


@pytest.mark.parametrize("name,via", [("syn0", "bai"), ("syn1", "csi"), ("t2", "bai"), ("t2", "index-file")])
def test_cli_tracks_equal_the_clipped_whole_file_run(files, cli, tmp_path, name, via):  # noqa: F811
    fx = files[name].fx
    bam = str(tmp_path / "in.bam")
    os.symlink(fx.path, bam)
    extra = []
    if via == "index-file":
        extra = ["--index-file", fx.indexes["csi"]]
    else:
        os.symlink(fx.indexes[via], bam + "." + via)
    iv = _cli_intervals(name, fx)
    table = mr.normalise(iv, fx.lens)
    assert 2 <= len(table) < len(iv)
    bed = mr.write_bed(str(tmp_path / "r.bed"), fx.names, iv, extra=["gene\t0\t+", ""], head=["# panel", "track name=panel"])
    pre = str(tmp_path / "o")
    r = _tiecov(["-R" if via != "csi" else "--regions-file", bed, "-c", pre + ".c", "-j", pre + ".j", "-s", pre + ".s"] + extra + [bam], env=dict(os.environ, TBK_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert "tiecov -R phases ms: %d regions" % len(table) in r.stderr
    assert read_lines(pre + ".c.bedgraph") == mr.clip_track_lines_union(cli[name]["c"], fx.names, table)
    assert read_lines(pre + ".s.bedgraph") == mr.clip_track_lines_union(cli[name]["s"], fx.names, table)
    jl = read_lines(pre + ".j.bed")
    assert jl == mr.clip_track_lines_union(cli[name]["j"], fx.names, table, junc=True)
    assert (len(jl) > 1 or name == "t2") and [l.split("\t")[3] for l in jl[1:]] == ["JUNC%08d" % (i + 1) for i in range(len(jl) - 1)]
    assert len(read_lines(pre + ".c.bedgraph")) > len(table)


def test_cli_bigwig_one_region_and_no_region(files, cli, tmp_path):  # noqa: F811
    from bigwig_reader import BigWig
    fx = files["t2"].fx
    iv = _cli_intervals("t2", fx)
    table = mr.normalise(iv, fx.lens)
    bed = mr.write_bed(str(tmp_path / "r.bed"), fx.names, iv)
    pre = str(tmp_path / "w")
    r = _tiecov(["-W", "-c", pre, "-R", bed, "--index-file", fx.indexes["bai"], fx.path])
    assert r.returncode == 0, r.stderr
    want = []
    for ln in mr.clip_track_lines_union(cli["t2"]["c"], fx.names, table)[1:]:
        c, a, b, v = ln.split("\t")
        want.append((c, int(a), int(b), float(np.float32(float(v)))))
    assert want and BigWig(pre + ".bigwig").intervals() == want
    # -r writes what -R writes for a BED of that one region, byte for byte; tiecov without either writes the whole-file tracks
    tid, beg, end = table[0]
    one = mr.write_bed(str(tmp_path / "one.bed"), fx.names, [table[0]])
    for opt, val, tag in (("-r", "%s:%d-%d" % (fx.names[tid], beg + 1, end), "a"), ("-R", one, "b")):
        r = _tiecov([opt, val, "-c", str(tmp_path / tag), "-j", str(tmp_path / tag), "--index-file", fx.indexes["csi"], fx.path])
        assert r.returncode == 0, r.stderr
    for ext in (".bedgraph", ".bed"):
        assert open(str(tmp_path / "a") + ext, "rb").read() == open(str(tmp_path / "b") + ext, "rb").read()
    assert read_lines(str(tmp_path / "a.bedgraph")) == rf.clip_track_lines(cli["t2"]["c"], fx.names[tid], beg, end)
    r = _tiecov(["-c", str(tmp_path / "p"), fx.path])
    assert r.returncode == 0 and read_lines(str(tmp_path / "p.bedgraph")) == cli["t2"]["c"]


def test_cli_errors_leave_no_output(files, tmp_path):
    fx = files["syn1"].fx
    out = tmp_path / "out"
    out.mkdir()
    pre = str(out / "x")
    three = ["-c", pre, "-j", pre, "-s", pre + "s"]
    bed = mr.write_bed(str(tmp_path / "r.bed"), fx.names, [(0, 100, 200), (0, 30 * W, 40 * W)])
    half = str(tmp_path / "half.bam")
    open(half, "wb").write(fx.data[:sorted(fx.msize)[len(fx.msize) // 2]] + cr.EOF_MEMBER)
    other = rf.Fixture(rf.golden_copy(tmp_path, "t2/t2.bam"))
    ix = ["--index-file", fx.indexes["bai"]]
    bad = str(tmp_path / "bad.bed")
    open(bad, "w").write("chrA\t5\t10\nchrA\tfive\t10\n")
    cases = [(["-R", bed, "--index-file", other.indexes["bai"], fx.path], "references"),
             (["-R", bed] + ix + [half], "outside"),
             (["-R", bad] + ix + [fx.path], "bad.bed line 2"),
             (["-R", bed, "-r", "chrA:5-10"] + ix + [fx.path], "do not go together"),
             (["-R", bed, "-R", bed] + ix + [fx.path], "more than once")]
    for args, msg in cases:
        r = _tiecov(three + args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert os.listdir(str(out)) == [], args
