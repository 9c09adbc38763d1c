"""`tiebrush -R BED`: several loci of indexed inputs collapsed in one run on the device.  The contract is `tiebrush -r`'s
with "the region" replaced by the table U: the output is what the same command line without -R makes of inputs in which every file is
replaced by its records that overlap any interval of U, a record that overlaps two of them kept once.  Expected values as in
test_gpu_tiebrush_region.py: bamio's parses filtered in numpy, the oracle on the filtered tile.  Every test fails on a build without the
feature: tbk_tile_regions is missing, -R is an unknown option."""
import os
import subprocess

import numpy as np
import pytest

import bai_reader as br
import csi_reader as cr
import multi_region as mr
import region_fixtures as rf
from helpers import read_lines
from test_gpu_tiebrush_region import (COLS, OPTION_SETS, _assert_tile, _linked, _tiebrush, _region_tile, ctx, merged, overlap_mask,  # noqa: F401
                                      recollapse, samples, select, syn)

pytestmark = pytest.mark.gpu

BIN = rf.BIN
W = rf.W


def table_mask(t, table):
    m = np.zeros(t.n_records, dtype=bool)
    for iv in table:
        m |= overlap_mask(t, *iv)
    return m


def _regions_tile(ctx, inp, order, kind, table, want_md=False, want_names=False):
    """the library's tile of the table for the inputs `order` -> (decoded records, out struct, file_off, numpy columns)"""
    from tiebrush_amd import api
    fspans = [inp.fx[f].spans(api.index_query_regions(inp.fx[f].path, table, inp.fx[f].indexes[kind])) for f in order]
    tb = np.array([inp.tile.tbmerged[f] for f in order], dtype=np.uint8)
    tile, fo = ctx.bam_decode_file_spans(fspans, inp.n_ref, tb, want_md, want_names)
    decoded = int(tile.n_records)
    assert int(fo[-1]) == decoded and int(tile.n_files) == len(order)
    out, fo2 = ctx.tile_regions(tile, table)
    fields = list(COLS)
    if out.yc_in:
        fields += ["yc_in", "yx_in", "yd_in"]
    if out.md_off:
        fields += ["md_off", "md_has"]
    if out.qname_off:
        fields += ["qname_off", "qname_hash"]
    got = ctx.soa_to_numpy(out, fields=tuple(fields)) if int(out.n_records) else {}
    return decoded, out, fo2, got


def _want_tile(inp, order, table):
    sub = inp.sub(order)
    m = table_mask(sub, table)
    base = np.concatenate([np.arange(int(inp.tile.file_off[f]), int(inp.tile.file_off[f + 1])) for f in order])
    return select(sub, m), base[m]


def _check(ctx, inp, order, kind, table, md=False, names=False, records=False):
    assert mr.is_normalised(table), table
    decoded, out, fo, got = _regions_tile(ctx, inp, order, kind, table, md, names)
    want, idx = _want_tile(inp, order, table)
    _assert_tile(got, out, fo, want, (order, kind, table), md, names)
    if records and want.n_records:
        blob, off = ctx.bam_records(np.arange(want.n_records))
        assert blob == inp.raw_records(idx), (order, kind, table)
        pick = np.array([want.n_records - 1, 0, want.n_records // 2])
        assert ctx.bam_records(pick)[0] == inp.raw_records(idx[pick])
    return decoded, want.n_records


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bai", "csi"])
@pytest.mark.parametrize("al", [0, 1])
def test_regions_tile_equals_the_numpy_filter(ctx, syn, al, kind):
    inp = syn[al]
    iso, z = 50 * W - 20, 60 * W + 5
    hand = [[(0, iso + 5, iso + 10), (0, iso + 20, iso + 30)],                          # one record under two intervals: kept once
            [(0, iso - 100, iso), (0, iso + 50, iso + 120)],                            # ends at its pos / begins at its end: out
            [(0, z - 1, z), (0, z + 1, z + 2)], [(0, z, z + 1), (0, z + 100, z + 101)],   # the record of reference length 0: out; in
            [(0, 100, 200), (1, 0, 1000), (2, 6000, 7000)],                             # nothing anywhere
            [(0, W + 100, W + 110), (1, 0, 100), (2, 5000, 5050)],                      # hits under the first and the last entry only
            [(0, 30 * W + 100 + 41 * i, 30 * W + 101 + 41 * i) for i in range(257)]]
    t = inp.tile
    assert int(table_mask(t, hand[0]).sum()) == int(overlap_mask(t, *hand[0][0]).sum()) == int(overlap_mask(t, *hand[0][1]).sum()) >= 1
    assert table_mask(t, hand[1]).sum() == 0 and table_mask(t, hand[2]).sum() == 0 and table_mask(t, hand[3]).sum() >= 1 and table_mask(t, hand[4]).sum() == 0
    filtered = 0
    for k, table in enumerate(hand + [mr.random_table(inp.fx[0], 40 * al + s) for s in range(20)]):
        decoded, kept = _check(ctx, inp, [0, 1, 2, 3], kind, table, records=k % 5 == 0)
        filtered += kept < decoded
    assert filtered > 10


@pytest.mark.parametrize("order", [[3, 0, 1], [0, 3, 1], [0, 1, 3], [3, 3, 3]])
def test_files_without_a_chunk(ctx, syn, order):
    """file 3 holds the last reference only: first, in the middle, last, and every file without a chunk"""
    from tiebrush_amd import api
    inp = syn[1]
    table = [(0, 30 * W + 500, 30 * W + 5003), (0, 31 * W, 31 * W + 10), (1, 0, 50)]
    assert api.index_query_regions(inp.fx[3].path, table, inp.fx[3].indexes["bai"]) == []
    decoded, kept = _check(ctx, inp, order, "bai", table, records=True)
    assert (kept == 0) == (order.count(3) == len(order)) and (decoded == 0) == (kept == 0)


def test_nothing_kept_and_everything_kept(ctx, syn):
    inp = syn[1]
    decoded, kept = _check(ctx, inp, [0, 1, 2], "bai", [(0, 50 * W + 30, 50 * W + 100), (0, 50 * W + 200, 50 * W + 300)])   # chunks decoded, no record overlaps
    assert decoded > 0 and kept == 0
    assert ctx.bam_records(np.zeros(0, np.uint32))[0] == b""
    decoded, kept = _check(ctx, inp, [3, 3], "bai", [(2, 4990, 5001), (2, 5049, 5060)], records=True)   # one record each, under both intervals
    assert decoded == kept == 2


def test_a_table_of_one_equals_the_one_region_entry(ctx, syn):
    inp = syn[0]
    for region in rf.syn_regions()[:12] + rf.random_regions(inp.fx[0], 3, 8):
        d1, out1, fo1, got1 = _region_tile(ctx, inp, [0, 1, 2, 3], "csi", region, True, True)
        n1, c1 = int(out1.n_records), int(out1.n_cigar_ops)
        d2, out2, fo2, got2 = _regions_tile(ctx, inp, [0, 1, 2, 3], "csi", [region], True, True)
        assert (d1, n1, c1, list(fo1)) == (d2, int(out2.n_records), int(out2.n_cigar_ops), list(fo2)), region
        assert set(got1) == set(got2)
        for k in got1:
            assert got1[k].tobytes() == got2[k].tobytes(), (region, k)


def test_an_invalid_table_changes_nothing(ctx, syn):
    from tiebrush_amd import _lib, api
    inp = syn[1]
    good = [(0, 30 * W + 500, 30 * W + 600), (0, 30 * W + 700, 30 * W + 800)]
    fx = inp.fx[0]
    tile, fo = ctx.bam_decode_file_spans([fx.spans(api.index_query_regions(fx.path, good, fx.indexes["bai"]))], inp.n_ref)
    for bad in ([], [good[1], good[0]], [(0, 5, 10), (0, 10, 20)], [(0, 5, 5)], [(-1, 0, 5)]):
        with pytest.raises(_lib.TbkError) as e:
            ctx.tile_regions(tile, bad)
        assert e.value.status == -1
    out, fo2 = ctx.tile_regions(tile, good)                               # the tile is still the context's
    assert int(out.n_records) == int(table_mask(inp.sub([0]), good).sum()) > 0


@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_merged_inputs_carry_yd_md_and_names(ctx, merged, kind):
    """t1.bam + plain + t2.bam: the tag, MD and QNAME columns of the kept records"""
    inp = merged
    t = inp.fx[2].recs[len(inp.fx[2].recs) // 3]
    tables = [[(t[0], max(0, t[1] - 3000), t[1] - 100), (t[0], t[1] + 10, t[1] + 3000)], [(t[0], 0, inp.fx[2].lens[t[0]]), (57, 0, inp.fx[2].lens[57])]] + \
        [mr.random_table(inp.fx[2], 9 + s) for s in range(4)]
    yd_seen = 0
    for k, table in enumerate(tables):
        decoded, out, fo, got = _regions_tile(ctx, inp, [0, 1, 2], kind, table, True, True)
        want, idx = _want_tile(inp, [0, 1, 2], table)
        if want.n_records:
            yd_seen += int((want.yd_in > 0).sum())
        _assert_tile(got, out, fo, want, (kind, table), md=True, names=True)
        if k < 2 and want.n_records:
            assert ctx.bam_records(np.arange(want.n_records))[0] == inp.raw_records(idx)
    assert yd_seen > 0


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _assert_output(inp, table, okw, out_path, stderr):
    """the record stream and YC / YX / YD of out_path equal the oracle's collapse of the filtered inputs"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import bamio
    m = table_mask(inp.tile, table)
    idx = np.flatnonzero(m)
    want = orc.collapse(select(inp.tile, m), **okw)
    o = bamio.read_bam(out_path)
    assert o.n == want["n_groups"]
    assert "%d input records written as %d" % (want["n_passed"], want["n_groups"]) in stderr
    fo = inp.tile.file_of()
    for g in range(o.n):
        gi = int(idx[int(want["rep"][g])])
        f = int(fo[gi])
        i = gi - int(inp.tile.file_off[f])
        assert bamio.record_identity(o, g) == bamio.record_identity(inp.bams[f], i), g
        assert o.yx[g] == want["yx"][g] and o.yd[g] == want["yd"][g], g
        if not inp.bams[f].has_yc[i]:
            assert o.has_yc[g] and np.float32(o.yc[g]) == np.float32(want["yc"][g]), g
    return o.n, int(m.sum())


def _loci(inp):
    """three loci inside the samples' 8 kb, given unsorted, two of them overlapping: a table of two"""
    recs = inp.fx[0].recs
    a, b = recs[len(recs) // 3], recs[(2 * len(recs)) // 3]
    return [(b[0], b[1] - 100, b[1] + 100), (a[0], a[1] - 150, a[1] + 50), (a[0], a[1], a[1] + 150)]


@pytest.mark.parametrize("flags,okw", [OPTION_SETS[i] for i in (0, 1, 4, 6)], ids=["default", "L", "A", "N5_Q1"])
def test_cli_loci_of_ten_inputs(samples, tmp_path, flags, okw):
    iv = _loci(samples)
    table = mr.normalise(iv, samples.fx[0].lens)
    assert len(table) == 2
    bed = mr.write_bed(str(tmp_path / "loci.bed"), samples.fx[0].names, iv, extra=["locus"])
    for writer, kind, opt in (("device", "bai", "-R"), ("host", "csi", "--regions-file")):
        paths = _linked(tmp_path, samples, kind, kind)
        out = str(tmp_path / (writer + ".bam"))
        r = _tiebrush([opt, bed, "--writer", writer, "-o", out] + flags + paths, env=dict(TBK_TIMING="1"))
        assert r.returncode == 0, r.stderr
        n_out, n_in = _assert_output(samples, table, okw, out, r.stderr)
        assert 0 < n_out and 0 < n_in < samples.tile.n_records // 2
        assert "region path ms: index queries" in r.stderr and "(2 regions)" in r.stderr and "chunks of 10 inputs" in r.stderr


@pytest.mark.parametrize("flags,okw", [OPTION_SETS[i] for i in (0, 1, 4, 6)], ids=["default", "L", "A", "N5_Q1"])
def test_cli_merged_inputs(recollapse, tmp_path, flags, okw):
    """t1.bam t2.bam are TieBrush outputs: their YC / YX / YD are carried into the groups of every interval"""
    inp = recollapse
    t = inp.fx[1].recs[len(inp.fx[1].recs) // 3]
    table = mr.normalise([(t[0], max(0, t[1] - 2000), t[1] - 50), (t[0], t[1] + 50, t[1] + 2000), (57, 0, inp.fx[1].lens[57])], inp.fx[1].lens)
    assert len(table) == 3
    bed = mr.write_bed(str(tmp_path / "m.bed"), inp.fx[0].names, table[::-1])
    for k, (writer, kind) in enumerate([("device", "csi"), ("host", "bai")]):
        out = str(tmp_path / ("m%d.bam" % k))
        r = _tiebrush(["-R", bed, "--writer", writer, "-o", out] + flags + _linked(tmp_path, inp, kind, kind))
        assert r.returncode == 0, r.stderr
        n_out, n_in = _assert_output(inp, table, okw, out, r.stderr)
        assert 0 < n_out <= n_in < inp.tile.n_records


def test_cli_index_tracks_and_an_empty_selection(samples, tmp_path):
    """--index: OUT.bam.bai is bai_reader's index of OUT.bam; --cov --junc --samp: tiecov -c -j -s OUT.bam's files, not clipped; a table
    that selects nothing: a valid BAM of header + EOF member"""
    iv = _loci(samples)
    bed = mr.write_bed(str(tmp_path / "loci.bed"), samples.fx[0].names, iv)
    paths = _linked(tmp_path, samples, "csi", "i")
    out, pre = str(tmp_path / "o.bam"), str(tmp_path / "t")
    r = _tiebrush(["-R", bed, "--index", "--cov", pre + ".c", "--junc", pre + ".j", "--samp", pre + ".s", "-o", out] + paths)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    bai = open(out + ".bai", "rb").read()
    assert bai == br.expected_bai(data)
    br.validate(data, bai)
    ref = str(tmp_path / "ref")
    tc = os.path.join(BIN, "tiecov")
    subprocess.run([tc, "-c", ref + ".c", "-j", ref + ".j", "-s", ref + ".s", out], check=True, capture_output=True)
    for ext in (".c.bedgraph", ".j.bed", ".s.bedgraph"):
        assert open(pre + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    assert len(read_lines(pre + ".c.bedgraph")) > 2
    out2 = str(tmp_path / "o2.bam")
    r = _tiebrush(["-R", bed, "--csi", "--writer", "host", "-o", out2] + paths)
    assert r.returncode == 0 and os.path.exists(out2 + ".csi"), r.stderr
    none = mr.write_bed(str(tmp_path / "none.bed"), samples.fx[0].names, [(0, 1000, 2000), (0, 5000, 6000), (1, 10, 20)])
    for writer in ("device", "host"):
        out3 = str(tmp_path / ("empty_%s.bam" % writer))
        r = _tiebrush(["-R", none, "--writer", writer, "--index", "-o", out3] + paths)
        assert r.returncode == 0, r.stderr
        assert "0 input records written as 0 (0.00% reduction)" in r.stderr and "nan" not in r.stderr
        d3 = open(out3, "rb").read()
        names, lens, recs, _ = br.read_bam(d3)
        assert recs == [] and names == samples.fx[0].names and d3.endswith(cr.EOF_MEMBER)
        assert open(out3 + ".bai", "rb").read() == br.expected_bai(d3)
