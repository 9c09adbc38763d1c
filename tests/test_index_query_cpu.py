"""The index reader and region parser behind `tiecov -r` (csrc/host/bai_read.h) on the host alone: `tbh_tool query` and
tbh_index_query against the tests' own readers (bai_reader.py / csi_reader.py) and a brute-force scan, through .bai and .csi at depths 0,
1, 5 and 6; the region parser's accepted forms and refusals; index discovery; refusals of a wrong or damaged index.  CPU only."""
import os
import shutil

import pytest

import bai_reader as br
import csi_reader as cr
import region_fixtures as rf
from tiebrush_amd import api


def _tool_query(fx, region, index=None):
    r = rf.tool("query", fx.path, region, *([index] if index else []))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    tid, beg, end = (int(x) for x in lines[0].split()[1:])
    chunks = [tuple(int(x, 16) for x in l.split()) for l in lines[1:] if l and l[0] in "0123456789abcdef" and len(l.split()) == 2]
    n_rec = int([l for l in lines if l.startswith("records ")][0].split()[1])
    n_hit = int([l for l in lines if l.startswith("overlapping ")][0].split()[1])
    hits = [int(l.split()[1], 16) for l in lines if l.startswith("hit ")]
    assert n_hit == len(hits)
    return (tid, beg, end), chunks, n_rec, hits


def _check(fx, kind, regions, n_tool):
    """every region through tbh_index_query; the first n_tool of them through `tbh_tool query` as well (a process each)"""
    ix = fx.indexes[kind]
    data_ix = open(ix, "rb").read()
    for k, (tid, beg, end) in enumerate(regions):
        want = fx.brute(tid, beg, end)
        chunks = api.index_query(fx.path, tid, beg, end, ix)
        idx = fx.in_chunks(chunks)                                   # sorted, disjoint, cut at record starts
        assert len(idx) == len(set(idx))                              # no record twice
        found = [fx.recs[i] for i in idx if fx.recs[i][0] == tid and fx.recs[i][1] < end and fx.recs[i][2] > beg]
        assert found == want, (kind, tid, beg, end)
        if k < n_tool:
            # the tests' own reader finds the same records through the same index (plain Python: a few regions per file)
            mine = br.query(fx.data, data_ix, tid, beg, end) if kind == "bai" else cr.query(fx.data, data_ix, tid, beg, end)
            assert mine == want
            reg, tchunks, n_rec, hits = _tool_query(fx, "%s:%d-%d" % (fx.names[tid], beg + 1, end), ix)
            assert reg == (tid, beg, end) and tchunks == chunks
            assert n_rec == len(idx) and hits == [r[3] for r in want]


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    d = tmp_path_factory.mktemp("region_syn")
    return {al: rf.Fixture(rf.write_syn(str(d / ("syn%d.bam" % al)), br.SYN_NAMES, br.SYN_LENS, br.synthetic_records(), al)) for al in (0, 1)}


@pytest.mark.parametrize("aligned", [0, 1])
@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_synthetic_file(syn, kind, aligned):
    """depth 5 (.bai) and depth 6 (.csi: the longest reference is 2^29) on both member layouts"""
    fx = syn[aligned]
    assert len(br.members(fx.data)) >= 10
    hand = rf.syn_regions()
    _check(fx, kind, hand + rf.random_regions(fx, 11 + aligned, 40), n_tool=12)
    # the nested parent-bin chunk: the region of the first leaf run is one chunk, and its records are read once
    chunks = api.index_query(fx.path, 0, rf.W + 150, rf.W + 250, fx.indexes[kind])
    assert len(fx.in_chunks(chunks)) == len(set(fx.in_chunks(chunks)))


@pytest.mark.parametrize("name", ["t1/t1.bam", "t2/t2.bam", "t12.bam", "t1/t1s0.bam"])
def test_goldens(tmp_path, name):
    fx = rf.Fixture(rf.golden_copy(tmp_path, name))
    whole = [(t, 0, fx.lens[t]) for t in sorted(set(r[0] for r in fx.recs))[:3]]
    for kind in ("bai", "csi"):
        _check(fx, kind, rf.random_regions(fx, 5, 40) + whole, n_tool=3)


def test_long_file_depth_6(tmp_path):
    """a 2^31 - 1 reference: CSI only, bins above 2^16, regions across 2^29 and up to the last base"""
    path = str(tmp_path / "long.bam")
    cr.write_bam(path, cr.LONG_NAMES, cr.LONG_LENS, cr.long_records())
    fx = rf.Fixture(path, kinds=("csi",))
    top = (1 << 31) - 1
    extra = [(0, (1 << 29) - 100, (1 << 29) + 100), (0, (3 << 29) - 50, (3 << 29) + 50), (0, 3 << 29, top), (0, top - 1, top), (0, top - 200, top),
             (0, 0, top), (0, 1 << 30, top), (2, (1 << 29) - 20, (1 << 29) + 1), (2, 1 << 29, (1 << 29) + 1), (2, 0, 1 << 29), (1, 0, 100000)]
    _check(fx, "csi", extra + rf.random_regions(fx, 9, 40), n_tool=6)
    assert rf.tool("bai", path).returncode != 0                      # (no .bai for this file: the region path has to take the .csi)


@pytest.mark.parametrize("ref_len,depth", [(10000, 0), (100000, 1)])
def test_depth_0_and_1(tmp_path, ref_len, depth):
    path = str(tmp_path / "small.bam")
    cr.write_bam(path, ["chrS"], [ref_len], cr.small_records(ref_len))
    fx = rf.Fixture(path)
    assert cr.parse_csi(open(fx.indexes["csi"], "rb").read())[0] == depth
    regions = [(0, 0, ref_len), (0, ref_len - 1, ref_len), (0, 0, 1), (0, 16383, 16385)] + rf.random_regions(fx, depth, 30)
    regions = [(t, b, min(e, ref_len)) for t, b, e in regions if b < min(e, ref_len)]
    for kind in ("bai", "csi"):
        _check(fx, kind, regions, n_tool=3)


# ---- the region parser ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colon(tmp_path_factory):
    """two references, "chr" and "chr:1" (a name that holds a colon), records on the first"""
    path = str(tmp_path_factory.mktemp("region_colon") / "colon.bam")
    cr.write_bam(path, ["chr", "chr:1"], [100000, 50000], cr.small_records(100000))
    return rf.Fixture(path)


@pytest.mark.parametrize("region,want", [
    ("chr", (0, 0, 100000)), ("chr:1", (1, 0, 50000)),               # the whole string is a name first
    ("chr:5", (0, 4, 100000)), ("chr:5-10", (0, 4, 10)), ("chr:1:5-10", (1, 4, 10)), ("chr:1:7", (1, 6, 50000)),
    ("chr:1,000-2,000", (0, 999, 2000)), ("chr:99,000-200000", (0, 98999, 100000)),   # commas; END cut to the reference
    ("chr:1-1", (0, 0, 1)), ("chr:100000", (0, 99999, 100000)), ("chr:1:50000-50000", (1, 49999, 50000)),
])
def test_region_forms(colon, region, want):
    assert _tool_query(colon, region)[0] == want


@pytest.mark.parametrize("region,msg", [
    ("nochr", "unknown reference name 'nochr'"), ("nochr:5-10", "unknown reference name 'nochr'"),
    ("chr:0-5", "malformed region"), ("chr:a-b", "malformed region"), ("chr:", "malformed region"), ("chr:5-", "malformed region"),
    ("chr:-5", "malformed region"), ("chr:5-1x", "malformed region"), ("chr:10-5", "BEG > END"), ("", "malformed region"),
])
def test_region_refusals(colon, region, msg):
    r = rf.tool("query", colon.path, region)
    assert r.returncode == 1 and msg in r.stderr and r.stdout == "", (r.stdout, r.stderr)


# ---- the index file ---------------------------------------------------------------------------------------------------------------------
def test_index_discovery_order(colon, tmp_path):
    bam = str(tmp_path / "x.bam")
    shutil.copy(colon.path, bam)
    r = rf.tool("query", bam, "chr")
    assert r.returncode == 1 and "no index found" in r.stderr
    for p in (bam + ".csi", bam + ".bai", str(tmp_path / "x.bai")):   # the message names the paths tried
        assert p in r.stderr
    junk = b"not an index at all"
    for p in (str(tmp_path / "x.bai"), bam + ".bai", bam + ".csi"):   # the later a path is tried, the earlier it is made: each wins in turn
        others = [q for q in (str(tmp_path / "x.bai"), bam + ".bai", bam + ".csi") if os.path.exists(q)]
        for q in others:
            open(q, "wb").write(junk)
        shutil.copy(colon.indexes["csi" if p.endswith(".csi") else "bai"], p)
        assert _tool_query(colon.__class__(bam, kinds=()), "chr:1-1000")[1], p
        assert api.index_query(bam, 0, 0, 1000)
    open(bam + ".csi", "wb").write(junk)                              # the first that EXISTS is taken, good or not
    r = rf.tool("query", bam, "chr")
    assert r.returncode == 1 and "x.bam.csi" in r.stderr and "magic" in r.stderr
    other = str(tmp_path / "elsewhere.idx")                           # --index-file / the INDEX argument
    shutil.copy(colon.indexes["csi"], other)
    assert _tool_query(colon.__class__(bam, kinds=()), "chr:1-1000", other)[1]
    r = rf.tool("query", bam, "chr", str(tmp_path / "missing.idx"))
    assert r.returncode == 1 and "missing.idx" in r.stderr


def test_wrong_and_damaged_indexes(colon, tmp_path):
    syn = rf.Fixture(rf.write_syn(str(tmp_path / "three.bam"), br.SYN_NAMES, br.SYN_LENS, br.synthetic_records()[:50], 0))
    for kind in ("bai", "csi"):
        r = rf.tool("query", colon.path, "chr", syn.indexes[kind])   # three references against the header's two
        assert r.returncode == 1 and "3 references" in r.stderr and "has 2" in r.stderr, r.stderr
        with pytest.raises(RuntimeError, match="3 references"):
            api.index_query(colon.path, 0, 0, 10, syn.indexes[kind])
        whole = open(colon.indexes[kind], "rb").read()
        for cut in (len(whole) // 2, len(whole) - 9, 6):
            bad = str(tmp_path / ("cut.%s" % kind))
            open(bad, "wb").write(whole[:cut])
            r = rf.tool("query", colon.path, "chr", bad)
            assert r.returncode == 1 and ("truncated" in r.stderr or "magic" in r.stderr), (kind, cut, r.stderr)
            with pytest.raises(RuntimeError):
                api.index_query(colon.path, 0, 0, 10, bad)


def test_chunk_outside_the_file(syn, tmp_path):
    """the index of the whole file beside the file cut short: a chunk that points behind its end is refused"""
    fx = syn[1]
    half = str(tmp_path / "half.bam")
    cut = sorted(fx.msize)[len(fx.msize) // 2]
    open(half, "wb").write(fx.data[:cut] + cr.EOF_MEMBER)             # (syn[1]: every member begins with a record)
    r = rf.tool("query", half, "chrA", fx.indexes["bai"])
    assert r.returncode == 1 and "outside" in r.stderr, r.stderr


def test_abi_versions_unchanged():
    from tiebrush_amd import _lib
    assert _lib.load_host().tbh_abi_version() == 1 and "tbh_index_query" in _lib.HOST_SYMBOLS
