"""Several regions in one run, the host side alone: the BED reader against the tests' own normalisation, the chunk query
over a table (tbh_index_query_regions, `tbh_tool rquery` / `mrquery`) against a brute-force scan, and the refusals of `tiebrush -R` and
`tiecov -R` that come before the device is brought up.  CPU only.  Every test fails on a build without the feature: the symbols, the
tool's forms and the option do not exist there."""
import os
import subprocess

import pytest

import bai_reader as br
import multi_region as mr
import region_fixtures as rf
from test_tiebrush_region_cpu import N_MANY, inputs  # noqa: F401  (the fixture of `tiebrush -r`'s refusals: the same files serve -R)
from tiebrush_amd import _lib, api

BIN = rf.BIN
W = rf.W


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    d = tmp_path_factory.mktemp("regions_syn")
    return {al: rf.Fixture(rf.write_syn(str(d / ("syn%d.bam" % al)), br.SYN_NAMES, br.SYN_LENS, br.synthetic_records(), al)) for al in (0, 1)}


# ---- the BED reader ----------------------------------------------------------------------------------------------------------------------
MESSY = [(0, 5000, 6000), (2, 100, 200), (0, 100, 300), (0, 250, 400),      # unsorted; two that overlap
         (0, 1000, 9000), (0, 2000, 3000),                                  # nested
         (0, 400, 500), (0, 20000, 20010), (0, 20011, 20020),               # abuts [250, 400): merged; one base apart: not merged
         (2, 900000, 5000000),                                              # an end beyond the reference: cut
         (1, 50, 50), (2, 1000000, 1000005),                                # empty; empty after the cut
         (1, 0, 10)]


def test_bed_reader_against_the_model(syn, tmp_path):
    fx = syn[0]
    want = mr.normalise(MESSY, fx.lens)
    assert mr.is_normalised(want) and (0, 100, 500) in want and (0, 1000, 9000) in want and (0, 20000, 20010) in want and (0, 20011, 20020) in want
    assert (2, 900000, fx.lens[2]) in want and not any(t == 1 and b == 50 for t, b, e in want)
    head = ["# a comment", "track name=x description=\"y z\"", "browser position chrA:1-100", "", "   "]
    variants = [dict(), dict(sep=" "), dict(extra=["name\t0\t+", "x"]), dict(eol="\r\n", head=head), dict(sep=" \t ", head=head, extra=["n 1"])]
    for k, kw in enumerate(variants):
        bed = mr.write_bed(str(tmp_path / ("v%d.bed" % k)), fx.names, MESSY, **kw)
        assert api.regions_from_bed(fx.path, bed) == want, kw
    r = rf.tool("rquery", fx.path, bed, fx.indexes["bai"])                    # the tool prints the same table
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "regions %d" % len(want)
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines[1:1 + len(want)]] == want
    # a table larger than the first buffer the wrapper offers
    many = [(0, 100 * i, 100 * i + 50) for i in range(300)]
    assert api.regions_from_bed(fx.path, mr.write_bed(str(tmp_path / "many.bed"), fx.names, many)) == many


@pytest.mark.parametrize("text,msgs", [
    ("chrA\t5\t10\nchrA\t7\n", ["line 2", "fewer than three fields"]),
    ("chrA\t5\t10\n\nchrA\n", ["line 3", "fewer than three fields"]),
    ("# c\nchrA\tx\t10\n", ["line 2", "start", "not a non-negative integer"]),
    ("chrA\t-5\t10\n", ["line 1", "start", "not a non-negative integer"]),
    ("chrA\t5\t1e3\n", ["line 1", "end", "not a non-negative integer"]),
    ("chrA\t5\t10\nchrA\t5\t\n", ["line 2", "fewer than three fields"]),
    ("track x\nchrA\t5\t10\r\nchrA\t10\t5\r\n", ["line 3", "start > end"]),
    ("chrA\t5\t10\nchrZ\t5\t10\n", ["line 2", "unknown reference name 'chrZ'"]),
    ("", ["no region"]), ("# only\ntrack t\n\n", ["no region"]), ("chrEmpty\t7\t7\nchrOne\t2000000\t2000010\n", ["no region"]),
])
def test_bed_refusals(syn, tmp_path, text, msgs):
    fx = syn[0]
    bed = str(tmp_path / "bad.bed")
    with open(bed, "w", newline="") as fh:
        fh.write(text)
    with pytest.raises(RuntimeError) as e:
        api.regions_from_bed(fx.path, bed)
    r = rf.tool("rquery", fx.path, bed)
    assert r.returncode == 1 and r.stdout == ""
    for m in msgs + ["bad.bed"]:
        assert m in str(e.value) and m in r.stderr, (m, str(e.value), r.stderr)
    with pytest.raises(RuntimeError, match="cannot read"):
        api.regions_from_bed(fx.path, str(tmp_path / "missing.bed"))


# ---- the chunk query over a table --------------------------------------------------------------------------------------------------------
def _check_table(fx, kind, table):
    """the chunks are sorted, byte-disjoint and cut at record starts; their records hold every record that overlaps an interval, none twice"""
    assert mr.is_normalised(table), table
    chunks = api.index_query_regions(fx.path, table, fx.indexes[kind])
    idx = fx.in_chunks(chunks)                                        # (asserts sorted, no two in one member, record starts)
    assert len(idx) == len(set(idx))
    inside = set(idx)
    want = mr.brute(fx.recs, table)
    pos = {r[3]: i for i, r in enumerate(fx.recs)}
    assert all(pos[r[3]] in inside for r in want), (kind, table)
    return chunks, want


@pytest.mark.parametrize("aligned", [0, 1])
@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_query_regions_on_the_synthetic_file(syn, kind, aligned):
    fx = syn[aligned]
    ix = fx.indexes[kind]
    for tid, beg, end in rf.syn_regions():                               # R = 1: tbh_index_query's result, element for element
        assert api.index_query_regions(fx.path, [(tid, beg, end)], ix) == api.index_query(fx.path, tid, beg, end, ix), (tid, beg, end)
    # pair one: two loci in one 16 kb window of the bulk; each one's own query names the same chunks, the table's names them once
    a, b = (0, 30 * W + 1000, 30 * W + 1010), (0, 30 * W + 3000, 30 * W + 3010)
    ca, cb = api.index_query(fx.path, *a, ix), api.index_query(fx.path, *b, ix)
    assert a[1] >> 14 == b[1] >> 14 and ca == cb and len(ca) >= 1 and fx.brute(*a) and fx.brute(*b)
    chunks, want = _check_table(fx, kind, [a, b])
    assert chunks == ca and want == sorted(fx.brute(*a) + fx.brute(*b), key=lambda r: r[3])
    # pair two: loci on two references, the first of which has no record
    assert fx.brute(1, 0, 1000) == [] and api.index_query(fx.path, 1, 0, 1000, ix) == []
    chunks, want = _check_table(fx, kind, [(1, 0, 1000), (2, 5000, 5100)])
    assert chunks == api.index_query(fx.path, 2, 5000, 5100, ix) and len(want) == 1
    for seed in range(20):
        _check_table(fx, kind, mr.random_table(fx, 100 * aligned + seed))
    # the tool, a process: the same chunks, the records in them and the hits by the host codec
    table = mr.random_table(fx, 7)
    bed = mr.write_bed(os.path.join(os.path.dirname(fx.path), "t%s%d.bed" % (kind, aligned)), fx.names, table)
    r = rf.tool("rquery", fx.path, bed, ix)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    tchunks = [tuple(int(x, 16) for x in l.split()) for l in lines if l and not l.startswith(("region", "records", "overlapping", "hit"))]
    chunks, want = _check_table(fx, kind, table)
    assert tchunks == chunks
    assert [int(l.split()[1], 16) for l in lines if l.startswith("hit ")] == [r[3] for r in want]
    assert int([l for l in lines if l.startswith("records ")][0].split()[1]) == len(fx.in_chunks(chunks))


@pytest.mark.parametrize("name", ["t1/t1.bam", "t2/t2.bam", "t12.bam", "t1/t1s0.bam"])
def test_query_regions_on_the_goldens(tmp_path, name):
    fx = rf.Fixture(rf.golden_copy(tmp_path, name))
    for kind in ("bai", "csi"):
        for tid, beg, end in rf.random_regions(fx, 5, 10):
            assert api.index_query_regions(fx.path, [(tid, beg, end)], fx.indexes[kind]) == api.index_query(fx.path, tid, beg, end, fx.indexes[kind])
        for seed in range(20):
            _check_table(fx, kind, mr.random_table(fx, seed))


def test_query_regions_refuses_a_table_that_is_not_normalised(syn):
    fx = syn[0]
    for bad in ([(0, 100, 200), (0, 200, 300)], [(0, 100, 200), (0, 150, 300)], [(0, 500, 600), (0, 100, 200)], [(2, 0, 10), (0, 0, 10)],
                [(0, 100, 200), (0, 300, 300)], [(0, 100, 200), (3, 0, 10)], [(0, -5, 10), (0, 20, 30)]):
        with pytest.raises(RuntimeError):
            api.index_query_regions(fx.path, bad, fx.indexes["bai"])
    with pytest.raises(RuntimeError):
        api.index_query_regions(fx.path, [], fx.indexes["bai"])


def test_mrquery(syn, tmp_path):
    """the plumbing of `tiebrush -R` on the host: every input's merged chunks read on threads, the records and hits per file"""
    table = mr.random_table(syn[0], 3)
    bed = mr.write_bed(str(tmp_path / "m.bed"), syn[0].names, table)
    r = rf.tool("mrquery", bed, 3, syn[0].path, syn[1].path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "regions %d" % len(table)
    for f, fx in enumerate((syn[0], syn[1])):
        chunks = api.index_query_regions(fx.path, table)
        ln = [l for l in lines if l.startswith("file %d " % f)][0].split()
        assert (int(ln[3]), int(ln[5]), int(ln[7])) == (len(chunks), len(fx.in_chunks(chunks)), len(mr.brute(fx.recs, table)))


# ---- the command lines: refusals before the device -----------------------------------------------------------------------------------
def _run(tool, args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, stdin=subprocess.DEVNULL)


def _bed(path, text):
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_tiebrush_refusals_come_before_anything_exists(inputs, tmp_path):  # noqa: F811
    a, b = inputs["a"].path, inputs["b"].path
    good = _bed(str(tmp_path / "good.bed"), "chr12\t5\t10\nchr12\t98595000\t98596000\n")
    whole = _bed(str(tmp_path / "whole.bed"), "chr12\t98000001\t400000000\nchr12\t0\t98000000\n")   # (two intervals: all of chr12 but one base)
    cases = [
        (["-R", good, "-r", "chr12:5-10", a, b], ["do not go together"]),
        (["--regions-file", good, "--region=chr12:5-10", a, b], ["do not go together"]),
        (["-R", good, "-R", good, a, b], ["-R / --regions-file given more than once"]),
        (["-R", good, "--regions-file=" + good, a, b], ["more than once"]),
        (["--regions-file", good, "-AR", good, a, b], ["more than once"]),
        (["-R", good, "--ranks", "2", a, b], ["--ranks"]),
        (["-R", _bed(str(tmp_path / "short.bed"), "chr12\t5\t10\nchr12\t7\n"), a, b], ["short.bed line 2", "fewer than three fields"]),
        (["-R", _bed(str(tmp_path / "neg.bed"), "chr12\t10\t5\n"), a, b], ["neg.bed line 1", "start > end"]),
        (["-R", _bed(str(tmp_path / "unk.bed"), "chr12\t5\t10\nchrZ\t1\t2\n"), a, b], ["unk.bed line 2", "unknown reference name 'chrZ'"]),
        (["-R", _bed(str(tmp_path / "none.bed"), "# nothing\n"), a, b], ["none.bed", "no region"]),
        (["-R", str(tmp_path / "missing.bed"), a, b], ["cannot read", "missing.bed"]),
        (["-R", good, a, inputs["bare"], b], ["no index found", inputs["bare"] + ".csi", inputs["bare"] + ".bai"]),
        (["-R", good, a, inputs["sam"]], ["not a BGZF", inputs["sam"]]),
        (["-R", good, a, "-"], ["standard input"]),
        (["-R", whole, b, inputs["half"]], ["outside", inputs["half"]]),                     # a chunk that points outside its file
        (["-R", good, inputs["many_a"], inputs["many_b"]], ["2 inputs name %d chunks" % N_MANY, "2 regions", "takes 65535", inputs["many_a"]]),
    ]
    out = tmp_path / "out"
    out.mkdir()
    pre = str(out / "t")
    for k, (args, msgs) in enumerate(cases):
        extra = [["--index"], ["--csi"], ["--cov", pre + ".c", "--junc", pre + ".j"], ["--writer", "host", "--cov", pre, "--bigwig"]][k % 4]
        r = _run("tiebrush", ["-o", str(out / "o.bam")] + extra + args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        for m in msgs:
            assert m in r.stderr, (args, m, r.stderr)
        assert "libtbk" not in r.stderr and "GPU" not in r.stderr, (args, r.stderr)      # (the device was never asked for)
        assert os.listdir(str(out)) == [], (args, os.listdir(str(out)))
    r = _run("tiebrush", ["-h"])
    assert r.returncode == 0 and "-R,--regions-file FILE" in r.stdout and "-r,--region REGION" in r.stdout


def test_tiecov_refusals_come_before_anything_exists(inputs, tmp_path):  # noqa: F811
    a, ix = inputs["a"].path, inputs["a"].indexes["bai"]
    good = _bed(str(tmp_path / "good.bed"), "chr12\t5\t10\n")
    out = tmp_path / "out"
    out.mkdir()
    pre = str(out / "x")
    cases = [
        (["-R", good, "-r", "chr12:5-10", "--index-file", ix, a], ["do not go together"]),
        (["-R", good, "-R", good, a], ["-R / --regions-file given more than once"]),
        (["--regions-file", good, "-WR", good, a], ["more than once"]),
        (["-R", good, "--regions-file=" + good, a], ["more than once"]),
        (["-R", _bed(str(tmp_path / "short.bed"), "chr12 5 10\nchr12 7\n"), a], ["short.bed line 2", "fewer than three fields"]),
        (["-R", _bed(str(tmp_path / "unk.bed"), "chrZ\t1\t2\n"), a], ["unk.bed line 1", "unknown reference name 'chrZ'"]),
        (["-R", _bed(str(tmp_path / "none.bed"), "\n"), a], ["no region"]),
        (["-R", str(tmp_path / "missing.bed"), a], ["cannot read"]),
        (["-R", good, inputs["bare"]], ["no index found"]),
        (["-R", good, "--index-file", str(tmp_path / "missing.idx"), a], ["missing.idx"]),
    ]
    for args, msgs in cases:
        r = _run("tiecov", ["-c", pre, "-j", pre] + args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        for m in msgs:
            assert m in r.stderr, (args, m, r.stderr)
        assert "cannot use GPU" not in r.stderr and os.listdir(str(out)) == [], (args, r.stderr, os.listdir(str(out)))
    r = _run("tiecov", ["-s", pre, "-R", good, "--index-file", ix, a])                        # (t1s0: no sample lines in its header)
    assert r.returncode == 1 and "no sample lines" in r.stderr and os.listdir(str(out)) == []
    r = _run("tiecov", ["-h"])
    assert "-R,--regions-file FILE" in r.stderr + r.stdout


def test_abi_versions_and_symbols():
    H = _lib.load_host()
    assert H.tbh_abi_version() == 1
    for s in ("tbh_regions_from_bed", "tbh_index_query_regions"):
        assert s in _lib.HOST_SYMBOLS and getattr(H, s)
    L = _lib.load()                                                     # (loads without a GPU: only tbk_create needs one)
    assert L.tbk_abi_version() == 9
    for s in ("tbk_regions_view", "tbk_cov_clip_regions", "tbk_sample_clip_regions", "tbk_tile_regions"):
        assert s in _lib.SYMBOLS and getattr(L, s)
