"""`tiecov --stream`: the whole file in batches of BGZF members, decoded and cut at bundle heads on the device.  The
contract is an identity with the run without the option: every track file byte for byte, at batch sizes of one member, 64 KiB and 1 MiB,
on inputs with many bundles (real cuts), with two bundles (the carry grows over many batches) and with one (everything is carried until
the end); the bigWig of -W with the same intervals and zoom summaries; what is refused, and that a failed run leaves no file."""
import os
import subprocess

import pytest

import bam_craft as bc
import tbi_reader as tr
from bigwig_reader import BigWig
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIECOV = os.path.join(ROOT, "tiebrush_amd", "_build", "tiecov")
T_RUN = 120
SIZES = ("1", "65536", "1M")
EXTS = (".coverage.bedgraph", ".junctions.bed", ".sample.bedgraph")


def _tiecov(args, env=None, ok=True):
    r = subprocess.run([TIECOV] + args, capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})))
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _tracks(d, tag, bam, extra, sample=True, env=None):
    pre = str(d / tag)
    args = ["-c", pre + ".coverage", "-j", pre + ".junctions"] + (["-s", pre + ".sample"] if sample else [])
    r = _tiecov(extra + args + [bam], env)
    return {e: _read(pre + e) for e in EXTS if sample or e != ".sample.bedgraph"}, r


def _tracks_gz(d, tag, bam, extra, sample=True):
    """a --tabix run: {ext: (.gz bytes, index bytes)}"""
    pre = str(d / tag)
    args = ["-c", pre + ".coverage", "-j", pre + ".junctions"] + (["-s", pre + ".sample"] if sample else [])
    r = _tiecov(extra + args + [bam])
    return {e: (_read(pre + e + ".gz"), _read(pre + e + ".gz.tbi")) for e in EXTS if sample or e != ".sample.bedgraph"}, r


def _assert_golden(got, g):
    """the streamed tracks against the reference's own files, as tests/test_gpu_cli.py holds the unstreamed ones: the reference prints a
    whole value without decimals where this writer prints .000, and the sample track's heat with another rounding (first four columns)"""
    def norm(blob, col):
        out = []
        for ln in blob.decode().splitlines():
            f = ln.split("\t")
            if len(f) > col:
                assert f[col].endswith(".000"), ln
                f[col] = f[col][:-4]
            out.append("\t".join(f))
        return out
    gold = lambda e: _read(g + e).decode().splitlines()
    assert norm(got[".coverage.bedgraph"], 3) == gold(".coverage.bedgraph")
    assert norm(got[".junctions.bed"], 4) == gold(".junctions.bed")
    ours, theirs = got[".sample.bedgraph"].decode().splitlines(), gold(".sample.bedgraph")
    assert ours[0] == theirs[0] and [ln.split("\t")[:4] for ln in ours[1:]] == [ln.split("\t")[:4] for ln in theirs[1:]]


@pytest.mark.parametrize("name", ["t1/t1.bam", "t2/t2.bam", "t12.bam", "t1/t1s0.bam", "t2/t2s0.bam"])
def test_streamed_tracks_are_the_unstreamed_bytes(tmp_path, name):
    bam = os.path.join(GOLDEN, name)
    sample = name in ("t1/t1.bam", "t2/t2.bam", "t12.bam")            # (the plain inputs have no @CO SAMPLE lines: -s is refused for them)
    want, _ = _tracks(tmp_path, "whole", bam, [], sample)
    if name in ("t1/t1.bam", "t2/t2.bam"):
        _assert_golden(_tracks(tmp_path, "g", bam, ["--stream", "--tile-bytes", "1"], sample)[0], os.path.join(GOLDEN, name[:2], name[:2]))
    tiles = []
    for n in SIZES:
        got, r = _tracks(tmp_path, "s" + n, bam, ["--stream", "--tile-bytes", n], sample, env={"TBK_TIMING": "1"})
        for e in want:
            assert got[e] == want[e], (name, n, e)
        line = [ln for ln in r.stderr.splitlines() if ln.startswith("tiecov --stream phases ms:")]
        assert len(line) == 1
        tiles.append((int(line[0].split(" batches")[0].split()[-1]), int(line[0].split("(")[1].split()[0])))
    assert tiles[0][0] > tiles[2][0] >= 1                             # a member a batch: many batches; 1 MiB: the file in one or two
    if name == "t1/t1.bam":
        assert tiles[0][1] >= 2                                       # many bundles: the stream really is cut and written in pieces
    if name == "t1/t1s0.bam":
        assert tiles[0][0] > 100 and tiles[0][1] <= 3                 # few bundles: nearly everything waits in the carry for the end


def test_tile_bytes_alone_implies_stream_and_stdout_works(tmp_path):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    want = _tiecov(["-c", "-", bam]).stdout
    r = _tiecov(["--tile-bytes", "4K", "-c", "stdout", bam], env={"TBK_TIMING": "1"})
    assert r.stdout == want and "tiecov --stream phases ms:" in r.stderr


def test_bigwig_has_the_same_intervals_and_zooms(tmp_path):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tiecov(["-W", "-c", a, bam])
    _tiecov(["--stream", "--tile-bytes", "1", "-W", "-c", b, "-j", b, bam])
    wa, wb = BigWig(a + ".bigwig"), BigWig(b + ".bigwig")
    assert wa.intervals() == wb.intervals() and len(wa.intervals()) > 100
    assert wa.summary == wb.summary and wa.n_zoom == wb.n_zoom
    for z in range(wa.n_zoom):
        assert wa.zoom(z) == wb.zoom(z), z
    assert _read(a + ".bigwig") == _read(b + ".bigwig")              # (the host writer saw the same rows in the same order)


@pytest.mark.parametrize("name,sample", [("t1/t1.bam", True), ("t2/t2.bam", True), ("t1/t1s0.bam", False)])
def test_tabix_tracks_tile_by_tile(tmp_path, name, sample):
    """--tabix under --stream, a member a batch (t1: several tiles, every track in several pieces; t1s0: one tile at the end): every .gz
    inflates to the plain track of the run without either option, its index is the restatement of its own bytes and answers seeded region
    queries like a linear filter (tbi_reader.check_file), and a handful of regions give the lines the unstreamed .gz gives"""
    bam = os.path.join(GOLDEN, name)
    plain, _ = _tracks(tmp_path, "plain", bam, [], sample)
    whole, _ = _tracks_gz(tmp_path, "whole", bam, ["--tabix"], sample)
    for n in ("1", "1M"):
        got, r = _tracks_gz(tmp_path, "s" + n, bam, ["--stream", "--tile-bytes", n, "--tabix"], sample)
        for e in plain:
            gz, ix = got[e]
            tr.check_file(gz, ix, plain[e], seed=5, n_random=40)
            wgz, wix = whole[e]
            lines = tr.inflate(gz).splitlines(keepends=True)[1:]
            picks = [lines[0], lines[len(lines) // 3], lines[len(lines) // 2], lines[-1]] if lines else []
            for ln in picks:
                f = ln.split(b"\t")
                for beg, end in ((int(f[1]), int(f[2])), (max(0, int(f[1]) - 5000), int(f[2]) + 5000)):
                    hit = tr.query(gz, ix, f[0], beg, end)
                    assert hit == tr.query(wgz, wix, f[0], beg, end) and ln in hit, (name, n, e, f[0], beg, end)


def test_tabix_with_bigwig_and_stdout_rules(tmp_path):
    """-W keeps the coverage a bigWig beside the tabix junctions; --tabix with -c - stays refused"""
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _tiecov(["--tabix", "-W", "-c", a, "-j", a, bam])
    _tiecov(["--stream", "--tile-bytes", "1", "--tabix", "-W", "-c", b, "-j", b, bam])
    assert _read(a + ".bigwig") == _read(b + ".bigwig")
    assert tr.inflate(_read(b + ".bed.gz")) == tr.inflate(_read(a + ".bed.gz"))
    tr.check_file(_read(b + ".bed.gz"), _read(b + ".bed.gz.tbi"), tr.inflate(_read(a + ".bed.gz")), seed=3, n_random=30)
    r = _tiecov(["--stream", "--tabix", "-c", "-", bam], ok=False)
    assert "--tabix needs a coverage file" in r.stderr


def test_crafted_file_with_straddling_records_and_unmapped_reads(tmp_path):
    """records that straddle one and two members, unmapped reads between them, several bundles on two references"""
    recs = []
    for i in range(400):
        tid, pos = (0, 100 + 37 * i) if i < 250 else (1, 50 + 900 * (i - 250))
        cigar = ((30 + i % 40, bc.M),) if i % 3 else ((20, bc.M), (500 + i, bc.N), (25, bc.M))
        aux = bc.tag("YC", "f", float(1 + i % 4)) + (bc.tag("XS", "A", "+") if i % 3 == 0 else b"")
        recs.append(bc.Rec(tid=tid, pos=pos, cigar=cigar, name=b"r%d" % i, l_seq=20 + (i % 7) * 30, aux=aux))
        if i % 11 == 5:
            recs.append(bc.Rec(tid=tid, pos=pos, flag=4, cigar=(), name=b"u%d" % i, l_seq=50))
    p = bc.payload(recs)
    path = str(tmp_path / "crafted.bam")
    with open(path, "wb") as f:
        f.write(bc.frame(p, list(range(90, len(p), 90))))
    lay = bc.layout(_read(path))
    assert len(lay.inside()) > 100 and max(len(r.raw) for r in recs) > 2 * 90
    want, _ = _tracks(tmp_path, "whole", path, [], sample=False)
    assert want[".coverage.bedgraph"].count(b"\n") > 50 and want[".junctions.bed"].count(b"\n") > 20
    for n in ("1", "1000", "1M"):
        got, _ = _tracks(tmp_path, "s" + n, path, ["--stream", "--tile-bytes", n], sample=False)
        assert got == want, n


def test_bundle_too_large_leaves_no_file(tmp_path):
    bam = os.path.join(GOLDEN, "t1", "t1s0.bam")
    pre = str(tmp_path / "big")
    from tiebrush_amd import bamio
    b = bamio.read_bam(bam, keep_names=False)                              # the one bundle begins with the file's first record
    assert not (int(b.flag[0]) & 4)
    where = "%s:%d" % (b.header.ref_names[int(b.tid[0])], int(b.pos[0]) + 1)
    for extra in ([], ["--tile-bytes", "1"], ["--tabix"]):                 # the first batch alone; a carry that grew over the cap; tabix writers open
        r = _tiecov(["--stream", "-c", pre, "-j", pre] + extra + [bam], env={"TBK_DEBUG": "stream_cap=1000"}, ok=False)
        assert "bundle too large for one tile" in r.stderr and where in r.stderr, (extra, where, r.stderr)
        assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("extra,phrase", [
    (["-r", "chr1"], "--stream and -r / -R / --index-file do not go together (a region run reads only the region's chunks)"),
    (["-R", "x.bed"], "--stream and -r / -R / --index-file do not go together (a region run reads only the region's chunks)"),
    (["--index-file", "x.bai"], "--stream and -r / -R / --index-file do not go together (a region run reads only the region's chunks)"),
    (["--features", "x.bed", "--summary", "x.tsv"], "--stream and --features / --summary do not go together (a feature across two tiles needs a carried partial sum)"),
    (["-W", "--bigwig-writer", "device"], "--stream and --bigwig-writer device do not go together (the device writer takes all rows at once)")])
def test_refused_combinations(tmp_path, extra, phrase):
    """the refusal's own sentence, not the usage text (which names every option and would satisfy a search for the words)"""
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    pre = str(tmp_path / "o")
    for opt in (["--stream"], ["--tile-bytes", "1M"]):
        r = _tiecov(opt + ["-c", pre, "-j", pre] + extra + [bam], ok=False)
        assert phrase in r.stderr and "usage:" not in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_sam_text_and_bad_sizes_are_refused(tmp_path):
    sam = str(tmp_path / "in.sam")
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\nr1\t0\tchr1\t10\t60\t20M\t*\t0\t0\t*\t*\n")
    pre = str(tmp_path / "o")
    r = _tiecov(["--stream", "-c", pre, sam], ok=False)
    assert "--stream needs a BAM file (BGZF); %s is SAM text" % sam in r.stderr and "usage:" not in r.stderr
    r = _tiecov(["--tile-bytes", "12Q", "-c", pre, os.path.join(GOLDEN, "t1", "t1.bam")], ok=False)
    assert "--tile-bytes takes a size in bytes, or with a K / M / G suffix (got '12Q')" in r.stderr and "usage:" not in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["in.sam"]
