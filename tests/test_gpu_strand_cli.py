"""`tiecov --strand-cov PREFIX` / `tiebrush --strand-cov PREFIX`.  The definition is an identity: each of the three files
is byte for byte the file `tiecov -c` writes, with the same further options, from a BAM that holds only that strand's mapped records
under the same header.  The test writes those three BAMs itself (bamio) and runs `tiecov -c` on them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import region_fixtures as rf
import strand_model as stm
import tbi_reader as tr
from bigwig_reader import BigWig
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIECOV = os.path.join(ROOT, "tiebrush_amd", "_build", "tiecov")
TIEBRUSH = os.path.join(ROOT, "tiebrush_amd", "_build", "tiebrush")
T_RUN = 120
CLASSES = stm.CLASSES
COUNTS = {"t1": (2504, 58, 917), "t12": (4405, 4169, 917), "t2": (4010, 4169, 0)}
PATHS = {"t1": "t1/t1.bam", "t12": "t12.bam", "t2": "t2/t2.bam"}


def _run(exe, args, env=None, ok=True, cwd=None):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})), cwd=cwd)
    assert (r.returncode == 0) == ok, (args, r.returncode, r.stderr[-2000:])
    return r


def _tiecov(args, **kw):
    return _run(TIECOV, args, **kw)


def _read(p):
    with open(p, "rb") as f:
        return f.read()


class Split:
    """a golden, its three filtered BAMs (the records of one class under the same header) and the model's parts"""

    def __init__(self, d, name):
        from tiebrush_amd import bamio, soa
        self.name, self.whole = name, rf.golden_copy(d, PATHS[name])
        b = bamio.read_bam(self.whole, keep_names=False)
        self.names = b.header.ref_names
        cin = soa.cov_input_from_bam(b)
        assert not (cin.flag & 4).any()
        cls = np.array([stm.classify(int(s)) for s in cin.strand])
        self.parts = stm.split(cin)
        self.bams = []
        for s in range(3):
            recs = []
            for i in np.flatnonzero(cls == s):
                o = int(b.rec_off[i])
                recs.append(bytes(b.raw[o:o + 4 + struct.unpack_from("<I", b.raw, o)[0]]))
            assert len(recs) == COUNTS[name][s] == self.parts[s].n_records
            p = os.path.join(str(d), "%s.%s.bam" % (name, CLASSES[s]))
            bamio.write_bam(p, b.header.text, b.header.ref_names, b.header.ref_lens, b"".join(recs), level=6)
            self.bams.append(p)


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand_cli")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Split(d, name)
        return cache[name]
    return get


def _strand_files(pre, ext=".bedgraph"):
    return [pre + "." + c + ext for c in CLASSES]


@pytest.mark.parametrize("name", sorted(PATHS))
def test_three_files_are_the_filtered_runs(tmp_path, splits, name):
    from oracle import oracle_ffi as orc
    sp = splits(name)
    pre = str(tmp_path / "s")
    r = _tiecov(["--strand-cov", pre, sp.whole], env={"TBK_TIMING": "1"})
    got = [_read(p) for p in _strand_files(pre)]
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in _strand_files(pre))   # the option alone is an output
    for s in range(3):
        f = str(tmp_path / ("f%d" % s))
        _tiecov(["-c", f, sp.bams[s]])
        assert got[s] == _read(f + ".bedgraph"), (name, CLASSES[s])
        rows = orc.coverage(stm.for_oracle(sp.parts[s]), want_junc=False) if sp.parts[s].n_records else dict(iv_tid=[], iv_start=[], iv_end=[], iv_val=[])
        assert got[s] == stm.cov_text(rows, sp.names), (name, CLASSES[s], "model")
    if name == "t2":
        assert got[2] == stm.HEADER                                    # an empty class: the header line alone
    counts = "%d+ %d- %d. records" % COUNTS[name]
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("strand phase ms:")]
    assert len(line) == 1 and line[0].startswith("strand phase ms: device | " + counts + " | "), r.stderr
    pre2 = str(tmp_path / "h")
    r = _tiecov(["--strand-cov", pre2, sp.whole], env={"TBK_TIMING": "1", "TBK_SPLIT_HOST": "1"})
    assert [_read(p) for p in _strand_files(pre2)] == got
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("strand phase ms:")]
    assert len(line) == 1 and line[0].startswith("strand phase ms: host | " + counts + " | "), r.stderr


def test_beside_the_other_outputs(tmp_path, splits):
    sp = splits("t1")
    bed = str(tmp_path / "f.bed")
    lines = _tiecov(["-c", "-", sp.whole]).stdout.splitlines()[1:]
    with open(bed, "w") as f:
        for k, ln in enumerate(lines[::max(1, len(lines) // 20)][:20]):
            c = ln.split("\t")
            f.write("%s\t%d\t%d\tf%d\t0\t%s\n" % (c[0], max(0, int(c[1]) - 50), int(c[2]) + 400, k, "+-."[k % 3]))
    outs = {}
    for tag, extra in (("a", []), ("b", ["--strand-cov", str(tmp_path / "b.strand")])):
        pre = str(tmp_path / tag)
        _tiecov(["-c", pre + ".c", "-j", pre + ".j", "-s", pre + ".s", "--features", bed, "--summary", pre + ".tsv"] + extra + [sp.whole])
        outs[tag] = [_read(pre + e) for e in (".c.bedgraph", ".j.bed", ".s.bedgraph", ".tsv")]
    assert outs["a"] == outs["b"] and all(len(x) > 100 for x in outs["a"])
    alone = str(tmp_path / "alone")
    _tiecov(["--strand-cov", alone, sp.whole])
    assert [_read(p) for p in _strand_files(str(tmp_path / "b.strand"))] == [_read(p) for p in _strand_files(alone)]


def test_bigwig(tmp_path, splits):
    sp = splits("t1")
    pre, dev = str(tmp_path / "w"), str(tmp_path / "d")
    _tiecov(["-W", "--strand-cov", pre, sp.whole])
    _tiecov(["-W", "--bigwig-writer", "device", "--strand-cov", dev, sp.whole])
    for s in range(3):
        f = str(tmp_path / ("f%d" % s))
        _tiecov(["-W", "-c", f, sp.bams[s]])
        assert _read(pre + "." + CLASSES[s] + ".bigwig") == _read(f + ".bigwig"), CLASSES[s]
        wa, wb = BigWig(f + ".bigwig"), BigWig(dev + "." + CLASSES[s] + ".bigwig")
        assert wa.intervals() == wb.intervals() and len(wa.intervals()) > 10
        assert wa.summary == wb.summary and wa.n_zoom == wb.n_zoom
        for z in range(wa.n_zoom):
            assert wa.zoom(z) == wb.zoom(z), (CLASSES[s], z)


def test_tabix(tmp_path, splits):
    sp = splits("t1")
    plain, gz = str(tmp_path / "p"), str(tmp_path / "z")
    _tiecov(["--strand-cov", plain, sp.whole])
    _tiecov(["--tabix", "--strand-cov", gz, sp.whole])
    for c in CLASSES:
        z, ix, text = _read("%s.%s.bedgraph.gz" % (gz, c)), _read("%s.%s.bedgraph.gz.tbi" % (gz, c)), _read("%s.%s.bedgraph" % (plain, c))
        assert tr.inflate(z) == text
        tr.check_file(z, ix, text, seed=7, n_random=30)
        ln = text.splitlines(keepends=True)[len(text.splitlines()) // 2].split(b"\t")
        hit = tr.query(z, ix, ln[0], int(ln[1]), int(ln[2]))
        assert b"\t".join(ln) in hit


def _indexed(sp, d):
    """indexed copies, as the region tests build them: the whole file and the three filtered ones"""
    out = []
    for p in [sp.whole] + sp.bams:
        q = os.path.join(str(d), "ix." + os.path.basename(p))
        with open(q, "wb") as f:
            f.write(_read(p))
        rf.index(q, "bai")
        out.append(q)
    return out[0], out[1:]


def test_region_and_regions_file(tmp_path, splits):
    sp = splits("t1")
    whole, parts = _indexed(sp, tmp_path)
    rows = [ln.split("\t") for ln in _tiecov(["-c", "-", sp.whole]).stdout.splitlines()[1:]]
    a, b = rows[len(rows) // 3], rows[2 * len(rows) // 3]
    region = "%s:%d-%d" % (a[0], max(1, int(a[1]) - 3000), int(a[2]) + 5000)
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:
        f.write("%s\t%d\t%d\n%s\t%d\t%d\n" % (a[0], max(0, int(a[1]) - 2000), int(a[2]) + 2500, b[0], int(b[1]) + 3, int(b[2]) + 4000))
    for tag, opt in (("r", ["-r", region]), ("R", ["-R", bed])):
        pre = str(tmp_path / tag)
        _tiecov(opt + ["--strand-cov", pre, whole])
        n_rows = 0
        for s in range(3):
            f = str(tmp_path / ("%s%d" % (tag, s)))
            _tiecov(opt + ["-c", f, parts[s]])
            assert _read(pre + "." + CLASSES[s] + ".bedgraph") == _read(f + ".bedgraph"), (tag, CLASSES[s])
            n_rows += _read(f + ".bedgraph").count(b"\n") - 1
        assert n_rows > 3, tag


def test_stream_gives_the_same_bytes(tmp_path, splits):
    sp = splits("t1")
    whole, cut = str(tmp_path / "w"), str(tmp_path / "c")
    _tiecov(["--strand-cov", whole, "-c", whole, sp.whole])
    r = _tiecov(["--stream", "--tile-bytes", "1", "--strand-cov", cut, "-c", cut, sp.whole], env={"TBK_TIMING": "1"})
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("tiecov --stream phases ms:")]
    assert len(line) == 1 and int(line[0].split("(")[1].split()[0]) >= 2           # several tiles were written
    for p, q in zip(_strand_files(whole) + [whole + ".bedgraph"], _strand_files(cut) + [cut + ".bedgraph"]):
        assert _read(p) == _read(q), p
    z = str(tmp_path / "z")
    _tiecov(["--stream", "--tile-bytes", "1", "--tabix", "--strand-cov", z, sp.whole])
    for c, p in zip(CLASSES, _strand_files(whole)):
        assert tr.inflate(_read("%s.%s.bedgraph.gz" % (z, c))) == _read(p), c
        tr.check_file(_read("%s.%s.bedgraph.gz" % (z, c)), _read("%s.%s.bedgraph.gz.tbi" % (z, c)), _read(p), seed=3, n_random=20)


def test_tiebrush(tmp_path):
    ins = sample_paths("t2")
    o, pre = str(tmp_path / "o.bam"), str(tmp_path / "tb")
    _run(TIEBRUSH, ["-o", o, "--strand-cov", pre] + ins)
    want = str(tmp_path / "tc")
    _tiecov(["--strand-cov", want, o])
    texts = [_read(p) for p in _strand_files(want)]
    assert [_read(p) for p in _strand_files(pre)] == texts and sum(len(t) for t in texts) > 1000
    o2, pre2 = str(tmp_path / "o2.bam"), str(tmp_path / "tb2")
    _run(TIEBRUSH, ["-o", o2, "--strand-cov", pre2, "--cov", pre2, "--junc", pre2, "--tabix"] + ins)
    for c, t in zip(CLASSES, texts):                                    # (the same inputs: the same output records, so the same tracks)
        assert tr.inflate(_read("%s.%s.bedgraph.gz" % (pre2, c))) == t, c
        tr.check_file(_read("%s.%s.bedgraph.gz" % (pre2, c)), _read("%s.%s.bedgraph.gz.tbi" % (pre2, c)), t, seed=2, n_random=20)
    plain = str(tmp_path / "plain")
    _tiecov(["-c", plain, "-j", plain, o])
    assert tr.inflate(_read(pre2 + ".bedgraph.gz")) == _read(plain + ".bedgraph") and tr.inflate(_read(pre2 + ".bed.gz")) == _read(plain + ".bed")


def _header_only(d, name="empty.bam"):
    """t1's header without a record, with its index"""
    from tiebrush_amd import bamio
    b = bamio.read_bam(os.path.join(GOLDEN, "t1", "t1.bam"), keep_names=False)
    p = os.path.join(str(d), name)
    bamio.write_bam(p, b.header.text, b.header.ref_names, b.header.ref_lens, b"", level=6)
    rf.index(p, "bai")
    return p


# regions of t1 without a read: a reference that has none (the index names no chunk), and the start of chr12, far before its first read
EMPTY_REGIONS = ("chr1:1-1000", "chr12:1-1000")


def _assert_three_empty(pre, cov_file):
    """the three files of a run without records: what -c wrote for the same input, the header line alone"""
    want = _read(cov_file)
    assert want == stm.HEADER
    assert [_read(p) for p in _strand_files(pre)] == [want] * 3


def test_input_without_records(tmp_path):
    """a header-only BAM: plain, --stream, -r, and beside -W / --tabix; each against `tiecov -c` on the same input"""
    bam = _header_only(tmp_path)
    for tag, extra in (("plain", []), ("stream", ["--stream"]), ("region", ["-r", "chr12:1-1000"])):
        pre = str(tmp_path / tag)
        _tiecov(extra + ["--strand-cov", pre, "-c", pre, bam])
        _assert_three_empty(pre, pre + ".bedgraph")
    pre = str(tmp_path / "host")
    _tiecov(["--strand-cov", pre, "-c", pre, bam], env={"TBK_SPLIT_HOST": "1"})
    _assert_three_empty(pre, pre + ".bedgraph")
    w, f = str(tmp_path / "w"), str(tmp_path / "f")
    _tiecov(["-W", "--strand-cov", w, bam])
    _tiecov(["-W", "-c", f, bam])
    assert [_read(p) for p in _strand_files(w, ".bigwig")] == [_read(f + ".bigwig")] * 3
    z, g = str(tmp_path / "z"), str(tmp_path / "g")
    _tiecov(["--tabix", "--strand-cov", z, bam])
    _tiecov(["--tabix", "-c", g, bam])
    for p in _strand_files(z, ".bedgraph.gz"):
        assert _read(p) == _read(g + ".bedgraph.gz") and _read(p + ".tbi") == _read(g + ".bedgraph.gz.tbi") and tr.inflate(_read(p)) == stm.HEADER


@pytest.mark.parametrize("region", EMPTY_REGIONS)
def test_region_without_reads(tmp_path, splits, region):
    sp = splits("t1")
    whole, _parts = _indexed(sp, tmp_path)
    pre = str(tmp_path / "e")
    _tiecov(["-r", region, "--strand-cov", pre, "-c", pre, "-j", pre, whole])
    _assert_three_empty(pre, pre + ".bedgraph")
    bed = str(tmp_path / "e.bed")
    with open(bed, "w") as f:
        f.write("chr1\t0\t1000\nchr12\t0\t1000\n")
    pre = str(tmp_path / "R")
    _tiecov(["-R", bed, "--strand-cov", pre, "-c", pre, whole])
    _assert_three_empty(pre, pre + ".bedgraph")


def test_tiebrush_region_without_reads(tmp_path):
    ins = []
    for k, p in enumerate(sample_paths("t2")[:3]):
        q = str(tmp_path / ("in%d.bam" % k))
        with open(q, "wb") as f:
            f.write(_read(p))
        rf.index(q, "bai")
        ins.append(q)
    o, pre = str(tmp_path / "o.bam"), str(tmp_path / "tb")
    _run(TIEBRUSH, ["-r", "chr12:1-1000", "-o", o, "--strand-cov", pre, "--cov", pre] + ins)
    from tiebrush_amd import bamio
    assert bamio.read_bam(o, keep_names=False).n == 0
    _assert_three_empty(pre, pre + ".bedgraph")
    f = str(tmp_path / "f")
    _tiecov(["-c", f, o])
    assert _read(f + ".bedgraph") == _read(pre + ".plus.bedgraph")


@pytest.mark.parametrize("extra", [["-r", "chr12"], ["-R", "x.bed"], ["--stream"]])
def test_split_host_with_device_records_is_refused_before_any_file(tmp_path, extra):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    r = _run(TIECOV, extra + ["--strand-cov", "p", "-c", "c", bam], env={"TBK_SPLIT_HOST": "1"}, ok=False, cwd=str(tmp_path))
    assert "TBK_SPLIT_HOST=1 divides host records" in r.stderr and "usage:" not in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("tool,args,phrase", [
    ("tiecov", ["--strand-cov", "-"], "--strand-cov needs a file prefix (not '-')"),
    ("tiecov", ["--strand-cov", "stdout"], "--strand-cov needs a file prefix (not 'stdout')"),
    ("tiecov", ["--strand-cov", "a", "--strand-cov", "b"], "--strand-cov given more than once"),
    ("tiecov", ["--strand-cov=a", "--strand-cov", "b"], "--strand-cov given more than once"),
    ("tiecov", ["--tabix"], "--tabix needs at least one of -c / -j / -s (it applies to their tracks)"),
    ("tiecov", ["-W"], "at least one of -c/-j/-s arguments required!"),
    ("tiebrush", ["--strand-cov", "a", "--ranks", "2"], "--strand-cov and --ranks do not go together"),
    ("tiebrush", ["--strand-cov", "-"], "--strand-cov needs a file prefix (not '-')"),
    ("tiebrush", ["--strand-cov", "a", "--strand-cov", "b"], "--strand-cov given more than once"),
    ("tiebrush", ["--tabix"], "--tabix needs at least one of --cov / --junc / --samp (it applies to their tracks)"),
    ("tiebrush", ["--bigwig"], "--bigwig needs --cov")])
def test_refusals_leave_no_file(tmp_path, tool, args, phrase):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    if tool == "tiecov":
        r = _run(TIECOV, args + [bam], ok=False, cwd=str(tmp_path))
    else:
        r = _run(TIEBRUSH, ["-o", "o.bam"] + args + [bam], ok=False, cwd=str(tmp_path))
    assert phrase in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []
