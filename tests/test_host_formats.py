"""Input / output formats of the host side beyond BAM + bedGraph: SAM text input (host/sam.cpp) and the
bigWig writer behind `tiecov -W` (host/bigwig.cpp).  CPU only: the GPU command lines are exercised in test_gpu_cli.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from bigwig_reader import BigWig
from helpers import GOLDEN, read_lines
from samtext import _aux_text, bam_to_sam_text
from tiebrush_amd import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("TBK_TEST_TBH_TOOL") or os.path.join(ROOT, "tiebrush_amd", "_build", "tbh_tool")   # (the override: the sanitizer builds of tools/san_check.sh)


def _records(path):
    raw = bamio.bgzf_decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, p)[0]
        refs.append((raw[p + 4:p + 4 + ln - 1], struct.unpack_from("<i", raw, p + 4 + ln)[0])); p += 4 + ln + 4
    out = []
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        out.append(raw[p + 4:p + 4 + bs]); p += 4 + bs
    return text, refs, out


def _fixed_and_aux(r):
    l_rn, n_cig, l_seq = r[8], struct.unpack_from("<H", r, 12)[0], struct.unpack_from("<i", r, 16)[0]
    a = 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return r[:a], _aux_text(r, a, len(r))


@pytest.mark.parametrize("name", ["t1/t1s0.bam", "t2/t2.bam", "t12.bam"])
def test_sam_text_input_reproduces_the_bam_records(tmp_path, name):
    """BAM -> SAM text (tests/samtext.py) -> the host reader -> BAM: every record comes back with the same fixed part, bin
    included, and the same tags; where the original was written with the smallest integer types (everything but the tags
    bam_aux_update_int left wider) the bytes are identical."""
    src = os.path.join(GOLDEN, name)
    text, recs = bam_to_sam_text(src)
    sam = tmp_path / "x.sam"
    sam.write_text(text)
    out = tmp_path / "y.bam"
    r = subprocess.run([TOOL, "cat", str(sam), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t0, refs0, _ = _records(src)
    t1, refs1, got = _records(str(out))
    assert refs0 == refs1 and t0.rstrip(b"\0") == t1.rstrip(b"\0")
    assert len(got) == len(recs)
    same = sum(a == b for a, b in zip(recs, got))
    assert same >= len(recs) - 10
    for a, b in zip(recs, got):
        if a != b:
            assert _fixed_and_aux(a) == _fixed_and_aux(b)


def test_sam_text_errors_are_loud(tmp_path):
    good = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\nr1\t0\tc1\t10\t60\t5M\t*\t0\t0\tACGTA\tIIIII\tNH:i:1\tXS:A:+\tZZ:B:s,1,-2\n"
    for i, bad in enumerate([good.replace("c1\t10", "c9\t10"), good.replace("5M", "5Q"), good.replace("NH:i:1", "NH:i:x"),
                             good.replace("IIIII", "III")]):
        p = tmp_path / ("b%d.sam" % i)
        p.write_text(bad)
        r = subprocess.run([TOOL, "cat", str(p), str(tmp_path / "o.bam")], capture_output=True, text=True)
        assert r.returncode != 0 and "line 3" in r.stderr, r.stderr
    p = tmp_path / "g.sam"
    p.write_text(good)
    assert subprocess.run([TOOL, "cat", str(p), str(tmp_path / "o.bam")]).returncode == 0
    b = bamio.read_bam(str(tmp_path / "o.bam"), keep_aux=True)
    assert b.n == 1 and int(b.pos[0]) == 9 and int(b.nh[0]) == 1 and chr(int(b.strand[0])) == "+"
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM\3\0" + b"\0" * 40)
    r = subprocess.run([TOOL, "cat", str(cram), str(tmp_path / "o.bam")], capture_output=True, text=True)
    assert r.returncode != 0 and "CRAM" in r.stderr


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_bigwig_writer_round_trip(tmp_path, name):
    """the golden coverage bedGraph through the bigWig writer and back through an independent reader: the same intervals
    (values as float32, as the reference passes them to libBigWig: tiecov.cpp:258), a chromosome tree with every @SQ, a
    total summary and zoom levels that add up"""
    bed = os.path.join(GOLDEN, name, name + ".coverage.bedgraph")
    bam = os.path.join(GOLDEN, name, name + ".bam")
    out = tmp_path / "c.bigwig"
    r = subprocess.run([TOOL, "bedgraph2bw", bam, bed, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = []
    for ln in read_lines(bed)[1:]:
        c, a, b, v = ln.split("\t")
        want.append((c, int(a), int(b), float(np.float32(float(v)))))
    bw = BigWig(str(out))
    hdr = bamio.read_bam(bam).header
    assert [bw.chroms[i] for i in range(len(bw.chroms))] == list(zip(hdr.ref_names, [int(x) for x in hdr.ref_lens]))
    got = bw.intervals()
    assert got == want
    covered = sum(b - a for _, a, b, _ in want)
    assert bw.summary[0] == covered
    assert bw.summary[1] == min(v for *_, v in want) and bw.summary[2] == max(v for *_, v in want)
    assert abs(bw.summary[3] - sum(v * (b - a) for _, a, b, v in want)) <= 1e-6 * bw.summary[3]
    assert 1 <= bw.n_zoom <= 10
    prev = 0
    for z in range(bw.n_zoom):
        red, recs = bw.zoom(z)
        assert red > prev
        prev = red
        assert sum(r[3] for r in recs) == covered                                   # every covered base in exactly one bin
        assert all(r[2] - r[1] <= red and r[3] <= r[2] - r[1] and r[4] <= r[5] for r in recs)
        assert abs(sum(r[6] for r in recs) - bw.summary[3]) <= 1e-3 * bw.summary[3]


def test_bigwig_many_chromosomes(tmp_path):
    """more chromosomes than one tree node holds (a two-level B+ tree) and more sections than one index node holds"""
    n = 700
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + ["@SQ\tSN:ctg%04d\tLN:%d" % (i, 5000 + i) for i in range(n)]
    sam = tmp_path / "h.sam"
    sam.write_text("\n".join(lines) + "\n")
    bed = tmp_path / "c.bedgraph"
    want = []
    with open(bed, "w") as f:
        f.write("track type=bedGraph\n")
        for i in range(0, n, 2):
            for j in range(3):
                f.write("ctg%04d\t%d\t%d\t%d\n" % (i, 10 + 100 * j, 60 + 100 * j, 1 + (i + j) % 7))
                want.append(("ctg%04d" % i, 10 + 100 * j, 60 + 100 * j, float(1 + (i + j) % 7)))
    out = tmp_path / "c.bigwig"
    r = subprocess.run([TOOL, "bedgraph2bw", str(sam), str(bed), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bw = BigWig(str(out))
    assert len(bw.chroms) == n and bw.chroms[699] == ("ctg0699", 5699)
    assert bw.intervals() == want


def test_mkbam_writes_what_the_python_writer_writes(tmp_path):
    """tbh_tool mkbam (the fast generator of the end-to-end bench leg) == synth.write_bams, record bytes and header"""
    from tiebrush_amd import bamio, synth
    tile = synth.make_tile(3, 1500, "c5", n_loci=40)
    a = synth.write_bams(tile, str(tmp_path / "py"))
    b = synth.write_bams_fast(tile, str(tmp_path / "cc"), threads=2)
    for pa, pb in zip(a, b):
        assert bamio.bgzf_decompress(open(pa, "rb").read()) == bamio.bgzf_decompress(open(pb, "rb").read())


def test_samtext_renders_golden_t2_as_the_reference_sam():
    """`test/t2/t2.sam` is the reference's own `samtools view` text of golden t2.bam: the tests' BAM -> SAM
    formatter reproduces it byte for byte (field text, tag types as samtools prints them, tag order), so a CLI output rendered by
    it can be compared with that file (tests/test_gpu_cli.py)."""
    import samtext
    from helpers import GOLDEN
    txt, recs = samtext.bam_to_sam_text(os.path.join(GOLDEN, "t2", "t2.bam"))
    lines = [ln for ln in txt.splitlines(True) if not ln.startswith("@")]
    gold = open(os.path.join(GOLDEN, "t2", "t2.sam")).read().splitlines(True)
    assert len(recs) == 8179 and lines == gold


def test_host_write_path_of_the_ranks_tool(tmp_path):
    """libtbh.so (include/tbh_host.h), the write-back half of `tiebrush --ranks`: raw records + YC / YX / YD in, parts of BGZF members
    out, header + parts + EOF = a BAM whose records carry the reference's tag forms (YC:f always, YX by value width, YD only when
    positive: tiebrush.cpp:506-525) — checked with the Python decoder on records of golden t1 (fresh records and records that
    already carry the tags)."""
    import ctypes as C
    from tiebrush_amd import _lib
    H = _lib.load_host()
    src = [os.path.join(GOLDEN, "t1", "t1s0.bam"), os.path.join(GOLDEN, "t1", "t1.bam")]
    assert [H.tbh_is_tiebrush(p.encode()) for p in src] == [0, 1]
    parts = []
    want = []
    # (the third part: t1s0's records over and over, more than 16384 of them — several slices, written in slice order)
    for pi, (p, many) in enumerate([(src[0], False), (src[1], False), (src[0], True)]):
        b = bamio.read_bam(p, keep_aux=True)
        n = 40000 if many else min(b.n, 3000)
        idx = [i % b.n for i in range(n)]
        recs = [bamio.record_bytes(b, i) for i in idx]                # raw records without block_size
        blob = np.frombuffer(b"".join(recs), np.uint8).copy()
        ln = np.array([len(r) for r in recs], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln)])[:-1].astype(np.uint64)
        rng = np.random.default_rng(5 + pi)
        yc = rng.integers(1, 70000, n).astype(np.float64)
        yx = rng.choice([1, 2, 254, 255, 65534, 65535, 70000], n).astype(np.int64)
        yd = rng.choice([0, 0, 3, 254, 255, 65535, 100000], n).astype(np.int32)
        part = str(tmp_path / ("p%d" % pi))
        assert H.tbh_tag_deflate_part(blob.ctypes.data, off.ctypes.data, ln.ctypes.data, n, yc.ctypes.data, yx.ctypes.data, yd.ctypes.data, 6, 3,
                                      part.encode()) == 0, H.tbh_last_error()
        parts.append(part)
        for i, j in enumerate(idx):
            # (an older integer-typed YC stays as it is: bam_aux_update_float refuses a non-float tag and the reference ignores
            # the return value, GSam.h:303-305 — the golden BAMs of 0.0.6 carry YC:i)
            old = {t: ty for t, ty, _ in bamio.record_aux(b, j)}.get("YC")
            want.append((bamio.record_identity(b, j), float(b.yc[j]) if old not in (None, "f", "d") else float(np.float32(yc[i])), int(yx[i]), int(yd[i]),
                         "f" if old in (None, "f", "d") else old))
    out = str(tmp_path / "o.bam")
    arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs])
    files = [os.path.join(GOLDEN, "t1", "t1s%d.bam" % i) for i in range(3)]
    cmd = ["tiebrush", "-o", out] + files
    assert H.tbh_write_bam_parts(out.encode(), b"0.0.7", len(cmd), arr(cmd), len(files), arr(files), len(parts), arr(parts), 1) == 0
    assert not os.path.exists(parts[0])
    o = bamio.read_bam(out, keep_aux=True)
    assert o.n == len(want) and o.header.is_tiebrush() and len(o.header.co_samples()) == 3
    for i, (ident, yc, yx, yd, yct) in enumerate(want):
        assert bamio.record_identity(o, i) == ident and o.has_yc[i] and o.yc[i] == yc and o.yx[i] == yx and o.yd[i] == yd, i
        types = {t: ty for t, ty, _ in bamio.record_aux(o, i)}
        assert types["YC"] == yct and ("YD" in types) == (yd > 0)
