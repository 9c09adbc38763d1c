"""`tiecov --gtf FILE --transcripts OUT.tsv` and `tiebrush ... --gtf FILE --transcripts OUT.tsv` on the goldens: the file
against the model's text, the device summariser against the host one, beside `--features --summary` and the tracks, tiebrush's file
against tiecov's on the BAM that run wrote, region runs, and the reference's example annotation on a crafted chr19 input.  The goldens'
YC is integral, so every sum is exact and the text cannot differ by a rounding."""
import os
import subprocess

import numpy as np
import pytest

import feature_scenes as fs
import multi_region as mr
import region_fixtures as rf
import tx_model as tm
import tx_scenes as ts
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu
BIN = rf.BIN
T_RUN = 120
GTF = os.path.join(GOLDEN, "sashimi", "example.gtf")


def _run(tool, args, env=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})))


def _golden(name, bam_loader, tmp_path):
    """the golden's BAM, header, rows (from its tracks) and a GTF of transcripts on them"""
    bam = os.path.join(GOLDEN, name, name + ".bam")
    h = bam_loader(bam).header
    names, lens = list(h.ref_names), list(h.ref_lens)
    rows = fs.read_tracks(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed"), names)
    gtf = tmp_path / "annot.gtf"
    gtf.write_text("\n".join(ts.golden_gtf(rows, names, lens)) + "\n")
    return bam, names, lens, rows, str(gtf)


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_transcripts_equal_the_model_the_host_and_tiebrush(tmp_path, bam_loader, name):
    from tiebrush_amd import api
    bam, names, lens, rows, gtf = _golden(name, bam_loader, tmp_path)
    tx = api.transcripts_from_gtf(bam, gtf)
    want = tm.tsv(names, tx, tm.per_row(rows, tx))
    dev, host, alone = tmp_path / "dev.tsv", tmp_path / "host.tsv", tmp_path / "alone.tsv"
    bed = tmp_path / "features.bed"
    bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
    # beside the tracks and --features --summary: they are what they are without the option
    r = _run("tiecov", ["--gtf", gtf, "--transcripts", dev, "--features", bed, "--summary", tmp_path / "sum.tsv", "-c", tmp_path / "c", "-j", tmp_path / "j", bam],
             env=dict(TBK_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert "transcripts phase ms: device | %d transcripts, %d exons" % (len(tx["tid"]), len(tx["ex_beg"])) in r.stderr
    assert dev.read_bytes() == want
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run("tiecov", ["--features", bed, "--summary", plain / "sum.tsv", "-c", plain / "c", "-j", plain / "j", bam])
    assert r.returncode == 0, r.stderr
    for f in ("c.bedgraph", "j.bed", "sum.tsv"):
        assert (tmp_path / f).read_bytes() == (plain / f).read_bytes(), f
    r = _run("tiecov", ["--gtf", gtf, "--transcripts", host, "-s", tmp_path / "s", bam], env=dict(TBK_TIMING="1", TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0 and "transcripts phase ms: host" in r.stderr, r.stderr
    assert host.read_bytes() == want
    # --transcripts alone counts as an output
    r = _run("tiecov", ["--transcripts", alone, "--gtf", gtf, bam])
    assert r.returncode == 0, r.stderr
    assert alone.read_bytes() == want
    assert sorted(os.listdir(tmp_path)) == ["alone.tsv", "annot.gtf", "c.bedgraph", "dev.tsv", "features.bed", "host.tsv", "j.bed", "plain", "s.bedgraph", "sum.tsv"]
    # the run that writes the BAM writes the file tiecov makes of that BAM, alone and beside its tracks
    d = tmp_path / "tb"
    d.mkdir()
    r = _run("tiebrush", ["-o", d / "o.bam", "--gtf", gtf, "--transcripts", d / "tb.tsv"] + sample_paths(name), env=dict(TBK_TIMING="1"))
    assert r.returncode == 0 and "transcripts phase ms: device" in r.stderr, r.stderr
    r = _run("tiecov", ["--gtf", gtf, "--transcripts", d / "tc.tsv", d / "o.bam"])
    assert r.returncode == 0, r.stderr
    assert (d / "tb.tsv").read_bytes() == (d / "tc.tsv").read_bytes()
    assert len((d / "tc.tsv").read_bytes().split(b"\n")) == len(want.split(b"\n"))
    r = _run("tiebrush", ["-o", d / "o2.bam", "--cov", d / "c", "--junc", d / "j", "--tabix", "--gtf", gtf, "--transcripts", d / "tb2.tsv"] + sample_paths(name),
             env=dict(TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0, r.stderr
    assert (d / "tb2.tsv").read_bytes() == (d / "tc.tsv").read_bytes() and os.path.exists(str(d / "c.bedgraph.gz")) and os.path.exists(str(d / "j.bed.gz.tbi"))


def test_transcripts_under_regions(tmp_path, bam_loader):
    """inside the intervals the rows are the whole file's: the transcripts there get the whole-file run's lines; one whose span is not
    inside one interval is refused with the line of its first exon"""
    from tiebrush_amd import api
    _, names, lens, rows, gtf = _golden("t2", bam_loader, tmp_path)
    fx = rf.Fixture(rf.golden_copy(tmp_path, "t2/t2.bam"), kinds=("bai",))
    tx = api.transcripts_from_gtf(fx.path, gtf)
    r = _run("tiecov", ["--gtf", gtf, "--transcripts", tmp_path / "whole.tsv", fx.path])
    assert r.returncode == 0, r.stderr
    whole = (tmp_path / "whole.tsv").read_bytes().split(b"\n")
    off = tx["tx_off"].astype(np.int64)
    span = [(int(tx["tid"][k]), int(tx["ex_beg"][off[k]]), int(tx["ex_end"][off[k + 1] - 1])) for k in range(len(tx["tid"]))]
    t0 = span[0][0]
    on = [k for k, s in enumerate(span) if s[0] == t0 and s[2] - s[1] < 20000]
    lo, hi = min(span[k][1] for k in on), max(span[k][2] for k in on)
    mid = (lo + hi) // 2
    iv = [(t0, mid, hi), (t0, lo, mid - 50)]
    table = mr.normalise(iv, lens)
    inside = [k for k in on if any(t == t0 and b <= span[k][1] and span[k][2] <= e for t, b, e in table)]
    outside = [k for k in on if k not in inside]
    assert len(inside) >= 5 and len(outside) >= 1
    src = open(gtf).read().split("\n")

    def lines_of(ks):
        ids = {tx["id"][k] for k in ks}
        return [ln for ln in src if ln and not ln.startswith("#") and ln.split("\t")[8].replace("transcript_id ", "\x00").split("\x00")[1].split(";")[0].strip(' "') in ids]
    sub = tmp_path / "inside.gtf"
    sub.write_text("\n".join(lines_of(inside)) + "\n")
    assert api.transcripts_from_gtf(fx.path, str(sub))["id"] == [tx["id"][k] for k in inside]
    regions = mr.write_bed(str(tmp_path / "regions.bed"), names, iv)
    for env in ({}, dict(TBK_SUMMARY_HOST="1")):
        r = _run("tiecov", ["-R", regions, "--gtf", sub, "--transcripts", tmp_path / "r.tsv", "-c", tmp_path / "rc", fx.path], env=env)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "r.tsv").read_bytes().split(b"\n") == [whole[0]] + [whole[1 + k] for k in inside] + [b""]
    # a transcript outside the table: refused with the line of its first exon, nothing written
    out = tmp_path / "out"
    out.mkdir()
    mixed = tmp_path / "mixed.gtf"
    head = lines_of(inside[:1])
    mixed.write_text("# one good transcript first\n" + "\n".join(head + lines_of(outside[:1])) + "\n")
    bad_tx = api.transcripts_from_gtf(fx.path, str(mixed))
    assert len(bad_tx["tid"]) == 2
    msg = "mixed.gtf line %d" % int(bad_tx["line"][1])
    r = _run("tiecov", ["-R", regions, "--gtf", mixed, "--transcripts", out / "x.tsv", "-c", out / "c", fx.path])
    assert r.returncode == 1 and msg in r.stderr and "inside" in r.stderr, r.stderr
    b, e = span[inside[0]][1], span[inside[0]][2]
    r = _run("tiecov", ["-r", "%s:%d-%d" % (names[t0], b + 2, e), "--gtf", mixed, "--transcripts", out / "x.tsv", "-j", out / "j", fx.path])
    assert r.returncode == 1 and "mixed.gtf line %d" % int(bad_tx["line"][0]) in r.stderr, r.stderr
    assert os.listdir(str(out)) == []
    r = _run("tiebrush", ["-o", out / "o.bam", "-R", regions, "--gtf", mixed, "--transcripts", out / "x.tsv", fx.path])
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert os.listdir(str(out)) == []
    r = _run("tiebrush", ["-o", out / "o.bam", "-R", regions, "--gtf", sub, "--transcripts", out / "x.tsv", fx.path])
    assert r.returncode == 0, r.stderr
    got = (out / "x.tsv").read_bytes().split(b"\n")
    assert got[0] + b"\n" == tm.HEADER.encode() and len(got) == len(inside) + 2


def test_the_reference_example_on_a_crafted_input(tmp_path):
    """tests/golden/sashimi/example.gtf against reads placed on chr19: spliced reads over the first transcript's introns, one of them
    on the other strand"""
    from tiebrush_amd import api, bamio
    names, lens = ["chr19"], [58617616]
    text = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr19\tLN:%d\n" % lens[0]
    hdr = str(tmp_path / "hdr.bam")
    bamio.write_bam(hdr, text, names, lens, b"", level=6)
    tx = api.transcripts_from_gtf(hdr, GTF)
    eb, ee = tx["ex_beg"][:5].tolist(), tx["ex_end"][:5].tolist()
    recs = []
    for k in range(4):                                            # 20 bases before the intron, the intron, 20 bases behind it
        n = ee[k] - 20, eb[k + 1] - ee[k]
        recs.append((n[0], [(20, "M"), (n[1], "N"), (20, "M")], b"-" if k != 2 else b"+", float(k + 2)))
    recs.sort(key=lambda r: r[0])
    sam = text + "".join("r%d\t0\tchr19\t%d\t60\t%s\t*\t0\t0\t%s\t*\tXS:A:%s\tYC:i:%d\n" % (i, p + 1, "".join("%d%s" % c for c in cig), "A" * 40, s.decode(), int(yc))
                         for i, (p, cig, s, yc) in enumerate(recs))
    inp = tmp_path / "in.sam"
    inp.write_text(sam)
    r = _run("tiecov", ["--gtf", GTF, "--transcripts", tmp_path / "x.tsv", "-c", tmp_path / "c", "-j", tmp_path / "j", inp])
    assert r.returncode == 0, r.stderr
    rows = fs.read_tracks(str(tmp_path / "c.bedgraph"), str(tmp_path / "j.bed"), names)
    assert len(rows["j_tid"]) == 4 and sorted(rows["j_strand"].tolist()) == sorted(b"---+")
    model = tm.per_row(rows, tx)
    assert (tmp_path / "x.tsv").read_bytes() == tm.tsv(names, tx, model)
    assert (model[0]["introns"], model[0]["introns_hit"], model[0]["junc_min"]) == (4, 3, 0.0) and model[0]["junc"] == [2.0, 3.0, 0.0, 5.0]
    assert model[0]["exons_hit"] == 5 and model[0]["covered"] == 160 and model[1]["introns_hit"] == 2 and model[2]["junc"] == model[1]["junc"]
