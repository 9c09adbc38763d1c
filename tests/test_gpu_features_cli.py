"""`tiecov --features BED --summary OUT.tsv` and `tiebrush ... --features BED --summary OUT.tsv` on the goldens: the file
against the model's text, the device summariser against the host one, tiebrush's file against tiecov's on the BAM that run wrote, region
runs, and the option rules.  The goldens' YC is integral, so every sum is exact and the text cannot differ by a rounding."""
import os
import subprocess

import pytest

import feature_model as fm
import feature_scenes as fs
import multi_region as mr
import region_fixtures as rf
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu
BIN = rf.BIN
T_RUN = 120
HEAD = b"#chrom\tstart\tend\tname\tstrand\tsize\tcovered\tsum\tmean0\tmean\tmax\tjunc\n"


def _run(tool, args, env=None, cwd=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})),
                          cwd=cwd)


def _golden(name, bam_loader, tmp_path):
    """the golden's BAM, header, rows (from its tracks) and a BED of features on them"""
    bam = os.path.join(GOLDEN, name, name + ".bam")
    h = bam_loader(bam).header
    names, lens = list(h.ref_names), list(h.ref_lens)
    rows = fs.read_tracks(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed"), names)
    bed = tmp_path / "features.bed"
    bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
    return bam, names, lens, rows, str(bed)


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_summary_equals_the_model_the_host_and_tiebrush(tmp_path, bam_loader, name):
    from tiebrush_amd import api
    bam, names, lens, rows, bed = _golden(name, bam_loader, tmp_path)
    feats = api.features_from_bed(bam, bed)
    want = fm.tsv(names, feats, fm.mark_dyadic(rows, fm.per_row(rows, feats)))
    dev, host, alone = tmp_path / "dev.tsv", tmp_path / "host.tsv", tmp_path / "alone.tsv"
    # beside the tracks: they are what they are without the option
    r = _run("tiecov", ["--features", bed, "--summary", dev, "-c", tmp_path / "c", "-j", tmp_path / "j", bam], env=dict(TBK_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert "summary phase ms: device | %d features" % len(feats["tid"]) in r.stderr
    assert dev.read_bytes() == want
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run("tiecov", ["-c", plain / "c", "-j", plain / "j", bam])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "c.bedgraph").read_bytes() == (plain / "c.bedgraph").read_bytes() and (tmp_path / "j.bed").read_bytes() == (plain / "j.bed").read_bytes()
    r = _run("tiecov", ["--features", bed, "--summary", host, "-s", tmp_path / "s", bam], env=dict(TBK_TIMING="1", TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0 and "summary phase ms: host" in r.stderr, r.stderr
    assert host.read_bytes() == want
    # --summary alone counts as an output
    r = _run("tiecov", ["--summary", alone, "--features", bed, bam])
    assert r.returncode == 0, r.stderr
    assert alone.read_bytes() == want
    assert sorted(os.listdir(tmp_path)) == ["alone.tsv", "c.bedgraph", "dev.tsv", "features.bed", "host.tsv", "j.bed", "plain", "s.bedgraph"]
    # the run that writes the BAM writes the file tiecov makes of that BAM, alone and beside its tracks (the BAM is this run's own
    # collapse of the samples, not the golden: only the line count is the model's)
    d = tmp_path / "tb"
    d.mkdir()
    r = _run("tiebrush", ["-o", d / "o.bam", "--features", bed, "--summary", d / "tb.tsv"] + sample_paths(name), env=dict(TBK_TIMING="1"))
    assert r.returncode == 0 and "summary phase ms: device" in r.stderr, r.stderr
    r = _run("tiecov", ["--features", bed, "--summary", d / "tc.tsv", d / "o.bam"])
    assert r.returncode == 0, r.stderr
    assert (d / "tb.tsv").read_bytes() == (d / "tc.tsv").read_bytes()
    assert len((d / "tc.tsv").read_bytes().split(b"\n")) == len(want.split(b"\n"))
    r = _run("tiebrush", ["-o", d / "o2.bam", "--cov", d / "c", "--junc", d / "j", "--tabix", "--features", bed, "--summary", d / "tb2.tsv"] + sample_paths(name),
             env=dict(TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0, r.stderr
    assert (d / "tb2.tsv").read_bytes() == (d / "tc.tsv").read_bytes() and os.path.exists(str(d / "c.bedgraph.gz")) and os.path.exists(str(d / "j.bed.gz.tbi"))


def test_summary_under_regions(tmp_path, bam_loader):
    """inside the intervals the rows are the whole file's: the features there get the whole-file run's lines; one outside is refused"""
    from tiebrush_amd import api
    _, names, lens, rows, bed = _golden("t2", bam_loader, tmp_path)
    fx = rf.Fixture(rf.golden_copy(tmp_path, "t2/t2.bam"), kinds=("bai",))
    feats = api.features_from_bed(fx.path, bed)
    r = _run("tiecov", ["--features", bed, "--summary", tmp_path / "whole.tsv", fx.path])
    assert r.returncode == 0, r.stderr
    whole = (tmp_path / "whole.tsv").read_bytes().split(b"\n")
    # a table of three intervals around a third of the features each (unsorted in the file, two of them abut)
    t0 = int(feats["tid"][0])
    on = [k for k in range(len(feats["tid"])) if int(feats["tid"][k]) == t0 and feats["end"][k] - feats["beg"][k] < 100000]
    lo, hi = int(min(feats["beg"][k] for k in on)), int(max(feats["end"][k] for k in on))
    mid = (lo + hi) // 2
    iv = [(t0, mid, hi), (t0, lo, (lo + mid) // 2), (t0, (lo + mid) // 2, mid - 50)]
    table = mr.normalise(iv, lens)
    assert len(table) == 2
    inside = [k for k in on if any(t == t0 and b <= feats["beg"][k] and feats["end"][k] <= e for t, b, e in table)]
    assert 10 <= len(inside) < len(on)
    src = open(bed).read().split("\n")
    sub = tmp_path / "inside.bed"
    sub.write_text("".join(src[int(feats["line"][k]) - 1] + "\n" for k in inside))
    regions = mr.write_bed(str(tmp_path / "regions.bed"), names, iv)
    for env in ({}, dict(TBK_SUMMARY_HOST="1")):
        r = _run("tiecov", ["-R", regions, "--features", sub, "--summary", tmp_path / "r.tsv", "-c", tmp_path / "rc", fx.path], env=env)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "r.tsv").read_bytes().split(b"\n") == [whole[0]] + [whole[1 + k] for k in inside] + [b""]
    k = inside[0]
    one = tmp_path / "one.bed"
    one.write_text(src[int(feats["line"][k]) - 1] + "\n")
    r = _run("tiecov", ["-r", "%s:%d-%d" % (names[t0], int(feats["beg"][k]) + 1, int(feats["end"][k])), "--features", one, "--summary", tmp_path / "one.tsv", fx.path])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.tsv").read_bytes().split(b"\n") == [whole[0], whole[1 + k], b""]
    # a feature across the gap of the table, and one outside it: refused with the line, nothing written
    out = tmp_path / "out"
    out.mkdir()
    gap = tmp_path / "gap.bed"
    gap.write_text("# two good ones first\n" + src[int(feats["line"][inside[0]]) - 1] + "\n%s\t%d\t%d\tacross\n" % (names[t0], mid - 60, mid + 10))
    r = _run("tiecov", ["-R", regions, "--features", gap, "--summary", out / "x.tsv", "-c", out / "c", fx.path])
    assert r.returncode == 1 and "gap.bed line 3" in r.stderr and "inside" in r.stderr, r.stderr
    r = _run("tiecov", ["-r", "%s:%d-%d" % (names[t0], lo + 1, mid), "--features", sub, "--summary", out / "x.tsv", "-j", out / "j", fx.path])
    assert r.returncode == 1 and "inside.bed line" in r.stderr, r.stderr
    assert os.listdir(str(out)) == []
    # tiebrush -R: the same rule against its region table
    r = _run("tiebrush", ["-o", out / "o.bam", "-R", regions, "--features", gap, "--summary", out / "x.tsv", fx.path])
    assert r.returncode == 1 and "gap.bed line 3" in r.stderr, r.stderr
    assert os.listdir(str(out)) == []
    r = _run("tiebrush", ["-o", out / "o.bam", "-R", regions, "--features", sub, "--summary", out / "x.tsv", fx.path])
    assert r.returncode == 0, r.stderr
    assert (out / "x.tsv").read_bytes().split(b"\n")[0] + b"\n" == HEAD and len((out / "x.tsv").read_bytes().split(b"\n")) == len(inside) + 2


def test_option_rules(tmp_path, bam_loader):
    bam, names, lens, rows, bed = _golden("t1", bam_loader, tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    tsv, pre = out / "x.tsv", out / "c"
    bad = tmp_path / "bad.bed"
    bad.write_text("%s\t1\t5\n%s\t1\t5\tn\t0\tplus\n" % (names[0], names[0]))
    unknown = tmp_path / "unknown.bed"
    unknown.write_text("%s\t1\t5\n\nnochrom\t1\t5\n" % names[0])
    empty = tmp_path / "empty.bed"
    empty.write_text("%s\t%d\t%d\n" % (names[0], lens[0], lens[0] + 5))
    cases = [("tiecov", ["--summary", tsv, "-c", pre, bam], "--features"),
             ("tiecov", ["--features", bed, "-c", pre, bam], "--summary"),
             ("tiecov", ["--features", bed, bam], "--summary"),
             ("tiecov", ["--features", bad, "--summary", tsv, "-c", pre, bam], "bad.bed line 2"),
             ("tiecov", ["--features", unknown, "--summary", tsv, "-c", pre, bam], "unknown.bed line 3"),
             ("tiecov", ["--features", empty, "--summary", tsv, "-c", pre, bam], "empty.bed line 1"),
             ("tiecov", ["--features", tmp_path / "missing.bed", "--summary", tsv, "-c", pre, bam], "cannot read"),
             ("tiecov", ["--tabix", "--features", bed, "--summary", tsv, bam], "--tabix needs"),
             ("tiebrush", ["-o", out / "o.bam", "--summary", tsv] + sample_paths("t1"), "--features"),
             ("tiebrush", ["-o", out / "o.bam", "--features", bed] + sample_paths("t1"), "--summary"),
             ("tiebrush", ["-o", out / "o.bam", "--features", bad, "--summary", tsv, "--cov", pre] + sample_paths("t1"), "bad.bed line 2"),
             ("tiebrush", ["-o", out / "o.bam", "--ranks", "2", "--features", bed, "--summary", tsv] + sample_paths("t1"), "--ranks"),
             ("tiebrush", ["-o", out / "o.bam", "--ranks=2", "--summary=%s" % tsv, "--features=%s" % bed] + sample_paths("t1"), "--ranks")]
    for tool, args, msg in cases:
        r = _run(tool, args)
        assert r.returncode == 1 and msg in r.stderr, (tool, args, r.stderr)
        assert os.listdir(str(out)) == [], (tool, args)
    for tool in ("tiecov", "tiebrush"):
        r = _run(tool, ["--help"])
        assert "--features BED --summary OUT.tsv" in r.stderr + r.stdout
