"""`tiecov / tiebrush --thresholds T1,.. --depth-summary OUT.tsv` and `--features BED --feature-depth OUT.tsv` on the
goldens: the files against the model's text from that run's own bedgraph, the device path against the host path, streamed runs against
the unstreamed one, tiebrush's files against tiecov's on the BAM that run wrote, a region run, and the option rules.  The goldens' YC is
integral, so every sum is exact and the text cannot differ by a rounding."""
import os
import subprocess

import pytest

import depth_model as dm
import feature_scenes as fs
import multi_region as mr
import region_fixtures as rf
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu
BIN = rf.BIN
T_RUN = 120
THR_TEXT = ["2", "5", "10", "50", "1000", "30000"]
THR = ",".join(THR_TEXT)


def _run(tool, args, env=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})))


def _header(bam_loader, bam):
    h = bam_loader(bam).header
    return list(h.ref_names), list(h.ref_lens)


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_depth_summary_equals_the_model_the_host_and_the_streamed_runs(tmp_path, bam_loader, name):
    bam = os.path.join(GOLDEN, name, name + ".bam")
    names, lens = _header(bam_loader, bam)
    dev = tmp_path / "dev.tsv"
    r = _run("tiecov", ["--thresholds", THR, "--depth-summary", dev, "-c", tmp_path / "c", "-j", tmp_path / "j", bam], env=dict(TBK_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert "depth phase ms: device | %d references" % len(names) in r.stderr
    rows = fs.read_tracks(str(tmp_path / "c.bedgraph"), str(tmp_path / "j.bed"), names)       # this run's own bedgraph
    thr = [float(t) for t in THR_TEXT]
    want, total = dm.depth_tsv(names, lens, THR_TEXT, dm.per_ref(rows, lens, thr))
    assert dev.read_bytes() == want
    assert total["covered"] > 0 and total["ge"][0] > total["ge"][3] > 0
    host = tmp_path / "host.tsv"
    r = _run("tiecov", ["--thresholds", THR, "--depth-summary", host, bam], env=dict(TBK_TIMING="1", TBK_SUMMARY_HOST="1"))     # alone: it counts as an output
    assert r.returncode == 0 and "depth phase ms: host" in r.stderr, r.stderr
    assert host.read_bytes() == want
    for tile in ("1", "65536", "1M"):
        out = tmp_path / ("stream_%s.tsv" % tile)
        r = _run("tiecov", ["--stream", "--tile-bytes", tile, "--thresholds", THR, "--depth-summary", out, "-c", tmp_path / ("sc" + tile), bam], env=dict(TBK_TIMING="1"))
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == want, tile
        assert (tmp_path / ("sc%s.bedgraph" % tile)).read_bytes() == (tmp_path / "c.bedgraph").read_bytes()
        if tile == "1" and name == "t1":
            line = [ln for ln in r.stderr.splitlines() if ln.startswith("tiecov --stream phases ms:")]
            assert len(line) == 1 and int(line[0].split("(")[1].split()[0]) >= 2, r.stderr                # several tiles were added up
    # without --thresholds: no ge_ columns
    plain = tmp_path / "plain.tsv"
    r = _run("tiecov", ["--depth-summary", plain, bam])
    assert r.returncode == 0, r.stderr
    assert plain.read_bytes() == dm.depth_tsv(names, lens, [], dm.per_ref(rows, lens, []))[0]
    r = _run("tiecov", ["--stream", "--tile-bytes", "65536", "--depth-summary", tmp_path / "plain_s.tsv", bam], env=dict(TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "plain_s.tsv").read_bytes() == plain.read_bytes()


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_feature_depth_and_tiebrush(tmp_path, bam_loader, name):
    from tiebrush_amd import api
    bam = os.path.join(GOLDEN, name, name + ".bam")
    names, lens = _header(bam_loader, bam)
    rows = fs.read_tracks(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed"), names)
    bed = tmp_path / "features.bed"
    bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
    feats = api.features_from_bed(bam, str(bed))
    thr = [float(t) for t in THR_TEXT]
    d = tmp_path / "tc"
    d.mkdir()
    # beside the summary, the per-reference table and a bigWig: each is what it is alone
    r = _run("tiecov", ["--features", bed, "--feature-depth", d / "f.tsv", "--thresholds", THR, "--depth-summary", d / "d.tsv", "--summary", d / "s.tsv", "-c", d / "c", "-W", bam])
    assert r.returncode == 0, r.stderr
    own = fs.read_tracks(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed"), names)
    cov, ge = dm.per_row(own, feats, thr)
    want = dm.feature_tsv(names, feats, THR_TEXT, cov, ge)
    assert (d / "f.tsv").read_bytes() == want
    assert (d / "d.tsv").read_bytes() == dm.depth_tsv(names, lens, THR_TEXT, dm.per_ref(own, lens, thr))[0]
    assert sorted(os.listdir(str(d))) == ["c.bigwig", "d.tsv", "f.tsv", "s.tsv"]
    r = _run("tiecov", ["--features", bed, "--feature-depth", d / "fh.tsv", "--thresholds", THR, bam], env=dict(TBK_SUMMARY_HOST="1"))       # alone
    assert r.returncode == 0, r.stderr
    assert (d / "fh.tsv").read_bytes() == want
    # the run that writes the BAM writes the files tiecov makes of that BAM
    b = tmp_path / "tb"
    b.mkdir()
    r = _run("tiebrush", ["-o", b / "o.bam", "--features", bed, "--feature-depth", b / "f.tsv", "--thresholds", THR, "--depth-summary", b / "d.tsv"] + sample_paths(name),
             env=dict(TBK_TIMING="1"))
    assert r.returncode == 0 and "depth phase ms: device" in r.stderr, r.stderr
    r = _run("tiecov", ["--features", bed, "--feature-depth", b / "tf.tsv", "--thresholds", THR, "--depth-summary", b / "td.tsv", b / "o.bam"])
    assert r.returncode == 0, r.stderr
    assert (b / "f.tsv").read_bytes() == (b / "tf.tsv").read_bytes() and (b / "d.tsv").read_bytes() == (b / "td.tsv").read_bytes()
    assert len((b / "f.tsv").read_bytes().split(b"\n")) == len(want.split(b"\n")) and len((b / "d.tsv").read_bytes().split(b"\n")) == len(names) + 3
    r = _run("tiebrush", ["-o", b / "o2.bam", "--cov", b / "c", "--tabix", "--depth-summary", b / "d2.tsv", "--thresholds", THR] + sample_paths(name),
             env=dict(TBK_SUMMARY_HOST="1"))
    assert r.returncode == 0, r.stderr
    assert (b / "d2.tsv").read_bytes() == (b / "td.tsv").read_bytes() and os.path.exists(str(b / "c.bedgraph.gz.tbi"))


def test_feature_depth_under_regions(tmp_path, bam_loader):
    """inside the intervals the rows are the whole file's: a feature there gets the whole-file run's line; one outside is refused"""
    from tiebrush_amd import api
    bam = os.path.join(GOLDEN, "t2", "t2.bam")
    names, lens = _header(bam_loader, bam)
    rows = fs.read_tracks(os.path.join(GOLDEN, "t2", "t2.coverage.bedgraph"), os.path.join(GOLDEN, "t2", "t2.junctions.bed"), names)
    bed = tmp_path / "features.bed"
    bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
    fx = rf.Fixture(rf.golden_copy(tmp_path, "t2/t2.bam"), kinds=("bai",))
    feats = api.features_from_bed(fx.path, str(bed))
    r = _run("tiecov", ["--features", bed, "--feature-depth", tmp_path / "whole.tsv", "--thresholds", THR, fx.path])
    assert r.returncode == 0, r.stderr
    whole = (tmp_path / "whole.tsv").read_bytes().split(b"\n")
    t0 = int(feats["tid"][0])
    on = [k for k in range(len(feats["tid"])) if int(feats["tid"][k]) == t0 and feats["end"][k] - feats["beg"][k] < 100000]
    lo, hi = int(min(feats["beg"][k] for k in on)), int(max(feats["end"][k] for k in on))
    mid = (lo + hi) // 2
    iv = [(t0, mid, hi), (t0, lo, mid - 50)]
    table = mr.normalise(iv, lens)
    inside = [k for k in on if any(t == t0 and b <= feats["beg"][k] and feats["end"][k] <= e for t, b, e in table)]
    outside = [k for k in on if k not in inside]
    assert len(inside) >= 10 and outside
    src = open(str(bed)).read().split("\n")
    sub = tmp_path / "inside.bed"
    sub.write_text("".join(src[int(feats["line"][k]) - 1] + "\n" for k in inside))
    regions = mr.write_bed(str(tmp_path / "regions.bed"), names, iv)
    for env in ({}, dict(TBK_SUMMARY_HOST="1")):
        r = _run("tiecov", ["-R", regions, "--features", sub, "--feature-depth", tmp_path / "r.tsv", "--thresholds", THR, "-c", tmp_path / "rc", fx.path], env=env)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "r.tsv").read_bytes().split(b"\n") == [whole[0]] + [whole[1 + k] for k in inside] + [b""]
    out = tmp_path / "out"
    out.mkdir()
    mixed = tmp_path / "mixed.bed"
    mixed.write_text(src[int(feats["line"][inside[0]]) - 1] + "\n" + src[int(feats["line"][outside[0]]) - 1] + "\n")
    for tool, lead in (("tiecov", []), ("tiebrush", ["-o", out / "o.bam"])):
        r = _run(tool, lead + ["-R", regions, "--features", mixed, "--feature-depth", out / "x.tsv", "--thresholds", THR, fx.path])
        assert r.returncode == 1 and "mixed.bed line 2" in r.stderr and "inside" in r.stderr, r.stderr
        assert os.listdir(str(out)) == []


def test_option_rules(tmp_path, bam_loader):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    names, lens = _header(bam_loader, bam)
    fx = rf.Fixture(rf.golden_copy(tmp_path, "t1/t1.bam"), kinds=("bai",))
    bed = tmp_path / "f.bed"
    bed.write_text("%s\t1\t500\n" % names[0])
    bad = tmp_path / "bad.bed"
    bad.write_text("%s\t1\t5\n%s\t1\t5\tn\t0\tplus\n" % (names[0], names[0]))
    out = tmp_path / "out"
    out.mkdir()
    d, f, pre = out / "d.tsv", out / "f.tsv", out / "c"
    tb = ["-o", out / "o.bam"]
    S = sample_paths("t1")
    region = ["-r", names[0]]
    cases = [("tiecov", ["--thresholds", "2,x", "--depth-summary", d, "-c", pre, bam], "--thresholds: 'x' is not a decimal number"),
             ("tiecov", ["--thresholds", "5,2", "--depth-summary", d, bam], "--thresholds: '2' is not above the threshold before it"),
             ("tiecov", ["--thresholds", "0", "--depth-summary", d, bam], "--thresholds: '0' is not a finite number above 0"),
             ("tiecov", ["--thresholds", ",".join(str(k) for k in range(1, 18)), "--depth-summary", d, bam], "--thresholds: more than 16 thresholds"),
             ("tiecov", ["--stream", "--thresholds", "nan", "--depth-summary", d, bam], "--thresholds: 'nan' is not a decimal number"),
             ("tiecov", ["--thresholds", THR, "-c", pre, bam], "--thresholds needs --depth-summary OUT.tsv or --feature-depth OUT.tsv"),
             ("tiecov", ["--feature-depth", f, "--thresholds", THR, "-c", pre, bam], "--feature-depth needs --features BED"),
             ("tiecov", ["--feature-depth", f, "--features", bed, "-c", pre, bam], "--feature-depth needs --thresholds"),
             ("tiecov", ["--features", bed, "-c", pre, bam], "--features BED and --summary OUT.tsv go together (--summary is missing)"),
             ("tiecov", ["--features", bed, "--depth-summary", d, "--thresholds", THR, bam], "--features BED and --summary OUT.tsv go together (--summary is missing)"),
             ("tiecov", ["--features", bad, "--feature-depth", f, "--thresholds", THR, "-c", pre, bam], "bad.bed line 2"),
             ("tiecov", region + ["--depth-summary", d, "--thresholds", THR, "-c", pre, fx.path], "--depth-summary and -r / -R do not go together"),
             ("tiecov", ["--stream", "--features", bed, "--feature-depth", f, "--thresholds", THR, bam], "--stream and --features / --summary do not go together"),
             ("tiecov", ["--tabix", "--depth-summary", d, bam], "--tabix needs"),
             ("tiebrush", tb + ["--thresholds", "1,1", "--depth-summary", d] + S, "--thresholds: '1' is not above the threshold before it"),
             ("tiebrush", tb + ["--thresholds", THR] + S, "--thresholds needs --depth-summary OUT.tsv or --feature-depth OUT.tsv"),
             ("tiebrush", tb + ["--feature-depth", f, "--thresholds", THR] + S, "--feature-depth needs --features BED"),
             ("tiebrush", tb + ["--feature-depth", f, "--features", bed] + S, "--feature-depth needs --thresholds"),
             ("tiebrush", tb + ["--features", bed] + S, "--features BED and --summary OUT.tsv go together (--summary is missing)"),
             ("tiebrush", tb + region + ["--depth-summary", d, fx.path], "--depth-summary and -r / -R do not go together"),
             ("tiebrush", tb + ["--ranks", "2", "--depth-summary", d] + S, "--thresholds / --depth-summary / --feature-depth are not available with --ranks"),
             ("tiebrush", tb + ["--ranks=2", "--feature-depth=%s" % f, "--features=%s" % bed, "--thresholds=%s" % THR] + S,
              "--thresholds / --depth-summary / --feature-depth are not available with --ranks")]
    for tool, args, msg in cases:
        r = _run(tool, args)
        assert r.returncode == 1 and msg in r.stderr, (tool, args, r.stderr)
        assert "usage:" not in r.stderr, (tool, args)                  # the refusal's own sentence, not the usage text
        assert os.listdir(str(out)) == [], (tool, args)
    for tool in ("tiecov", "tiebrush"):
        r = _run(tool, ["--help"])
        text = r.stderr + r.stdout
        assert "--features BED --summary OUT.tsv" in text and "--depth-summary OUT.tsv" in text and "--feature-depth OUT.tsv" in text and "--thresholds T1,T2,..." in text
