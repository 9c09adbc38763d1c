"""tbh::run_tracks and tbh::CovRecs (tiebrush_amd/csrc/host/tracks.{h,cpp}) — what tiecov and `tiebrush --cov / --junc / --samp` do
with their records — without a GPU.  tests/support/track_run_probe.cpp is compiled with the host sources and no libtbk, once as it is
and once under the address and undefined-behaviour sanitizers; its TrackApi is a table of scripted host stubs that log every call, so
the scenes check the capacities, the order of the calls, the retry, the fallbacks, the fatal messages and the bytes of the files."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_craft as bc
from bigwig_reader import BigWig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tiebrush_amd", "csrc", "host")
PROBE = os.path.join(ROOT, "tests", "support", "track_run_probe.cpp")

NAMES = ("chr1", "chr2")
IV = [(0, 10, 20, 1.0), (0, 20, 35, 2.5), (1, 5, 9, 1234.0625)]                     # the probe's canned rows
JUNC = [(0, 20, 300, 3.0, "+"), (1, 100, 250, 0.5, "-")]
SAMP = [(0, 10, 35, 2, 0.25), (1, 5, 9, 1, 1.0)]
COV_HEAD = "track type=bedGraph\n"
JUNC_HEAD = "track name=junctions\n"
SAMP_HEAD = ('track type=bedGraph name="Sample Count Heatmap" description="Sample Count Heatmap" visibility=full '
             'graphType="heatmap" color=200,100,0 altColor=0,100,200\n')
COV_TEXT = COV_HEAD + "".join("%s\t%d\t%d\t%.3f\n" % (NAMES[t], s, e, v) for t, s, e, v in IV)
JUNC_TEXT = JUNC_HEAD + "".join("%s\t%d\t%d\tJUNC%08d\t%.3f\t%c\n" % (NAMES[t], s, e, i + 1, v, st) for i, (t, s, e, v, st) in enumerate(JUNC))
SAMP_TEXT = SAMP_HEAD + "".join("%s\t%d\t%d\t%ld\t%f\n" % (NAMES[t], s, e, c, h) for t, s, e, c, h in SAMP)
RECS, CO = 3, 5                                                                    # the input's counts in every scene with rows
CAP_IV, CAP_J = 2 * CO + 2 * RECS + 16, CO + 16


def _lib_sources():
    mk = open(os.path.join(HOST, "Makefile")).read()
    return [os.path.join(HOST, f) for f in re.search(r"^LIB := (.*)$", mk, re.M).group(1).split()]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    """both builds, compiled side by side"""
    d = tmp_path_factory.mktemp("trp")
    flags = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    exe = {k: str(d / ("track_run_probe_" + k)) for k in flags}
    jobs = {k: subprocess.Popen(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + f + ["-o", exe[k], PROBE] + _lib_sources() + ["-lz", "-ldl"])
            for k, f in flags.items()}
    for k, j in jobs.items():
        assert j.wait() == 0, k
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, probes):
    return probes[request.param]


class Run:
    def __init__(self, probe, tmp_path, *args, ok=True):
        self.dir = str(tmp_path)
        r = subprocess.run([probe, "run", self.dir] + list(args), capture_output=True, text=True, env={k: v for k, v in os.environ.items() if not k.startswith("TBK_")})
        self.rc, self.err = r.returncode, r.stderr
        self.log = r.stdout.splitlines()
        assert (self.rc == 0) == ok, (self.rc, self.err[-2000:])

    def calls(self, name):
        return [dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in self.log if ln.split()[0] == name]

    def order(self):
        return [ln.split()[0] for ln in self.log]

    def text(self, name):
        return open(os.path.join(self.dir, name)).read()

    def host_tracks(self):
        return int(self.log[-1].split("host_tracks=")[1])


ROWS = ("recs=%d" % RECS, "co=%d" % CO)
ALL = ("cov=1", "junc=1", "samp=1")


def test_no_records(probe, tmp_path):
    r = Run(probe, tmp_path, *ALL)
    assert (r.text("c.bedgraph"), r.text("j.bed"), r.text("s.bedgraph")) == (COV_HEAD, JUNC_HEAD, SAMP_HEAD)
    assert r.order() == ["coverage_tile", "sample_tile", "times"]
    assert r.calls("coverage_tile") == [dict(ctx="1", recs="0", co="0", cap_intervals="16", cap_junctions="16")]


def test_plain_text(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, *ALL)
    assert (r.text("c.bedgraph"), r.text("j.bed"), r.text("s.bedgraph")) == (COV_TEXT, JUNC_TEXT, SAMP_TEXT)
    assert r.calls("coverage_tile") == [dict(ctx="1", recs=str(RECS), co=str(CO), cap_intervals=str(CAP_IV), cap_junctions=str(CAP_J))]
    assert r.calls("sample_tile") == [dict(call="1", num_samples="3", cap_intervals=str(CAP_IV))]
    assert r.order() == ["coverage_tile", "sample_tile", "times"]                   # the host formatter: no names, no device text
    assert r.host_tracks() == 3


def test_one_side_not_wanted(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, "junc=1")                                       # (a capacity of zero: that side is not computed)
    assert r.calls("coverage_tile")[0]["cap_intervals"] == "0" and r.calls("coverage_tile")[0]["cap_junctions"] == str(CAP_J)
    assert r.text("j.bed") == JUNC_TEXT and r.order() == ["coverage_tile", "times"]


def test_tabix(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, *ALL, "tabix=1")
    for name, want in (("c.bedgraph.gz", COV_TEXT), ("j.bed.gz", JUNC_TEXT), ("s.bedgraph.gz", SAMP_TEXT)):
        assert gzip.decompress(open(os.path.join(r.dir, name), "rb").read()).decode() == want
        assert os.path.getsize(os.path.join(r.dir, name + ".tbi")) > 0
    assert sorted(os.listdir(r.dir)) == sorted(n + e for n in ("c.bedgraph.gz", "j.bed.gz", "s.bedgraph.gz") for e in ("", ".tbi"))
    # the stub refuses every track before its first run: a line each on stderr, and the host path wrote them
    assert r.err.count("Warning: the device track writer refused") == 3 and "the stub writes no run" in r.err
    assert r.order() == ["coverage_tile", "track_names", "track_bgzf", "track_bgzf", "sample_tile", "track_bgzf", "times"]
    assert [c["kind"] for c in r.calls("track_bgzf")] == ["0", "1", "2"] and r.calls("track_bgzf")[0]["n_ref"] == "2"
    assert r.calls("track_names") == [dict(n="2", bytes="chr1chr2")]
    assert r.host_tracks() == 0                                                      # (no plain-text track)


@pytest.mark.parametrize("writer", ["host", "device"])
def test_bigwig(probe, tmp_path, writer):
    r = Run(probe, tmp_path, *ROWS, "cov=1", "bigwig=1", "bw_device=%d" % (writer == "device"))
    got = BigWig(os.path.join(r.dir, "c.bigwig")).intervals()
    assert got == [(NAMES[t], s, e, float(np.float32(v))) for t, s, e, v in IV]
    if writer == "device":                                                           # the stub refuses: the host producer takes the file
        assert r.calls("bigwig_build") == [dict(rows="3", n_ref="2")] and "Warning: the device bigWig writer refused" in r.err
    else:
        assert r.calls("bigwig_build") == [] and r.err == ""


def test_summary_alone(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, "summary=1")
    assert r.order() == ["coverage_tile", "cov_summary", "times"]
    assert r.calls("coverage_tile")[0]["cap_intervals"] == str(CAP_IV) and r.calls("coverage_tile")[0]["cap_junctions"] == str(CAP_J)
    assert r.calls("cov_summary") == [dict(intervals="3", junctions="2", features="2")]
    assert r.text("OUT.tsv") == ("#chrom\tstart\tend\tname\tstrand\tsize\tcovered\tsum\tmean0\tmean\tmax\tjunc\n"
                                 "chr1\t10\t30\tf0\t+\t20\t4\t10.000\t0.500\t2.500\t2.500\t0.000\n"
                                 "chr2\t100\t250\tf1\t.\t150\t5\t11.000\t0.073\t2.200\t2.500\t1.000\n")
    assert os.listdir(r.dir) == ["OUT.tsv"]


@pytest.mark.parametrize("regions", [1, 3])
def test_clip(probe, tmp_path, regions):
    r = Run(probe, tmp_path, *ROWS, *ALL, "summary=1", "clip=%d" % regions)
    one = regions == 1
    cov_clip, samp_clip = ("cov_clip", "sample_clip") if one else ("cov_clip_regions", "sample_clip_regions")
    assert r.order() == ["coverage_tile", "cov_summary", cov_clip, "sample_tile", samp_clip, "times"]   # the summary before the cut
    assert r.calls("coverage_tile")[0]["cap_intervals"] == str(CAP_IV + regions) and r.calls("coverage_tile")[0]["cap_junctions"] == str(CAP_J)
    assert r.calls("sample_tile") == [dict(call="1", num_samples="3", cap_intervals=str(CAP_IV + regions))]
    if one:
        assert r.calls(cov_clip) == [dict(rows="3", tid="0", beg="5", end="40")] and r.calls(samp_clip) == [dict(rows="2", tid="0", beg="5", end="40")]
    else:
        assert r.calls(cov_clip) == [dict(rows="3", regions="3")] and r.calls(samp_clip) == [dict(rows="2", regions="3")]
    assert (r.text("c.bedgraph"), r.text("j.bed"), r.text("s.bedgraph")) == (COV_TEXT, JUNC_TEXT, SAMP_TEXT)


@pytest.mark.parametrize("regions", [0, 3])
def test_sample_e2big(probe, tmp_path, regions):
    r = Run(probe, tmp_path, *ROWS, "samp=1", "e2big=40", *(["clip=%d" % regions] if regions else []))
    assert [c["cap_intervals"] for c in r.calls("sample_tile")] == [str(CAP_IV + regions), str(40 + 16 + regions)]   # exactly two calls
    assert r.text("s.bedgraph") == SAMP_TEXT


def test_device_text(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, *ALL, "device_text=1")
    assert r.order() == ["track_names", "coverage_tile", "format_track", "format_track", "sample_tile", "format_track", "times"]
    assert r.calls("track_names") == [dict(n="2", bytes="chr1chr2")]
    assert r.text("c.bedgraph") == COV_HEAD + "MARKER kind=0 rows=3\n" and r.text("j.bed") == JUNC_HEAD + "MARKER kind=1 rows=2\n"
    assert r.text("s.bedgraph") == SAMP_HEAD + "MARKER kind=2 rows=2\n"
    assert r.host_tracks() == 0


def test_device_text_with_tabix_sets_the_names_once(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, *ALL, "device_text=1", "tabix=1")
    assert r.order() == ["track_names", "coverage_tile", "track_bgzf", "track_bgzf", "sample_tile", "track_bgzf", "times"]


def test_device_text_refused(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, "cov=1", "device_text=1", "fmt=unsupported")
    assert r.text("c.bedgraph") == COV_TEXT and r.host_tracks() == 1
    assert r.order() == ["track_names", "coverage_tile", "format_track", "times"]


def test_device_text_sink_failure(probe, tmp_path):
    r = Run(probe, tmp_path, *ROWS, "cov=1", "device_text=1", "fmt=sinkfail", ok=False)
    assert "failed to write an output line" in r.err


def test_null_entries_are_fatal(probe, tmp_path):
    for i, (args, msg) in enumerate([(("cov=1", "tabix=1", "device_text=1", "null=track_bgzf"), "Error: --tabix: libtbk.so lacks tbk_track_bgzf\n"),
                                     (("cov=1", "bigwig=1", "bw_device=1", "null=bigwig_build"), "Error: --bigwig-writer device: libtbk.so lacks tbk_bigwig_build\n"),
                                     (("summary=1", "null=cov_summary"), "Error: --summary: the loaded libtbk.so has no tbk_cov_summary (an older build?)\n")]):
        d = tmp_path / str(i)
        d.mkdir()
        r = Run(probe, d, *ROWS, *args, ok=False)
        assert r.rc == 1 and r.err == msg
    # without the device writer nobody asks for tbk_bigwig_build
    d = tmp_path / "host"
    d.mkdir()
    Run(probe, d, *ROWS, "cov=1", "bigwig=1", "null=bigwig_build")


def test_strand_rule_and_record_table(probe, tmp_path):
    M, N, S = bc.M, bc.N, bc.S
    T = bc.tag
    cases = [  # aux, flag, cigar -> strand, yc, yx
        (T("XS", "A", "+"), 16, ((10, M),), "+", 1.0, 1),
        (T("XS", "A", "-"), 0, ((5, S), (10, M), (100, N), (7, M)), "-", 1.0, 1),
        (T("ts", "A", "+"), 0, ((10, M),), "+", 1.0, 1),
        (T("ts", "A", "+"), 16, ((10, M),), "-", 1.0, 1),
        (T("ts", "A", "-"), 16, ((10, M), (50, N), (10, M)), "+", 1.0, 1),
        (b"", 0, ((10, M),), ".", 1.0, 1),
        (T("XS", "i", 43), 0, ((10, M),), ".", 1.0, 1),                             # XS of an odd type is no strand ...
        (T("XS", "i", 43) + T("ts", "A", "-"), 0, ((10, M),), "-", 1.0, 1),         # ... and leaves the word to ts
        (T("ts", "A", "-") + T("XS", "Z", "+x"), 16, ((10, M),), "+", 1.0, 1),      # XS wins wherever it stands
        (T("YC", "f", 2.5) + T("YX", "C", 4) + T("XS", "A", "-"), 0, (), "-", 2.5, 4),
        (T("XS", "A", "?") + T("ts", "A", "+"), 0, ((10, M),), ".", 1.0, 1),
    ]
    recs = [bc.Rec(tid=i % 2, pos=100 + i, flag=flag, cigar=cigar, name=b"r%d" % i, aux=aux) for i, (aux, flag, cigar, _, _, _) in enumerate(cases)]
    path = str(tmp_path / "strand.bam")
    open(path, "wb").write(bc.one_member(recs))
    r = subprocess.run([probe, "strand", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want, off = [], 0
    for i, (aux, flag, cigar, strand, yc, yx) in enumerate(cases):
        want.append(" ".join(["%d %d %d %s %g %d %d %d" % (i % 2, 100 + i, flag, strand, yc, yx, off, len(cigar))] + [str((l << 4) | o) for l, o in cigar]))
        off += len(cigar)
    assert r.stdout.splitlines() == want
