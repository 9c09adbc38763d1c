"""`tiecov -W --bigwig-writer device` and `tiebrush --cov P --bigwig --bigwig-writer device` on the golden samples: the device-built
file against the default (host) writer's by the contract of DESIGN.md 4h — the same levels, reductions, sections, payload bytes,
R-tree keys, chromosome tree, summary, section count and uncompressBufSize; only the compressed bytes may differ."""
import os
import shutil
import subprocess

import pytest

import bigwig_payloads as bp
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")


def _run(exe, args, ok=True):
    r = subprocess.run([os.path.join(BIN, exe)] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, TBK_TIMING="1"))
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _writer_line(r):
    return [ln for ln in r.stderr.splitlines() if ln.startswith("bigwig phase ms:")]


def _pair(tmp_path, bam, extra):
    """the same tiecov -W run with the default writer and with the device writer -> (host view, device view)"""
    h, d = str(tmp_path / "host"), str(tmp_path / "dev")
    rh = _run("tiecov", ["-W", "-c", h] + extra + [bam])
    rd = _run("tiecov", ["-W", "--bigwig-writer", "device", "-c", d] + extra + [bam])
    assert len(_writer_line(rh)) == 1 and "writer host" in _writer_line(rh)[0]
    assert len(_writer_line(rd)) == 1 and "writer device" in _writer_line(rd)[0], rd.stderr
    return bp.file_view(h + ".bigwig"), bp.file_view(d + ".bigwig")


def _indexed(tmp_path, name):
    bam = str(tmp_path / (name + ".bam"))
    shutil.copy(os.path.join(GOLDEN, name, name + ".bam"), bam)
    r = subprocess.run([os.path.join(BIN, "tbh_tool"), "bai", bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return bam


def _golden_rows(name):
    rows = []
    for ln in open(os.path.join(GOLDEN, name, name + ".coverage.bedgraph")):
        f = ln.split("\t")
        if len(f) == 4:
            rows.append((f[0], int(f[1]), int(f[2])))
    return rows


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tiecov_device_writer_equals_default(tmp_path, name):
    host, dev = _pair(tmp_path, os.path.join(GOLDEN, name, name + ".bam"), [])
    bp.same_files(dev, host)
    assert sum(len(lv["sections"]) for lv in host["levels"]) > 1 and host["levels"][0]["n_items"] == len(_golden_rows(name))


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tiecov_region_device_writer(tmp_path, name):
    """-r: the writer takes the clipped rows (the same run_tracks)"""
    rows = _golden_rows(name)
    a, b = rows[len(rows) // 3], rows[len(rows) // 2]
    chrom = a[0]
    beg, end = a[1] + 1, (b[2] if b[0] == chrom else a[2] + 5000)
    bam = _indexed(tmp_path, name)
    host, dev = _pair(tmp_path, bam, ["-r", "%s:%d-%d" % (chrom, beg + 1, end)])
    bp.same_files(dev, host)
    assert 0 < host["levels"][0]["n_items"] < len(rows)


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tiecov_regions_file_device_writer(tmp_path, name):
    rows = _golden_rows(name)
    picks = [rows[len(rows) // 5], rows[len(rows) // 2], rows[(4 * len(rows)) // 5]]
    bed = str(tmp_path / "u.bed")
    with open(bed, "w") as f:
        for c, s, e in picks:
            f.write("%s\t%d\t%d\n" % (c, max(0, s - 700), e + 900))
    bam = _indexed(tmp_path, name)
    host, dev = _pair(tmp_path, bam, ["-R", bed])
    bp.same_files(dev, host)
    assert 0 < host["levels"][0]["n_items"] < len(rows)


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tiebrush_device_writer_equals_tiecov_of_its_output(tmp_path, name):
    out, pre, ref = str(tmp_path / "o.bam"), str(tmp_path / "tb"), str(tmp_path / "tc")
    r = _run("tiebrush", ["-o", out, "--cov", pre, "--bigwig", "--bigwig-writer", "device"] + sample_paths(name))
    assert len(_writer_line(r)) == 1 and "writer device" in _writer_line(r)[0], r.stderr
    _run("tiecov", ["-W", "-c", ref, out])
    bp.same_files(bp.file_view(pre + ".bigwig"), bp.file_view(ref + ".bigwig"))


def test_option_refused_without_bigwig(tmp_path):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    r = _run("tiecov", ["--bigwig-writer", "device", "-c", tmp_path / "x", bam], ok=False)
    assert r.returncode != 0 and "--bigwig-writer needs -W" in r.stderr and not os.path.exists(str(tmp_path / "x.bedgraph"))
    r = _run("tiecov", ["-W", "--bigwig-writer", "gpu", "-c", tmp_path / "x", bam], ok=False)
    assert r.returncode != 0 and "host or device" in r.stderr
    r = _run("tiebrush", ["-o", tmp_path / "o.bam", "--cov", tmp_path / "y", "--bigwig-writer", "device"] + sample_paths("t1"), ok=False)
    assert r.returncode != 0 and "--bigwig-writer needs --bigwig" in r.stderr and not os.path.exists(str(tmp_path / "o.bam"))
