"""The batch reader of a streamed decode (tiebrush_amd/csrc/host/stream_read.{h,cpp}) on the host alone: `tbh_tool batches`
on the goldens and on the framings of tests/bam_craft.py — records that straddle one and two members, members that lie inside one record,
empty members, a header through three members — at BYTES = 1 (a member a batch), a member's size, and more than the file.  For every
BYTES the batches' record ranges partition the file's records in order, every batch starts with the member that held the last tail, at
the tail; and what the reader refuses.  A stand-alone probe with the same loop is built plain and under the address and
undefined-behaviour sanitizers and must print the same lines."""
import os
import re
import subprocess

import pytest

import bam_craft as bc
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tiebrush_amd", "csrc", "host")
TOOL = os.path.join(ROOT, "tiebrush_amd", "_build", "tbh_tool")
PROBE = os.path.join(ROOT, "tests", "support", "stream_read_probe.cpp")
LINE = re.compile(r"batch (\d+) members=(\d+)\.\.(\d+) first_uoff=(\d+) records=(\d+)\.\.(\d+) tail=(\d+) last=([01])$")
CRAFTED = ("member_edges/member", "member_edges/hand", "huge_record/a", "huge_record/b", "big_header/member", "big_header/hand", "long_record/member",
           "long_record/hand")
GOLDENS = ("t1/t1.bam", "t2/t2.bam", "t12.bam", "t1/t1s0.bam", "t2/t2s0.bam")


def _files(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_read")
    out = {}
    for name in CRAFTED:
        p = str(d / (name.replace("/", "_") + ".bam"))
        with open(p, "wb") as f:
            f.write(bc.well_formed()[name].files[0])
        out[name] = p
    for g in GOLDENS:
        out[g] = os.path.join(GOLDEN, g)
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _files(tmp_path_factory)


def _batches(exe, path, nbytes, ok=True):
    r = subprocess.run([exe, "batches", path, str(nbytes)] if exe == TOOL else [exe, path, str(nbytes)], capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-1000:])
    return r


def _check(path, nbytes, text):
    """the lines against the file's own layout (bam_craft.Layout: every member, the header's end, the record chain)"""
    lay = bc.layout(open(path, "rb").read())
    mstart = list(lay.mstart) + [lay.n]
    offs = list(lay.offs) + [lay.n]
    nrec, nmem = len(lay.offs), len(lay.msize)
    lines = text.splitlines()
    assert lines[0].startswith("header n_targets=")
    end = re.match(r"end records=(\d+) members=(\d+) bytes_read=(\d+) reinflated=(\d+)$", lines[-1])
    assert end and int(end.group(1)) == nrec and int(end.group(2)) == nmem and int(end.group(3)) == os.path.getsize(path)
    rows = [tuple(int(x) for x in LINE.match(ln).groups()) for ln in lines[1:-1]]
    assert rows and [r[0] for r in rows] == list(range(len(rows)))
    prev_r1, prev_b, prev_tail_at = 0, None, lay.first
    for k, a, b, uoff, r0, r1, tail, last in rows:
        assert r0 == prev_r1 and r1 >= r0                          # the record ranges follow one another
        assert a < b <= nmem or (a == b == nmem)
        start = mstart[a] + uoff
        assert start == prev_tail_at == offs[r0], (k, start, prev_tail_at)   # the batch begins where the last one's whole records ended
        assert uoff < max(lay.msize[a], 1) if a < nmem else uoff == 0     # ... inside the member that holds that byte
        assert mstart[a] + tail == offs[r1], k                     # the tail by the host codec is the end of the batch's last whole record
        assert mstart[a] + tail <= mstart[b]
        if prev_b is not None:
            assert b > prev_b or last                              # every batch adds members (until the file ends)
            if nbytes == 1:
                assert b == prev_b + 1 or last
        prev_r1, prev_b, prev_tail_at = r1, b, mstart[a] + tail
    assert prev_r1 == nrec and rows[-1][7] == 1 and all(r[7] == 0 for r in rows[:-1])
    return rows, lay


def _member_bytes(path):
    """the compressed size of the file's first member"""
    data = open(path, "rb").read(18)
    return int.from_bytes(data[16:18], "little") + 1


@pytest.mark.parametrize("name", CRAFTED + GOLDENS)
def test_batches_partition_the_records(files, name):
    path = files[name]
    size = os.path.getsize(path)
    for nbytes in (1, _member_bytes(path), size + 1000):
        rows, lay = _check(path, nbytes, _batches(TOOL, path, nbytes).stdout)
        if nbytes > size:
            assert len(rows) == 1
        if nbytes == 1:
            assert len(rows) >= len([z for z in lay.msize if z]) - 4  # (about a batch a member; the header's members open the first)


def test_the_framings_are_what_they_are_there_for(files):
    """records straddle one and two members; a record longer than a batch makes batches without a whole record that keep their members"""
    rows, lay = _check(files["huge_record/a"], 1, _batches(TOOL, files["huge_record/a"], 1).stdout)
    empty = [r for r in rows if r[5] == r[4] and not r[7]]
    assert len(empty) >= 2                                          # batches that held no whole record ...
    grown = [r for r in rows if r[2] - r[1] >= 3]
    assert grown                                                    # ... kept all their members and added one, until the record was whole
    rows, lay = _check(files["big_header/hand"], 1, _batches(TOOL, files["big_header/hand"], 1).stdout)
    assert rows[0][1] == 2 and rows[0][3] > 0                       # the first record in the middle of the third member
    rows, lay = _check(files["member_edges/hand"], 1, _batches(TOOL, files["member_edges/hand"], 1).stdout)
    assert 0 in lay.msize[:-1] and any(r[3] > 0 for r in rows)      # empty members in the middle, batches that begin inside a member
    rows, lay = _check(files["t1/t1s0.bam"], 65536, _batches(TOOL, files["t1/t1s0.bam"], 65536).stdout)
    assert len(rows) >= 5 and len(lay.msize) > 200                  # (small members: a batch of 64 KiB holds some thirty of them)


def test_refusals_name_the_file(files, tmp_path):
    data = open(files["huge_record/a"], "rb").read()
    cases = {"cut_in_a_member": (data[:len(data) - 28 - 100], "truncated"),
             "garbage_behind": (data + b"not a member at all!", "not a BGZF"),
             "no_bam": (bc.frame(b"hello world, no BAM here"), "not a BAM")}
    lay = bc.layout(data)
    # the file cut at a member boundary inside the huge record: whole members, an incomplete last record
    off, k = 0, 0
    while k < 3:
        off += int.from_bytes(data[off + 16:off + 18], "little") + 1
        k += 1
    assert lay.mstart[3] not in lay.offs and lay.first < lay.mstart[3] < lay.n
    cases["cut_at_a_member_inside_a_record"] = (data[:off], "truncated")
    for name, (blob, word) in cases.items():
        p = str(tmp_path / (name + ".bam"))
        with open(p, "wb") as f:
            f.write(blob)
        for nbytes in (1, 1 << 20):
            r = _batches(TOOL, p, nbytes, ok=False)
            assert word in r.stderr and p in r.stderr, (name, r.stderr)


def _lib_sources():
    mk = open(os.path.join(HOST, "Makefile")).read()
    return [os.path.join(HOST, f) for f in re.search(r"^LIB := (.*)$", mk, re.M).group(1).split()]


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("srp")
    flags = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    exe = {k: str(d / ("stream_read_probe_" + k)) for k in flags}
    jobs = {k: subprocess.Popen(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + f + ["-o", exe[k], PROBE] + _lib_sources() + ["-lz", "-ldl"])
            for k, f in flags.items()}
    for k, j in jobs.items():
        assert j.wait() == 0, k
    return exe


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_probe_builds_print_the_tools_lines(files, probes, build, tmp_path):
    for name in ("huge_record/a", "big_header/hand", "member_edges/hand", "t1/t1.bam"):
        path = files[name]
        for nbytes in (1, _member_bytes(path), 1 << 30):
            want = _batches(TOOL, path, nbytes).stdout
            got = _batches(probes[build], path, nbytes)
            assert got.stdout == want and got.stderr == "", (name, nbytes, got.stderr[-2000:])
    p = str(tmp_path / "cut.bam")
    with open(p, "wb") as f:
        f.write(open(files["huge_record/a"], "rb").read()[:-200])
    r = _batches(probes[build], p, 1, ok=False)
    assert r.returncode == 1 and "truncated" in r.stderr
