"""`tiebrush --index` and tbk_bam_encode_indexed (baix.hip): the index part of every encoded run and the .bai of every route's output
against the restatement of the index contract in bai_reader.py, exactly."""
import os
import subprocess

import numpy as np
import pytest

import bai_reader as br
from helpers import GOLDEN, sample_paths
from test_gpu_encode import _golden_case

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiebrush_amd", "_build")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden_ref_len():
    return br.read_bam(open(os.path.join(GOLDEN, "t12.bam"), "rb").read())[1]


def check_part(run, part, ref_len):
    want = br.expected_part(run, ref_len)
    assert np.array_equal(part["rec_vbeg"], want["rec_vbeg"])
    assert [tuple(int(x) for x in c) for c in part["chunks"][["tid", "bin", "beg", "end"]].tolist()] == want["chunks"]
    assert part["lin_first"] == want["lin_first"] and np.array_equal(part["lin"], want["lin"])
    assert [tuple(int(x) for x in r) for r in part["refs"][["tid", "n_records", "first", "last"]].tolist()] == want["refs"]


@pytest.mark.parametrize("case", ["t1", "t2", "t12"])
def test_library_part_equals_the_restatement_on_goldens(ctx, golden_ref_len, case):
    if case == "t12":
        names, tb = ["t1/t1.bam", "t2/t2.bam"], [1, 1]
    else:
        names, tb = [os.path.relpath(p, GOLDEN) for p in sample_paths(case)], [0] * 10
    s, rep, yc, yx, yd = _golden_case(ctx, names, tb, keep_results=True)
    n_dev, m = int(s.n_records), len(rep)
    blob, off = ctx.bam_records(rep)
    recs = {i: blob[int(off[i]) + 4:int(off[i + 1])] for i in range(m)}
    half = n_dev // 2
    for nd, host in ((n_dev, None), (0, recs), (half, {i: r for i, r in recs.items() if rep[i] >= half})):   # the three hand-over forms
        want, pay = ctx.bam_encode(rep, yc, yx, yd, n_dev=nd, host_records=host)
        run, pay_i, part = ctx.bam_encode_indexed(rep, yc, yx, yd, golden_ref_len, n_dev=nd, host_records=host)
        assert run == want and pay_i == pay
        check_part(run, part, golden_ref_len)
    a, b = 7, m - 11                                                 # TBK_MEM_KEPT, a range that does not start at group 0
    want, _ = ctx.bam_encode(rep[a:b], None, None, None, n_dev=n_dev, kept_first=a)
    run, _, part = ctx.bam_encode_indexed(rep[a:b], None, None, None, golden_ref_len, n_dev=n_dev, kept_first=a)
    assert run == want
    check_part(run, part, golden_ref_len)
    ctx.bam_release()


def test_library_part_on_the_synthetic_records(ctx):
    """every shape of bai_reader.synthetic_records as host records: runs of exactly 63 .. 257 records of one bin, nine members and more"""
    recs = [r[4:] for r in br.synthetic_records()]
    n = len(recs)
    yc, yx, yd = np.ones(n), np.arange(n) % 300, np.arange(n) % 3
    run, _, part = ctx.bam_encode_indexed(np.arange(n, dtype=np.uint32), yc, yx, yd, br.SYN_LENS, n_dev=0, host_records=dict(enumerate(recs)))
    assert run == ctx.bam_encode(np.arange(n, dtype=np.uint32), yc, yx, yd, n_dev=0, host_records=dict(enumerate(recs)))[0]
    assert len(br.members(run)) >= 9
    check_part(run, part, br.SYN_LENS)
    for w, k in br.SYN_RUNS.items():                                 # each run is one chunk or, across members, chunks that cover k records
        ch = [c for c in part["chunks"] if c["tid"] == 0 and c["bin"] == 4681 + w]
        vb = part["rec_vbeg"]
        assert sum(int(np.sum((vb[:-1] >= c["beg"]) & (vb[:-1] < c["end"]))) for c in ch) == k
    assert [int(t) for t in part["refs"]["tid"]] == [0, 2]


@pytest.mark.parametrize("scan", ["lookback", "3pass"])
def test_library_part_under_each_form_of_the_scan_engine(scan, monkeypatch):
    """scan= forces one form for every scan_op_run: the running maximum of the record ends (ix_max_scan) over 3 * 2048 + 5 records — three
    full tiles and a short one, long records that carry their end across them, two references — under each form, against the restatement;
    the look-back launches the scan's name once, the three-launch form twice (reduce and down-sweep)"""
    from helpers import tbk_debug
    from tiebrush_amd import api, bamio
    n = 3 * 2048 + 5
    rng = np.random.default_rng(29)
    ref_len = [200000, 1000, 300000]
    tid = np.sort(rng.choice([0, 2], n))
    pos = rng.integers(0, 150000, n)
    pos = pos[np.lexsort((pos, tid))]
    recs = {i: bamio.encode_record(int(tid[i]), int(pos[i]), 0, 60, [int(rng.choice([30, 50, 2000, 40000])) << 4], b"r%d" % i)[4:] for i in range(n)}
    tbk_debug(monkeypatch, scan=scan)
    c = api.Context(0)
    c.set_profiling(True)
    try:
        run, _, part = c.bam_encode_indexed(np.arange(n, dtype=np.uint32), np.ones(n), np.ones(n), np.zeros(n), ref_len, n_dev=0, host_records=recs)
        kt = c.kernel_times()
        check_part(run, part, ref_len)
        assert kt["ix_max_scan"][1] == (1 if scan == "lookback" else 2), kt
    finally:
        c.close()


def test_library_refusals_leave_the_context_usable(ctx):
    from tiebrush_amd import bamio
    from tiebrush_amd.api import TbkError
    ok = bamio.encode_record(0, 100, 0, 60, [50 << 4], b"a")[4:]
    ref_len = [1 << 29, 1000]
    cases = {"refID >= n_ref": bamio.encode_record(2, 100, 0, 60, [50 << 4], b"b")[4:],
             "end > 2^29": bamio.encode_record(0, (1 << 29) - 10, 0, 60, [50 << 4], b"c")[4:],
             "end behind the reference": bamio.encode_record(1, 20000, 0, 60, [50 << 4], b"d")[4:]}
    for what, bad in cases.items():
        with pytest.raises(TbkError) as e:
            ctx.bam_encode_indexed(np.arange(2, dtype=np.uint32), [1.0, 1.0], [1, 1], [0, 0], ref_len, n_dev=0, host_records={0: ok, 1: bad})
        assert e.value.status == -1, what                           # TBK_EINVAL, raised by the kernels' bounds checks
        run, _, part = ctx.bam_encode_indexed(np.arange(1, dtype=np.uint32), [1.0], [1], [0], ref_len, n_dev=0, host_records={0: ok})
        check_part(run, part, ref_len)
    with pytest.raises(TbkError) as e:                               # refIDs that decrease
        ctx.bam_encode_indexed(np.arange(2, dtype=np.uint32), [1.0, 1.0], [1, 1], [0, 0], ref_len, n_dev=0,
                               host_records={0: bamio.encode_record(1, 5, 0, 60, [50 << 4], b"e")[4:], 1: ok})
    assert e.value.status == -1
    with pytest.raises(TbkError):                                    # a reference a BAI cannot address
        ctx.bam_encode_indexed(np.arange(1, dtype=np.uint32), [1.0], [1], [0], [(1 << 29) + 1], n_dev=0, host_records={0: ok})


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _tiebrush(outdir, extra=(), env=None):
    """tiebrush -o o.bam ... on the ten t1 samples, run INSIDE outdir: the @PG line of the output header records the command line as typed,
    so two runs with the same options write the same header whatever their directories are"""
    os.makedirs(outdir, exist_ok=True)
    args = [os.path.join(BIN, "tiebrush"), "-o", "o.bam"] + list(extra) + sample_paths("t1")
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), cwd=outdir)
    return r, os.path.join(outdir, "o.bam")


def _split_header(data):
    """(header text, the file's bytes from the first member that holds records on)"""
    import struct
    mem = br.members(data)
    payload = b"".join(p for _, p in mem)
    l_text = struct.unpack_from("<I", payload, 4)[0]
    q = 8 + l_text
    n_ref = struct.unpack_from("<I", payload, q)[0]
    q += 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<I", payload, q)[0]
    done = 0
    for at, p in mem:                                   # (the header goes out in members of its own, ahead of the first record member)
        if done == q:
            return payload[8:8 + l_text].decode(), data[at:]
        done += len(p)
    raise AssertionError("the header does not end on a member boundary")


def same_bam_but_for_the_option(with_index, plain):
    """--index is part of the command line the @PG header line records: apart from that word the header texts are equal, and every byte from the
    first record member on — members, EOF member — is identical"""
    ta, ra = _split_header(with_index)
    tb, rb = _split_header(plain)
    assert ta.replace(" --index", "") == tb and ta != tb
    assert ra == rb


def _check_output(path, queries=False):
    data, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
    assert bai == br.expected_bai(data)
    br.validate(data, bai)
    if queries:
        br.region_checks(data, bai, seed=11, n_random=60)
    return data, bai


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """the outputs without --index, by writer: what --index must not change"""
    d = tmp_path_factory.mktemp("plain")
    out = {}
    for w in ("device", "host"):
        r, p = _tiebrush(str(d / w), ["--writer", w])
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(p + ".bai")
        out[w] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("writer", ["device", "host"])
def test_cli_index_by_writer(tmp_path, plain_runs, writer):
    r, p = _tiebrush(str(tmp_path), ["--writer", writer, "--index"])
    assert r.returncode == 0, r.stderr
    data, _ = _check_output(p, queries=True)
    same_bam_but_for_the_option(data, plain_runs[writer])


@pytest.mark.parametrize("route_env", [{"TBK_HYBRID": "1"}, {"TBK_DEVICE_DECODE": "1"}, {"TBK_HOST_FAST": "0", "TBK_DEVICE_DECODE": "0", "TBK_TILE_RECORDS": "2000"}],
                         ids=["hybrid", "device-decode", "streaming"])
def test_cli_index_on_the_other_routes(tmp_path, route_env):
    r, p = _tiebrush(str(tmp_path), ["--index"], env=route_env)
    assert r.returncode == 0, r.stderr
    _check_output(p)


@pytest.mark.parametrize("groups", [256, 100])
def test_cli_index_with_small_chunks(tmp_path, groups):
    """several parts from the two encode contexts; with 100 groups a chunk a run of one bin straddles parts"""
    r, p = _tiebrush(str(tmp_path / "chunked"), ["--index"], env={"TBK_DW_CHUNK_GROUPS": str(groups)})
    assert r.returncode == 0, r.stderr
    data, bai = _check_output(p)
    r, q = _tiebrush(str(tmp_path / "whole"), ["--index"])
    assert r.returncode == 0, r.stderr
    if data == open(q, "rb").read():                                 # (the chunking may cut other members: then the restatement of this file is the reference)
        assert bai == open(q + ".bai", "rb").read()


def test_cli_index_when_the_device_writer_refuses_a_chunk(tmp_path):
    r, p = _tiebrush(str(tmp_path), ["--index"], env={"TBK_DW_CHUNK_GROUPS": "256", "TBK_TEST_DW_REFUSE_CHUNK": "1", "TBK_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert "host writer" in r.stderr                                 # chunk 0 by the device, the rest by the host writer
    _check_output(p, queries=True)


def test_cli_index_with_tracks(tmp_path):
    opts = ["--cov", "t.cov", "--junc", "t.junc", "--samp", "t.samp"]   # (the coverage and the sample counts both end in .bedgraph: a prefix each)
    ra, a = _tiebrush(str(tmp_path / "a"), opts)
    rb, b = _tiebrush(str(tmp_path / "b"), opts + ["--index"])
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    data, _ = _check_output(b)
    same_bam_but_for_the_option(data, open(a, "rb").read())
    tracks = sorted(f for f in os.listdir(os.path.dirname(a)) if f.startswith("t."))
    assert tracks == ["t.cov.bedgraph", "t.junc.bed", "t.samp.bedgraph"]
    for t in tracks:
        assert open(os.path.join(os.path.dirname(a), t), "rb").read() == open(os.path.join(os.path.dirname(b), t), "rb").read(), t


def test_cli_index_refusals(tmp_path):
    r, p = _tiebrush(str(tmp_path), ["--ranks", "2", "--index"])
    assert r.returncode != 0 and "--index" in r.stderr and "--ranks" in r.stderr
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([os.path.join(BIN, "tiebrush"), "-o", "-", "--index"] + sample_paths("t1"), capture_output=True, cwd=str(tmp_path))
    assert r.returncode != 0 and b"--index" in r.stderr and r.stdout == b""
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([os.path.join(BIN, "tiebrush"), "-h"], capture_output=True, text=True)
    assert "--index" in r.stdout
