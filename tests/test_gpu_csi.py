"""`tiebrush --csi` and tbk_bam_encode_indexed with a CSI depth (baix.hip): the index part of every encoded run and the .csi of every route's
output against the restatement of the CSI contract in csi_reader.py, exactly — references up to 2^31 - 1 included."""
import os
import subprocess

import numpy as np
import pytest

import bai_reader as br
import csi_reader as cr
from helpers import GOLDEN, sample_paths
from test_gpu_encode import _golden_case
from test_gpu_index import _split_header, _tiebrush

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


def _chunks(part):
    return [tuple(int(x) for x in c) for c in part["chunks"][["tid", "bin", "beg", "end"]].tolist()]


def check_part(run, part, ref_len, depth):
    want = cr.expected_part(run, ref_len, depth)
    assert np.array_equal(part["rec_vbeg"], want["rec_vbeg"])
    assert _chunks(part) == want["chunks"]
    assert part["lin_first"] == want["lin_first"] and np.array_equal(part["lin"], want["lin"])
    assert [tuple(int(x) for x in r) for r in part["refs"][["tid", "n_records", "first", "last"]].tolist()] == want["refs"]


def same_parts(a, b):
    assert _chunks(a) == _chunks(b) and a["lin_first"] == b["lin_first"]
    for k in ("lin", "refs", "rec_vbeg"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", ["t1", "t2", "t12"])
def test_library_depth_5_equals_the_bai_part_on_goldens(ctx, golden_ref_len, case):
    if case == "t12":
        names, tb = ["t1/t1.bam", "t2/t2.bam"], [1, 1]
    else:
        names, tb = [os.path.relpath(p, GOLDEN) for p in sample_paths(case)], [0] * 10
    assert cr.depth_for(golden_ref_len) == 5
    s, rep, yc, yx, yd = _golden_case(ctx, names, tb, keep_results=True)
    n_dev, m = int(s.n_records), len(rep)
    blob, off = ctx.bam_records(rep)
    recs = {i: blob[int(off[i]) + 4:int(off[i + 1])] for i in range(m)}
    half = n_dev // 2
    for nd, host in ((n_dev, None), (0, recs), (half, {i: r for i, r in recs.items() if rep[i] >= half})):   # the three hand-over forms
        want, pay, bai_part = ctx.bam_encode_indexed(rep, yc, yx, yd, golden_ref_len, n_dev=nd, host_records=host)
        run, pay_c, part = ctx.bam_encode_indexed(rep, yc, yx, yd, golden_ref_len, n_dev=nd, host_records=host, csi_depth=5)
        assert run == want and pay_c == pay
        same_parts(part, bai_part)
        check_part(run, part, golden_ref_len, 5)
    a, b = 7, m - 11                                                 # TBK_MEM_KEPT, a range that does not start at group 0
    want, _, bai_part = ctx.bam_encode_indexed(rep[a:b], None, None, None, golden_ref_len, n_dev=n_dev, kept_first=a)
    run, _, part = ctx.bam_encode_indexed(rep[a:b], None, None, None, golden_ref_len, n_dev=n_dev, kept_first=a, csi_depth=5)
    assert run == want
    same_parts(part, bai_part)
    check_part(run, part, golden_ref_len, 5)
    ctx.bam_release()


def _encode_host(ctx, recs, ref_len, depth):
    n = len(recs)
    yc, yx, yd = np.ones(n), np.arange(n) % 300, np.arange(n) % 3
    return ctx.bam_encode_indexed(np.arange(n, dtype=np.uint32), yc, yx, yd, ref_len, n_dev=0, host_records=dict(enumerate(recs)), csi_depth=depth)


def test_library_part_on_the_long_records(ctx):
    """depth 6, a reference of 2^31 - 1: leaf bins from 37449 to 168520, so most bins need more than 16 bits of the run sort's key"""
    recs = [r[4:] for r in cr.long_records()]
    run, _, part = _encode_host(ctx, recs, cr.LONG_LENS, 6)
    assert len(br.members(run)) >= 9
    check_part(run, part, cr.LONG_LENS, 6)
    ch = _chunks(part)
    high = [c for c in ch if c[1] >= 1 << 16]
    assert len(high) >= 20 and high == sorted(high, key=lambda c: c[:3])   # ascending (tid, bin, beg) above 2^16: the sort mask
    assert ch == sorted(ch, key=lambda c: c[:3])
    assert max(c[1] for c in ch if c[0] == 0) == cr.LONG_LAST_LEAF
    assert [c[1] for c in ch if c[0] == 2] == [0]                    # across 2^29 on the last reference: bin 0
    assert [int(t) for t in part["refs"]["tid"]] == [0, 2]
    assert len(part["lin"]) == (1 << 17) + 7 + (1 << 15) + 1         # the whole of reference 0, the empty one, up to 2^29 + 40 on the last


@pytest.mark.parametrize("ref_len,depth", [(10000, 0), (100000, 1)])
def test_library_depth_0_and_1(ctx, ref_len, depth):
    recs = [r[4:] for r in cr.small_records(ref_len)]
    run, _, part = _encode_host(ctx, recs, [ref_len], depth)
    check_part(run, part, [ref_len], depth)
    assert set(cr.bin_level(c[1], depth) for c in _chunks(part)) == set(range(depth + 1))
    assert all(c[1] < cr.meta_bin(depth) - 1 for c in _chunks(part))


def test_library_refusals_leave_the_context_usable(ctx):
    from tiebrush_amd import bamio
    from tiebrush_amd.api import TbkError
    ok = bamio.encode_record(0, 100, 0, 60, [50 << 4], b"a")[4:]
    plain = bamio.encode_record(0, 0, 0, 60, [50 << 4], b"b")
    two = np.arange(2, dtype=np.uint32)
    cases = {"depth 7": (7, [1000], ok),
             "a reference longer than depth 5 addresses": (5, [(1 << 29) + 1], ok),
             "end behind the reference's last window": (6, [1 << 30, 1000], cr.moved(plain, 1, 20000)[4:]),
             "end behind what depth 1 addresses": (1, [1 << 17], cr.moved(plain, 0, (1 << 17) - 10)[4:]),
             "refID outside the header": (6, [1 << 30, 1000], cr.moved(plain, 2, 100)[4:])}
    for what, (depth, ref_len, bad) in cases.items():
        with pytest.raises(TbkError) as e:
            ctx.bam_encode_indexed(two, [1.0, 1.0], [1, 1], [0, 0], ref_len, n_dev=0, host_records={0: ok, 1: bad}, csi_depth=depth)
        assert e.value.status == -1, what                           # TBK_EINVAL
        run, _, part = ctx.bam_encode_indexed(two[:1], [1.0], [1], [0], [1 << 30, 1000], n_dev=0, host_records={0: ok}, csi_depth=6)
        check_part(run, part, [1 << 30, 1000], 6)
    with pytest.raises(TbkError) as e:                               # without a depth: the BAI's refusal, as before
        ctx.bam_encode_indexed(two[:1], [1.0], [1], [0], [(1 << 29) + 1], n_dev=0, host_records={0: ok})
    assert e.value.status == -1
    run, _, part = ctx.bam_encode_indexed(two[:1], [1.0], [1], [0], [(1 << 29) + 1], n_dev=0, host_records={0: ok}, csi_depth=6)
    check_part(run, part, [(1 << 29) + 1], 6)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def same_bam_but_for_the_option(with_csi, plain):
    """test_gpu_index.same_bam_but_for_the_option for --csi: the @PG line records the command line, so apart from that word the header texts
    are equal, and every byte from the first record member on is identical"""
    ta, ra = _split_header(with_csi)
    tb, rb = _split_header(plain)
    assert ta.replace(" --csi", "") == tb and ta != tb
    assert ra == rb


def _check_output(path, queries=False):
    data, csi = open(path, "rb").read(), open(path + ".csi", "rb").read()
    assert cr.inflate(csi) == cr.expected_csi(data)
    assert sorted(os.listdir(os.path.dirname(path))) == ["o.bam", "o.bam.csi"]   # no .bai, no temporary file
    if queries:
        cr.validate(data, csi)
        cr.region_checks(data, csi, seed=11, n_random=60)
    return data, csi


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """the outputs without the option, by writer: what --csi must not change"""
    d = tmp_path_factory.mktemp("plain_csi")
    out = {}
    for w in ("device", "host"):
        r, p = _tiebrush(str(d / w), ["--writer", w])
        assert r.returncode == 0, r.stderr
        assert os.listdir(str(d / w)) == ["o.bam"]
        out[w] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("writer", ["device", "host"])
def test_cli_csi_by_writer(tmp_path, plain_runs, writer):
    r, p = _tiebrush(str(tmp_path), ["--writer", writer, "--csi"])
    assert r.returncode == 0, r.stderr
    data, _ = _check_output(p, queries=True)
    same_bam_but_for_the_option(data, plain_runs[writer])


@pytest.mark.parametrize("route_env", [{"TBK_HYBRID": "1"}, {"TBK_DEVICE_DECODE": "1"}, {"TBK_HOST_FAST": "0", "TBK_DEVICE_DECODE": "0", "TBK_TILE_RECORDS": "2000"}],
                         ids=["hybrid", "device-decode", "streaming"])
def test_cli_csi_on_the_other_routes(tmp_path, route_env):
    r, p = _tiebrush(str(tmp_path), ["--csi"], env=route_env)
    assert r.returncode == 0, r.stderr
    _check_output(p)


@pytest.mark.parametrize("groups", [256, 100])
def test_cli_csi_with_small_chunks(tmp_path, groups):
    """several parts from the two encode contexts; with 100 groups a chunk a run of one bin straddles parts"""
    r, p = _tiebrush(str(tmp_path), ["--csi"], env={"TBK_DW_CHUNK_GROUPS": str(groups)})
    assert r.returncode == 0, r.stderr
    _check_output(p)


def test_cli_csi_when_the_device_writer_refuses_a_chunk(tmp_path):
    r, p = _tiebrush(str(tmp_path), ["--csi"], env={"TBK_DW_CHUNK_GROUPS": "256", "TBK_TEST_DW_REFUSE_CHUNK": "1", "TBK_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert "host writer" in r.stderr                                 # chunk 0 by the device, the rest by the host writer
    _check_output(p)


def test_cli_csi_with_tracks(tmp_path):
    opts = ["--cov", "t.cov", "--junc", "t.junc", "--samp", "t.samp"]
    ra, a = _tiebrush(str(tmp_path / "a"), opts)
    rb, b = _tiebrush(str(tmp_path / "b"), opts + ["--csi"])
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    data, csi = open(b, "rb").read(), open(b + ".csi", "rb").read()
    assert cr.inflate(csi) == cr.expected_csi(data)
    same_bam_but_for_the_option(data, open(a, "rb").read())
    tracks = ["t.cov.bedgraph", "t.junc.bed", "t.samp.bedgraph"]
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["o.bam", "o.bam.csi"] + tracks
    for t in tracks:
        assert open(os.path.join(os.path.dirname(a), t), "rb").read() == open(os.path.join(os.path.dirname(b), t), "rb").read(), t


@pytest.fixture(scope="module")
def long_inputs(tmp_path_factory):
    """three coordinate-sorted inputs cut from the long records: record i goes to file i % 3"""
    d = tmp_path_factory.mktemp("long_in")
    recs = cr.long_records()
    paths = []
    for k in range(3):
        paths.append(str(d / ("in%d.bam" % k)))
        cr.write_bam(paths[-1], cr.LONG_NAMES, cr.LONG_LENS, recs[k::3])
    return paths


@pytest.mark.parametrize("writer", ["device", "host"])
def test_cli_csi_on_references_beyond_2_29(tmp_path, long_inputs, writer):
    tool = os.path.join(BIN, "tiebrush")
    r = subprocess.run([tool, "-o", "o.bam", "--writer", writer, "--index"] + long_inputs, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "chrLong" in r.stderr and "--index" in r.stderr
    assert os.listdir(str(tmp_path)) == []                           # refused before the output is created
    r = subprocess.run([tool, "-o", "o.bam", "--writer", writer, "--csi"] + long_inputs, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    data, csi = _check_output(str(tmp_path / "o.bam"), queries=True)
    _, lens, recs, _ = br.read_bam(data)
    assert lens == cr.LONG_LENS and len(recs) > 5000
    depth, refs, _ = cr.parse_csi(csi)
    assert depth == 6 and refs[1] == [] and [b for b, _, _ in refs[2]] == [0, cr.meta_bin(6)]
    assert [b for b, _, _ in refs[0]][-2:] == [cr.LONG_LAST_LEAF, cr.meta_bin(6)]
    top = (1 << 31) - 1
    for region in ((0, (3 << 29) - 50, (3 << 29) + 50), (0, top - 1, top), (0, 1 << 30, top), (2, (1 << 29) - 5, (1 << 29) + 1), (2, 1 << 29, (1 << 29) + 1)):
        got = cr.query(data, csi, *region)
        assert got and got == br.brute(recs, *region), region


def test_cli_csi_refusals(tmp_path):
    tool = os.path.join(BIN, "tiebrush")
    r, _ = _tiebrush(str(tmp_path), ["--csi", "--index"])
    assert r.returncode != 0 and "--csi" in r.stderr and "--index" in r.stderr
    assert os.listdir(str(tmp_path)) == []
    r, _ = _tiebrush(str(tmp_path), ["--ranks", "2", "--csi"])
    assert r.returncode != 0 and "--csi" in r.stderr and "--ranks" in r.stderr
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([tool, "-o", "-", "--csi"] + sample_paths("t1"), capture_output=True, cwd=str(tmp_path))
    assert r.returncode != 0 and b"--csi" in r.stderr and b"-o -" in r.stderr and r.stdout == b""
    assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([tool, "-h"], capture_output=True, text=True)
    assert "--csi" in r.stdout and "--index" in r.stdout
