"""tbk_track_bgzf and `tiecov --tabix` / `tiebrush --tabix` on the MI355X.

The contract: the runs of tbk_track_bgzf, inflated, are tbk_format_track's bytes behind the header, in members cut every 0xff00 payload
bytes, and every run's index part is the restatement's (tbi_reader.expected_part) for that run; a command line's FILE.gz inflates to the
plain track of the same command line without --tabix, and its index is the restatement of its own bytes (tbi_reader.check_file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tbi_reader as tr
from helpers import GOLDEN, sample_paths

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")
T_RUN = 120
CUT = 0xff00


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _arr(rows):
    tid, st, en = (np.array([r[k] for r in rows], dtype=np.int32) for k in range(3))
    return tid, st, en


def _kind_args(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "cov":
        return dict(val=np.round(rng.random(n) * 50, 3))
    if kind == "junc":
        return dict(val=np.round(rng.random(n) * 50, 3), strand=rng.choice(np.frombuffer(b"+-.", dtype=np.uint8), n))
    return dict(count=rng.integers(0, 40, n, dtype=np.int64), heat=(rng.random(n) + 0.1).astype(np.float32))


def _check_part(got, want, where):
    if got is None:
        assert False, "no part"
    assert [tuple(int(x) for x in c) for c in got["chunks"]] == want["chunks"], where
    assert got["lin_first"] == want["lin_first"] and np.array_equal(got["lin"], want["lin"]), where
    assert [(int(r["tid"]), int(r["n_records"]), int(r["first"]), int(r["last"])) for r in got["refs"]] == want["refs"], where


def _check(ctx, kind, names, ref_len, rows, head=b"", depth=None, slices=(None, 4096, 1), seed=0, kw=None):
    """the library contract for one scene under every slice size (None: the default, one run; 4096 bytes; 1: one line a slice);
    returns the runs of the first"""
    tid, st, en = _arr(rows)
    kw = kw or _kind_args(kind, len(rows), seed)
    ctx.track_names(names)
    nb = [n.encode() for n in names]
    first = None
    for fs in slices:
        try:
            ctx.set_debug("" if fs is None else "fmt_slice=%d" % fs)
            text = ctx.format_track(kind, tid, st, en, **kw)
            runs = ctx.track_bgzf(kind, tid, st, en, head=head, ref_len=ref_len, csi_depth=depth, **kw)
        finally:
            ctx.set_debug("")
        assert b"".join(tr.inflate(run) for run, _ in runs) == head + text, fs
        assert ctx.last_track_bytes == (len(head) + len(text), sum(len(r) for r, _ in runs))
        if fs is None:
            assert len(runs) == 1
        if fs == 1:
            assert len(runs) == max(len(rows), 1)                    # one line a slice (the header rides with slice 0)
        for k, (run, part) in enumerate(runs):
            pays = [len(p) for _, p in tr.br.members(run)]
            assert all(x == CUT for x in pays[:-1]) and 0 < pays[-1] <= CUT, (fs, k)   # cut as bgzip cuts, the last one short, no EOF member
            _check_part(part, tr.expected_part(run, len(head) if k == 0 else 0, nb, ref_len, depth), (fs, k))
        first = first or runs
    return first


LENS = [1 << 29, 100000, 1 << 20]
NAMES = ["c", "chrEmpty", "chrOne"]


def test_lines_at_the_member_cuts(ctx):
    """every row its own leaf bin (its own chunk), lines of 28 bytes behind a header of 12: row 2330 ends exactly on the first cut, row
    2331 begins exactly on it, row 4662 straddles the second"""
    head = b"#track head\n"
    n = 7000
    rows = [(0, 100000000 + 16384 * i, 100000010 + 16384 * i) for i in range(n)]
    assert len(head) + 28 * 2331 == CUT and len(head) + 28 * 4662 < 2 * CUT < len(head) + 28 * 4663
    # (one line a slice has no cut to meet: the scene runs with the two slice sizes that have)
    runs = _check(ctx, "cov", NAMES, LENS, rows, head=head, slices=(None, 4096), kw=dict(val=np.ones(n)))
    run, part = runs[0]
    offs = [at for at, _ in tr.br.members(run)]
    beg = {int(c["beg"]) for c in part["chunks"]}
    assert offs[1] << 16 in beg                                      # row 2331: offset 0 of the second member
    assert (offs[0] << 16 | (CUT - 28)) in beg                       # row 2330: the last 28 bytes of the first
    assert (offs[1] << 16 | (CUT - 12)) in beg                       # row 4662: begins 12 bytes before the second cut


@pytest.mark.parametrize("kind", ["cov", "junc", "sample"])
def test_every_kind_and_a_header_longer_than_the_first_line(ctx, kind):
    rng = np.random.default_rng(5)
    st = np.sort(rng.integers(0, 900000, 3000))
    rows = [(0, int(s), int(s) + int(w)) for s, w in zip(st, rng.integers(0, 40000, 3000))] + [(2, 10, 10), (2, 500, 100000)]
    head = b"track " + b"x" * 200 + b"\n"
    _check(ctx, kind, NAMES, LENS, rows, head=head, seed=3, slices=(None, 4096))
    _check(ctx, kind, NAMES, LENS, rows[:150] + rows[-2:], head=head, seed=3, slices=(1,))   # (one line a slice: a run per row, fewer rows)
    _check(ctx, kind, NAMES, LENS, rows[:50], head=b"", slices=(None, 1))


def test_the_header_alone(ctx):
    ctx.track_names(NAMES)
    z = np.zeros(0, dtype=np.int32)
    head = b"track type=bedGraph\n"
    runs = ctx.track_bgzf("cov", z, z, z, val=np.zeros(0), head=head, ref_len=LENS)
    assert len(runs) == 1 and tr.inflate(runs[0][0]) == head
    p = runs[0][1]
    assert len(p["chunks"]) == 0 and len(p["lin"]) == 0 and len(p["refs"]) == 0
    assert ctx.track_bgzf("cov", z, z, z, val=np.zeros(0), ref_len=LENS) == []       # nothing at all: no run
    runs = ctx.track_bgzf("cov", z, z, z, val=np.zeros(0), head=head)                  # compressed only
    assert runs[0][1] is None and tr.inflate(runs[0][0]) == head


def test_one_bin_twice_with_its_parent_between(ctx):
    """100-200, 150-40000, 300-400: two runs of leaf bin 4681 with a record of bin 585 between them.  Inside one member the two chunks
    merge; with more than a member of parent-bin rows between them they do not"""
    runs = _check(ctx, "cov", NAMES, LENS, [(0, 100, 200), (0, 150, 40000), (0, 300, 400)])
    assert [(int(c["bin"])) for c in runs[0][1]["chunks"]] == [585, 4681]
    far = [(0, 100, 200)] + [(0, 150 + i, 40000) for i in range(3800)] + [(0, 4000, 4100)]
    runs = _check(ctx, "cov", NAMES, LENS, far, slices=(None, 4096))
    part = runs[0][1]
    leaf = [c for c in part["chunks"] if int(c["bin"]) == 4681]
    assert len(leaf) == 2 and int(leaf[0]["end"]) >> 16 < int(leaf[1]["beg"]) >> 16


def test_a_long_reference_name_takes_the_per_lane_path(ctx):
    names = ["n" * 1500, "chrEmpty", "chrOne"]
    rows = [(0, 1000 * i, 1000 * i + 700) for i in range(300)] + [(2, 5, 50)]
    _check(ctx, "cov", names, LENS, rows, head=b"track type=bedGraph\n", slices=(None, 4096))
    _check(ctx, "cov", names, LENS, rows[:40] + rows[-1:], head=b"track type=bedGraph\n", slices=(1,))


@pytest.mark.parametrize("depth,length", [(0, 16384), (1, 131072), (5, 1 << 29), (6, (1 << 31) - 1)])
def test_csi_depths(ctx, depth, length):
    edges = [1 << (14 + 3 * l) for l in range(depth)]
    rows = [(0, 10, 20), (0, 10, 10), (0, 300, 9000)] + [(0, e - 30, e + 30) for e in edges] + [(0, length - 100, length)]
    rows.sort(key=lambda r: r[1])
    runs = _check(ctx, "cov", ["only"], [length], rows, depth=depth, slices=(None, 1))
    bins = {int(c["bin"]) for c in runs[0][1]["chunks"]}
    assert (0 in bins) and len(bins) >= depth + 1


# ---- refusals: each is followed by a good call on the same context -----------------------------------------------------------------------
def _good(ctx):
    ctx.track_names(NAMES)
    _check(ctx, "cov", NAMES, LENS, [(0, 100, 200), (2, 5, 9)], head=b"h\n", slices=(None,))


REFUSED = [
    ("tid without a name", NAMES[:2], LENS, [(0, 1, 2), (2, 1, 2)], {}),
    ("tid >= n_ref", NAMES, LENS[:2], [(0, 1, 2), (2, 1, 2)], {}),
    ("negative tid", NAMES, LENS, [(-1, 1, 2)], {}),
    ("negative start", NAMES, LENS, [(0, -5, 2)], {}),
    ("end beyond 2^29", NAMES, LENS, [(0, 5, (1 << 29) + 1)], {}),
    ("end beyond the depth", NAMES, [100000, 100000, 100000], [(0, 5, (1 << 17) + 1)], dict(csi_depth=1)),
    ("end beyond its reference's last window", NAMES, LENS, [(1, 5, 120000)], {}),
    ("tid decreasing", NAMES, LENS, [(2, 1, 2), (0, 5, 6)], {}),
    ("start decreasing", NAMES, LENS, [(0, 10, 20), (0, 9, 30)], {}),
    ("a reference a BAI cannot address", NAMES, [(1 << 29) + 1, 5, 5], [(0, 1, 2)], {}),
    ("depth above 6", NAMES, LENS, [(0, 1, 2)], dict(csi_depth=7)),
]


@pytest.mark.parametrize("what,names,lens,rows,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(ctx, what, names, lens, rows, kw):
    from tiebrush_amd.api import TbkError
    ctx.track_names(names)
    tid, st, en = _arr(rows)
    for fs in ("", "fmt_slice=1"):                                    # (the order is checked across slices too)
        try:
            ctx.set_debug(fs)
            with pytest.raises(TbkError) as e:
                ctx.track_bgzf("cov", tid, st, en, val=np.ones(len(rows)), head=b"h\n", ref_len=lens, **kw)
        finally:
            ctx.set_debug("")
        assert e.value.status == -1, what                             # TBK_EINVAL
    _good(ctx)


def test_range_refusal_comes_before_the_first_run(ctx):
    from tiebrush_amd.api import TbkError
    ctx.track_names(NAMES)
    tid, st, en = _arr([(0, 10 * i, 10 * i + 5) for i in range(100)])
    val = np.ones(100)
    val[99] = float("inf")
    try:
        ctx.set_debug("fmt_slice=1")
        with pytest.raises(TbkError) as e:
            ctx.track_bgzf("cov", tid, st, en, val=val, head=b"h\n", ref_len=LENS)
    finally:
        ctx.set_debug("")
    assert e.value.status == -5 and e.value.n_runs == 0               # TBK_EUNSUPPORTED
    _good(ctx)


def test_a_sink_that_refuses_stops_the_call(ctx):
    from tiebrush_amd.api import TbkError
    ctx.track_names(NAMES)
    tid, st, en = _arr([(0, 10 * i, 10 * i + 5) for i in range(100)])
    try:
        ctx.set_debug("fmt_slice=1")
        with pytest.raises(TbkError) as e:
            ctx.track_bgzf("cov", tid, st, en, val=np.ones(100), ref_len=LENS, on_run=lambda run, part: True)
    finally:
        ctx.set_debug("")
    assert e.value.status == -1 and 1 <= e.value.n_runs <= 2
    _good(ctx)


def test_device_rows(ctx):
    import torch
    rows = [(0, 37 * i, 37 * i + 30) for i in range(5000)]
    tid, st, en = _arr(rows)
    val = np.round(np.random.default_rng(1).random(5000) * 9, 3)
    ctx.track_names(NAMES)
    want = ctx.track_bgzf("cov", tid, st, en, val=val, head=b"h\n", ref_len=LENS)
    dev = [torch.from_numpy(a).to("cuda:0") for a in (tid, st, en, val)]
    got = ctx.track_bgzf("cov", *dev[:3], val=dev[3], head=b"h\n", ref_len=LENS)
    assert [r for r, _ in got] == [r for r, _ in want]


# ---- the command lines ------------------------------------------------------------------------------------------------------------------
def _run(args, env=None):
    return subprocess.run(args, check=True, capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})))


def _read(p):
    with open(p, "rb") as f:
        return f.read()


TRACKS = [("c", ".bedgraph"), ("j", ".bed"), ("s", ".bedgraph")]


def _tiecov_pair(tmp_path, tag, bam, extra=(), env=None, writer="device"):
    """tiecov -c -j -s with and without --tabix: every .gz inflates to the plain track, every index is the restatement of its own file"""
    plain, tbx = str(tmp_path / (tag + "_p")), str(tmp_path / (tag + "_t"))
    opts = lambda pre: [x for o, _ in TRACKS for x in ("-" + o, pre + "." + o)]
    _run([os.path.join(BIN, "tiecov")] + list(extra) + opts(plain) + [bam])
    r = _run([os.path.join(BIN, "tiecov"), "--tabix"] + list(extra) + opts(tbx) + [bam], env=dict(TBK_TIMING="1", **(env or {})))
    assert r.stderr.count("tabix phase ms: writer %s" % writer) == 3, r.stderr
    out = {}
    for o, ext in TRACKS:
        gz, p = tbx + "." + o + ext + ".gz", _read(plain + "." + o + ext)
        assert not os.path.exists(tbx + "." + o + ext)               # no plain track beside the .gz
        ix = gz + (".csi" if os.path.exists(gz + ".csi") else ".tbi")
        assert not os.path.exists(ix + ".tmp")
        tr.check_file(_read(gz), _read(ix), p, seed=11, n_random=60)
        out[o] = (_read(gz), _read(ix), p)
    return out


def _indexed_copy(tmp_path, src, name):
    dst = str(tmp_path / name)
    with open(dst, "wb") as f:
        f.write(_read(src))
    _run([os.path.join(BIN, "tbh_tool"), "bai", dst])
    return dst


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    """a BAM whose coverage text exceeds two members: 7000 reads 120 apart, spliced reads for the junction track, two samples"""
    from tiebrush_amd import bamio
    d = tmp_path_factory.mktemp("crafted")
    names, lens = ["chr1", "chrEmpty", "chr2"], [1 << 20, 50000, 300000]
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens)) + "@CO\tSAMPLE:a\n@CO\tSAMPLE:b\n"
    M, N = 0, 3
    recs = []
    for i in range(7000):
        cig = [(50 << 4) | M] if i % 50 else [(20 << 4) | M, (300 << 4) | N, (30 << 4) | M]
        recs.append(bamio.encode_record(0, 1000 + 120 * i, 0, 60, cig, b"r%d" % i, aux=b"XSA+" + b"YXC" + bytes([1 + i % 2])))
    recs += [bamio.encode_record(2, 100 + 70 * i, 0, 60, [(40 << 4) | M], b"q%d" % i) for i in range(50)]
    path = str(d / "crafted.bam")
    bamio.write_bam(path, text, names, lens, b"".join(recs), level=6)
    _run([os.path.join(BIN, "tbh_tool"), "bai", path])
    return path


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tiecov_tabix_on_the_goldens(tmp_path, name):
    bam = os.path.join(GOLDEN, name, name + ".bam")
    dev = _tiecov_pair(tmp_path, "d", bam)
    host = _tiecov_pair(tmp_path, "h", bam, env=dict(TBK_TRACK_HOST_FMT="1"), writer="host")
    for o, _ in TRACKS:
        assert tr.inflate(dev[o][0]) == tr.inflate(host[o][0])


def test_tiecov_tabix_on_the_crafted_bam(tmp_path, crafted):
    dev = _tiecov_pair(tmp_path, "d", crafted)
    assert len(dev["c"][2]) > 2 * CUT and len(tr.br.members(dev["c"][0])) >= 4
    host = _tiecov_pair(tmp_path, "h", crafted, env=dict(TBK_TRACK_HOST_FMT="1"), writer="host")
    for o, _ in TRACKS:
        assert tr.inflate(dev[o][0]) == tr.inflate(host[o][0])
    ix = tr.parse(dev["c"][1])
    assert ix["names"] == [b"chr1", b"chr2"] and ix["skip"] == 1


def test_runs_of_one_bin_across_slice_boundaries(tmp_path, crafted):
    """slices of a few lines: the runs of one bin straddle the slice boundaries and come together again in the combiner (BaiIndex::add),
    for the device's runs and for the host path's"""
    small = _tiecov_pair(tmp_path, "s", crafted, env=dict(TBK_DEBUG="fmt_slice=4096"))
    hsmall = _tiecov_pair(tmp_path, "hs", crafted, env=dict(TBK_DEBUG="fmt_slice=4096", TBK_TRACK_HOST_FMT="1"), writer="host")
    for o, _ in TRACKS:
        assert tr.inflate(small[o][0]) == tr.inflate(hsmall[o][0])
    n_mem = len(tr.br.members(small["c"][0]))
    assert n_mem > 30 and n_mem > 5 * (len(small["c"][2]) // CUT + 1)            # a short member per slice
    one_bin = max(len(ch) for R in tr.parse(small["c"][1])["refs"] for _, ch in R["bins"].values())
    assert one_bin < n_mem // 2                                                   # the chunks did come together


def test_tiecov_tabix_under_regions(tmp_path, crafted):
    _tiecov_pair(tmp_path, "r", crafted, extra=["-r", "chr1:100,000-400,000"])
    _tiecov_pair(tmp_path, "rh", crafted, extra=["-r", "chr1:100,000-400,000"], env=dict(TBK_TRACK_HOST_FMT="1"), writer="host")
    bed = tmp_path / "u.bed"
    bed.write_text("chr1\t5000\t90000\nchr1\t200000\t260000\nchr2\t0\t2000\n")
    got = _tiecov_pair(tmp_path, "R", crafted, extra=["-R", str(bed)])
    assert tr.parse(got["c"][1])["names"] == [b"chr1", b"chr2"]
    t1 = _indexed_copy(tmp_path, os.path.join(GOLDEN, "t1", "t1.bam"), "t1.bam")
    first = _read(os.path.join(GOLDEN, "t1", "t1.coverage.bedgraph")).split(b"\n")[1].split(b"\t")
    reg = "%s:%d-%d" % (first[0].decode(), int(first[1]) + 1, int(first[1]) + 3000)
    _tiecov_pair(tmp_path, "g", t1, extra=["-r", reg])


def test_tiecov_tabix_with_bigwig_keeps_the_bigwig(tmp_path, crafted):
    pre, ref = str(tmp_path / "w"), str(tmp_path / "p")
    _run([os.path.join(BIN, "tiecov"), "-W", "-c", ref, "-j", ref, "-s", ref + "s", crafted])
    _run([os.path.join(BIN, "tiecov"), "--tabix", "-W", "-c", pre, "-j", pre, "-s", pre + "s", crafted])
    assert _read(pre + ".bigwig") == _read(ref + ".bigwig")
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("w")) == ["w.bed.gz", "w.bed.gz.tbi", "w.bigwig", "ws.bedgraph.gz", "ws.bedgraph.gz.tbi"]
    tr.check_file(_read(pre + ".bed.gz"), _read(pre + ".bed.gz.tbi"), _read(ref + ".bed"))
    tr.check_file(_read(pre + "s.bedgraph.gz"), _read(pre + "s.bedgraph.gz.tbi"), _read(ref + "s.bedgraph"))


def test_older_files_go_before_the_run(tmp_path, crafted):
    pre = str(tmp_path / "o")
    for stale in (".bedgraph.gz", ".bedgraph.gz.tbi", ".bedgraph.gz.csi"):
        with open(pre + stale, "wb") as f:
            f.write(b"stale")
    _run([os.path.join(BIN, "tiecov"), "--tabix", "-c", pre, crafted])
    assert not os.path.exists(pre + ".bedgraph.gz.csi")
    _run([os.path.join(BIN, "tiecov"), "-c", pre, crafted])
    tr.check_file(_read(pre + ".bedgraph.gz"), _read(pre + ".bedgraph.gz.tbi"), _read(pre + ".bedgraph"))


def _header_and_records(data):
    """(header text, the file's bytes from the first member that holds records on): the header goes out in members of its own"""
    mem = tr.br.members(data)
    payload = b"".join(p for _, p in mem)
    l_text = struct.unpack_from("<I", payload, 4)[0]
    q = 8 + l_text
    n_ref = struct.unpack_from("<I", payload, q)[0]
    q += 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<I", payload, q)[0]
    done = 0
    for at, p in mem:
        if done == q:
            return payload[8:8 + l_text].decode(), data[at:]
        done += len(p)
    raise AssertionError("the header does not end on a member boundary")


@pytest.mark.parametrize("name,env,writer", [("t1", {}, "device"), ("t2", {}, "device"), ("t1", dict(TBK_TRACK_HOST_FMT="1"), "host")])
def test_tiebrush_tabix(tmp_path, name, env, writer):
    """the runs are made INSIDE their directories with the same relative names: the @PG line of the output header records the command
    line as typed, so the two BAMs differ in the word --tabix there and nowhere else"""
    paths = sample_paths(name)
    tracks = ["--cov", "c", "--junc", "j", "--samp", "s", "-o", "o.bam"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    run = lambda args, d, e: subprocess.run([os.path.join(BIN, "tiebrush")] + args + paths, check=True, capture_output=True, text=True, timeout=T_RUN,
                                            env=dict(os.environ, **e), cwd=str(d))
    run(tracks, a, env)
    r = run(tracks + ["--tabix"], b, dict(TBK_TIMING="1", **env))
    ta, ra = _header_and_records(_read(str(a / "o.bam")))
    tb, rb = _header_and_records(_read(str(b / "o.bam")))
    assert tb.replace(" --tabix", "") == ta and ta != tb and ra == rb
    assert r.stderr.count("tabix phase ms: writer %s" % writer) == 3, r.stderr
    for o, ext in TRACKS:
        gz = str(b / (o + ext + ".gz"))
        assert not os.path.exists(str(b / (o + ext)))
        tr.check_file(_read(gz), _read(gz + ".tbi"), _read(str(a / (o + ext))), seed=13, n_random=60)


def test_a_long_reference_gets_a_csi(tmp_path):
    from tiebrush_amd import bamio
    names, lens = ["chrLong", "chrB"], [(1 << 29) + 70000, 1000]
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens))
    pos = [100, 5000, (1 << 29) - 20, (1 << 29) + 100, (1 << 29) + 60000]
    recs = [bamio.encode_record(0, p, 0, 60, [(50 << 4)], b"r%d" % i) for i, p in enumerate(pos)] + [bamio.encode_record(1, 10, 0, 60, [(50 << 4)], b"x")]
    bam = str(tmp_path / "l.bam")
    bamio.write_bam(bam, text, names, lens, b"".join(recs), level=6)
    pre = str(tmp_path / "l")
    _run([os.path.join(BIN, "tiecov"), "-c", pre, bam])
    for env in ({}, dict(TBK_TRACK_HOST_FMT="1")):
        _run([os.path.join(BIN, "tiecov"), "--tabix", "-c", pre, bam], env=env)
        assert not os.path.exists(pre + ".bedgraph.gz.tbi")
        gz, csi = _read(pre + ".bedgraph.gz"), _read(pre + ".bedgraph.gz.csi")
        tr.check_file(gz, csi, _read(pre + ".bedgraph"))
        assert tr.parse(csi)["depth"] == 6
        assert len(tr.query(gz, csi, b"chrLong", (1 << 29) + 50, (1 << 29) + 200)) == 1
