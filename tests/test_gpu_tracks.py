"""`tiebrush --cov / --junc / --samp / --bigwig` and the device formatter (tbk_format_track) on the MI355X.

The contract: every track file is byte for byte what `tiecov -c / -j / -s` writes when it reads the BAM that the same tiebrush run wrote,
for every route and writer.  The formatter prints what glibc's printf prints, checked against Python's % formatting (correctly rounded
as well)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, sample_paths, read_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")
T_RUN = 300  # seconds a command line may take


def _run(args, env=None):
    return subprocess.run(args, check=True, capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, **(env or {})))


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _fused_vs_tiecov(tmp_path, tag, paths, flags=(), env=None, samp=True):
    """tiebrush with the three tracks, then tiecov on its BAM: the same bytes in every track file"""
    out = str(tmp_path / (tag + ".bam"))
    pre, ref = str(tmp_path / (tag + "_f")), str(tmp_path / (tag + "_r"))
    tr = ["--cov", pre + ".cov", "--junc", pre + ".junc"] + (["--samp", pre + ".samp"] if samp else [])
    r = _run([os.path.join(BIN, "tiebrush")] + list(flags) + tr + ["-o", out] + list(paths), env=env)
    _run([os.path.join(BIN, "tiecov"), "-c", ref + ".cov", "-j", ref + ".junc"] + (["-s", ref + ".samp"] if samp else []) + [out])
    files = [".cov.bedgraph", ".junc.bed"] + ([".samp.bedgraph"] if samp else [])
    for suf in files:
        a, b = _read(pre + suf), _read(ref + suf)
        assert a == b, (tag, suf, len(a), len(b))
    return r, out, {suf: _read(pre + suf) for suf in files}


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_fused_tracks_on_the_golden_samples(tmp_path, name):
    """fails without the feature: --cov is an unknown option there"""
    _, _, got = _fused_vs_tiecov(tmp_path, name, sample_paths(name), flags=["-A"])
    # ... and the reference's golden tracks under test_tiecov_cli's normalisation (values printed with .000 there)
    def norm(text, col):
        out = []
        for ln in text.decode().splitlines():
            f = ln.split("\t")
            if len(f) > col:
                assert f[col].endswith(".000"), ln
                f[col] = f[col][:-4]
            out.append("\t".join(f))
        return out
    assert norm(got[".cov.bedgraph"], 3) == read_lines(os.path.join(GOLDEN, name, name + ".coverage.bedgraph"))
    assert norm(got[".junc.bed"], 4) == read_lines(os.path.join(GOLDEN, name, name + ".junctions.bed"))
    ours = got[".samp.bedgraph"].decode().splitlines()
    gold = read_lines(os.path.join(GOLDEN, name, name + ".sample.bedgraph"))
    assert ours[0] == gold[0]
    assert ["\t".join(ln.split("\t")[:4]) for ln in ours[1:]] == ["\t".join(ln.split("\t")[:4]) for ln in gold[1:]]


ROUTES = [("whole", {}), ("stream", dict(TBK_HOST_FAST="0")), ("tiles", dict(TBK_TILE_RECORDS="5000")), ("tiny_tiles", dict(TBK_TILE_RECORDS="3")),
          ("device", dict(TBK_DEVICE_DECODE="1")), ("hybrid", dict(TBK_HYBRID="1")), ("whole_nomem", dict(TBK_TEST_WHOLE_ENOMEM="1")),
          ("device_nomem", dict(TBK_DEVICE_DECODE="1", TBK_TEST_WHOLE_ENOMEM="1")), ("hybrid_nomem", dict(TBK_HYBRID="1", TBK_TEST_WHOLE_ENOMEM="1"))]


@pytest.mark.parametrize("inputs", ["plain", "merged"])
def test_routes_and_writers_give_tiecov_tracks(tmp_path, inputs):
    """every route x both writers; the merged set carries TieBrush inputs with integer YC (the written value stays stale)"""
    paths = sample_paths("t2") if inputs == "plain" else [os.path.join(GOLDEN, "t1", "t1.bam"), os.path.join(GOLDEN, "t2", "t2.bam")] + sample_paths("t1")[:2]
    first = None
    for tag, env in ROUTES:
        for writer in ("device", "host"):
            r, _, got = _fused_vs_tiecov(tmp_path, "%s_%s_%s" % (inputs, tag, writer), paths, flags=["--writer", writer], env=dict(TBK_TIMING="1", **env))
            if tag == "whole":
                assert "host path ms" in r.stderr
            if tag.endswith("nomem"):
                assert "not used" in r.stderr or "given up" in r.stderr, r.stderr
            assert "tracks ms:" in r.stderr
            first = first or got
            assert got == first, (tag, writer)   # (the output records are the same on every route: so are the tracks)


def test_tiny_tiles_keep_the_tracks_exact(tmp_path):
    """tiles of a few records on synthetic inputs with long introns: the tracks of the streamed run equal the one-tile run's"""
    from tiebrush_amd import synth
    tile = synth.make_tile(4, 3000, "c2", n_loci=40)
    paths = synth.write_bams(tile, str(tmp_path / "in"))
    _, _, whole = _fused_vs_tiecov(tmp_path, "whole", paths)
    for k in ("3", "17", "400"):
        _, _, tiled = _fused_vs_tiecov(tmp_path, "tiles" + k, paths, env=dict(TBK_TILE_RECORDS=k))
        assert tiled == whole, k


@pytest.mark.parametrize("profile,flags", [("c5", ["-P"]), ("c5", ["-E", "-N", "5", "-Q", "1"]), ("c5", ["--keep-secondary", "-S", "--store-frac"])])
def test_options_on_synthetic_bams(tmp_path, profile, flags):
    from tiebrush_amd import synth
    tile = synth.make_tile(3, 4000, profile, n_loci=60)
    paths = synth.write_bams(tile, str(tmp_path / "in"))
    _, _, got = _fused_vs_tiecov(tmp_path, "o", paths, flags=flags)
    if "--store-frac" in flags:
        vals = {ln.split("\t")[3] for ln in got[".cov.bedgraph"].decode().splitlines()[1:]}
        assert any(not v.endswith(".000") for v in vals)   # fractional YC reached the text


def test_an_output_larger_than_the_readers_first_window(tmp_path):
    """an output of many megabytes: tiecov decodes all of it (its reader opens the header only and inflates records on demand), and
    the fused tracks equal that"""
    import torch
    from tiebrush_amd import synth, synth_dev
    tile = synth_dev.tile_to_host(synth_dev.make_tile_device(4, 250000, "c2", device="cuda:0"))
    torch.cuda.empty_cache()
    paths = synth.write_bams_fast(tile, str(tmp_path / "in"), seq=True)
    _, out, got = _fused_vs_tiecov(tmp_path, "big", paths, env=dict(TBK_TIMING="1"))
    assert os.path.getsize(out) > (8 << 20)
    assert got[".junc.bed"].count(b"\n") > 10000


def test_host_formatter_fallback_gives_the_same_bytes(tmp_path):
    _, _, dev = _fused_vs_tiecov(tmp_path, "dev", sample_paths("t1"))
    _, _, host = _fused_vs_tiecov(tmp_path, "host", sample_paths("t1"), env=dict(TBK_TRACK_HOST_FMT="1"))
    assert dev == host


def test_bigwig_matches_tiecov(tmp_path):
    out = str(tmp_path / "o.bam")
    _run([os.path.join(BIN, "tiebrush"), "--cov", str(tmp_path / "f"), "--bigwig", "-o", out] + sample_paths("t1"))
    _run([os.path.join(BIN, "tiecov"), "-W", "-c", str(tmp_path / "r"), out])
    assert not os.path.exists(str(tmp_path / "f.bedgraph"))
    assert _read(str(tmp_path / "f.bigwig")) == _read(str(tmp_path / "r.bigwig"))


def test_coverage_to_stdout(tmp_path):
    out = str(tmp_path / "o.bam")
    r = _run([os.path.join(BIN, "tiebrush"), "--cov", "-", "-o", out] + sample_paths("t2"))
    ref = _run([os.path.join(BIN, "tiecov"), "-c", "stdout", out])
    assert r.stdout == ref.stdout and r.stdout.startswith("chr")   # (no header line on standard output, as in tiecov)


# ---- the formatter through the Python API ---------------------------------------------------------------------------------------------

def _i32(x):
    return ((int(x) + 2**31) % 2**32) - 2**31


def _want(kind, names, tid, st, en, val=None, strand=None, count=None, heat=None, first=1):
    if kind == "cov":
        return "".join("%s\t%d\t%d\t%.3f\n" % (names[tid[i]], st[i], en[i], val[i]) for i in range(len(tid))).encode()
    if kind == "junc":
        return "".join("%s\t%d\t%d\tJUNC%08d\t%.3f\t%c\n" % (names[tid[i]], st[i], en[i], _i32(first + i), val[i], chr(strand[i]))
                       for i in range(len(tid))).encode()
    return "".join("%s\t%d\t%d\t%d\t%f\n" % (names[tid[i]], st[i], en[i], count[i], float(heat[i])) for i in range(len(tid))).encode()


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _values(rng):
    v = [0.0, -0.0, 1.0, -1.0, 0.0005, -0.0005, 0.0015, 0.0625, -0.0625, 2.5e-4, 1e-300, 5e-324, -5e-324, 999.9995, 9.9995, 0.9995,
         2.0**53, 2.0**53 - 1, 2.0**62, -(2.0**62), 9.2e18, 123456789.0005, -0.0001]
    v += [k / 16 for k in range(-64, 65)] + [k / 2**11 for k in range(0, 4096, 7)]
    for c in (0.9995, 9.9995, 99.9995, 999.9995, 1.0005, 0.0005, 12.3445):   # the neighbours of a carry / a tie
        x = c
        for _ in range(3):
            x = np.nextafter(x, 0)
        for _ in range(7):
            v.append(float(x))
            x = np.nextafter(x, 2 * c)
    v += list(rng.integers(-2**53, 2**53, 300).astype(np.float64))
    v += list(rng.standard_normal(2000) * 10.0 ** rng.integers(-8, 16, 2000))
    v += list(rng.random(2000) * 1000)
    return np.array(v, dtype=np.float64)


def test_formatter_matches_printf(ctx):
    rng = np.random.default_rng(7)
    names = ["chr1", "chrX", "scaffold_" + "n" * 1500, "", "chrUn_KI270302v1"]
    ctx.track_names(names)
    val = _values(rng)
    n = len(val)
    tid = rng.integers(0, len(names), n).astype(np.int32)
    st = rng.integers(-2**31, 2**31, n).astype(np.int32)
    en = rng.integers(-2**31, 2**31, n).astype(np.int32)
    st[:4] = [-2**31, 2**31 - 1, 0, -1]
    strand = rng.choice(np.frombuffer(b"+-.", dtype=np.uint8), n)
    got = ctx.format_track("cov", tid, st, en, val=val)
    assert got == _want("cov", names, tid, st, en, val=val)
    for first in (1, 10**8 - 5, 2**31 - 10):
        got = ctx.format_track("junc", tid, st, en, val=val, strand=strand, first_junc=first)
        assert got == _want("junc", names, tid, st, en, val=val, strand=strand, first=first), first
    count = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    count[:3] = [0, -2**63, 2**63 - 1]
    heat = np.concatenate([(rng.random(n // 2) * 1.4 + 0.1), rng.standard_normal(n - n // 2) * 1e6]).astype(np.float32)
    heat[:4] = [0.1, 1.5, -0.0, 0.0000005]
    got = ctx.format_track("sample", tid, st, en, count=count, heat=heat)
    assert got == _want("sample", names, tid, st, en, count=count, heat=heat)


def test_formatter_on_device_rows_and_small_slices(ctx):
    import torch
    rng = np.random.default_rng(11)
    names = ["c%d" % i for i in range(30)] + ["long" * 400]
    ctx.track_names(names)
    n = 50000
    tid = rng.integers(0, len(names), n).astype(np.int32)
    st = rng.integers(0, 10**9, n).astype(np.int32)
    en = (st + rng.integers(1, 1000, n)).astype(np.int32)
    val = np.round(rng.random(n) * 100, 4)
    want = _want("cov", names, tid, st, en, val=val)
    dev = [torch.from_numpy(a).to("cuda:0") for a in (tid, st, en, val)]
    assert ctx.format_track("cov", *dev[:3], val=dev[3]) == want
    try:
        ctx.set_debug("fmt_slice=4096")   # many slices through the two staging buffers
        assert ctx.format_track("cov", tid, st, en, val=val) == want
        ctx.set_debug("fmt_slice=1")      # one line a slice
        assert ctx.format_track("cov", tid[:3000], st[:3000], en[:3000], val=val[:3000]) == want[:len(_want("cov", names, tid[:3000], st[:3000], en[:3000], val=val[:3000]))]
    finally:
        ctx.set_debug("")
    assert ctx.format_track("cov", tid[:0], st[:0], en[:0], val=val[:0]) == b""


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan"), 2.0**63, -(2.0**63), 1e300])
def test_formatter_refuses_values_outside_its_range(ctx, bad):
    from tiebrush_amd.api import TbkError
    ctx.track_names(["chr1"])
    val = np.array([1.0, bad, 2.0])
    z = np.zeros(3, dtype=np.int32)
    with pytest.raises(TbkError) as e:
        ctx.format_track("cov", z, z, z, val=val)
    assert e.value.status == -5   # TBK_EUNSUPPORTED
    with pytest.raises(TbkError) as e:
        with np.errstate(over="ignore"):
            heat = np.array([1.0, bad, 0.0]).astype(np.float32)   # (1e300 -> inf)
        ctx.format_track("sample", z, z, z, count=np.zeros(3, dtype=np.int64), heat=heat)
    assert e.value.status == -5
