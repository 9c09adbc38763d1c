"""CPU tests of the tabix tracks: `tbh_tool tabix` — the host path alone: host codec members cut at 0xff00, bai_build_part
per slice, BaiIndex's TBI / tabix-CSI serialisers — against the restatement and the reader of tbi_reader.py, and the refusals of
`tiecov --tabix` / `tiebrush --tabix`, which come before a device is touched."""
import os
import subprocess

import pytest

import csi_reader as cr
import tbi_reader as tr
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")
TOOL = os.environ.get("TBK_TEST_TBH_TOOL") or os.path.join(BIN, "tbh_tool")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(TOOL) and os.path.exists(os.path.join(BIN, "tiecov")) and os.path.exists(os.path.join(BIN, "tiebrush"))):
        import __graft_entry__ as g
        g.build()


def _tabix(bam, track, out):
    return subprocess.run([TOOL, "tabix", str(bam), str(track), str(out)], capture_output=True, text=True, timeout=120)


GOLDEN_TRACKS = [(t, k) for t in ("t1", "t2") for k in ("coverage.bedgraph", "junctions.bed", "sample.bedgraph")]


@pytest.mark.parametrize("t,kind", GOLDEN_TRACKS)
def test_golden_track(tmp_path, t, kind):
    src = os.path.join(GOLDEN, t, "%s.%s" % (t, kind))
    out = tmp_path / (kind + ".gz")
    r = _tabix(os.path.join(GOLDEN, t, t + ".bam"), src, out)
    assert r.returncode == 0, r.stderr
    plain = open(src, "rb").read()
    gz, tbi = out.read_bytes(), (tmp_path / (kind + ".gz.tbi")).read_bytes()
    assert not (tmp_path / (kind + ".gz.csi")).exists() and not (tmp_path / (kind + ".gz.tbi.tmp")).exists()
    n = tr.check_file(gz, tbi, plain, seed=7, n_random=200)
    assert n >= 200
    ix = tr.parse(tbi)
    seen = [l.split(b"\t")[0] for l in plain.split(b"\n")[1:-1]]
    assert ix["depth"] is None and ix["skip"] == 1 and ix["names"] == sorted(set(seen), key=seen.index)
    assert all(R["pseudo"] is not None for R in ix["refs"])


def _write_bam(path, names, lens):
    return cr.write_bam(str(path), names, lens, [])


def _track(rows, head=b"track type=bedGraph\n"):
    return head + b"".join(b"%s\t%d\t%d\t%d.000\n" % (n, s, e, i % 7) for i, (n, s, e) in enumerate(rows))


def _level_rows(name, depth):
    """rows that land in a bin of every level of a `depth`-level scheme, down to bin 0: one inside a 16 kb window and one across a boundary
    of 2^(14 + 3 l) for every l < depth, in start order; a row with end == start among them"""
    rows = [(name, 100, 200), (name, 150, 150), (name, 300, 400)]
    for l in range(depth):
        edge = 1 << (14 + 3 * l)
        rows.append((name, edge - 20 - l, edge + 20))
    return sorted(rows, key=lambda r: r[1])


def test_synthetic_tbi(tmp_path):
    names, lens = ["chrA", "chrEmpty", "chrOne"], [1 << 29, 100000, 1000000]
    bam = tmp_path / "h.bam"
    _write_bam(bam, names, lens)
    rows = _level_rows(b"chrA", 5) + [(b"chrA", 40000 + 37 * i, 40000 + 37 * i + 30) for i in range(9000)]
    rows.sort(key=lambda r: r[1])
    rows += [(b"chrA", (1 << 29) - 100, 1 << 29), (b"chrOne", 5000, 5050), (b"chrOne", 5000, 5000), (b"chrOne", 999000, 1000000)]
    plain = _track(rows)
    assert len(plain) > 3 * 0xff00
    src = tmp_path / "s.bedgraph"
    src.write_bytes(plain)
    r = _tabix(bam, src, tmp_path / "s.gz")
    assert r.returncode == 0, r.stderr
    gz, tbi = (tmp_path / "s.gz").read_bytes(), (tmp_path / "s.gz.tbi").read_bytes()
    tr.check_file(gz, tbi, plain, seed=3)
    ix = tr.parse(tbi)
    assert ix["names"] == [b"chrA", b"chrOne"]                       # the reference without rows is not listed
    bins = set(ix["refs"][0]["bins"])
    assert 0 in bins and all(any(cr.first_bin(l) <= b < cr.first_bin(l + 1) for b in bins) for l in range(6))
    # the row with end == start is found where a row [start, start + 1) would be
    got = tr.query(gz, tbi, b"chrOne", 5000, 5001)
    assert [g.split(b"\t")[1:3] for g in got] == [[b"5000", b"5050"], [b"5000", b"5000"]]
    assert tr.query(gz, tbi, b"chrA", 150, 151)[1].split(b"\t")[1:3] == [b"150", b"150"]


def test_synthetic_csi(tmp_path):
    names, lens = ["chrLong", "chrEmpty", "chrOne"], [(1 << 29) + 70000, 100000, 1000000]
    bam = tmp_path / "h.bam"
    _write_bam(bam, names, lens)
    rows = _level_rows(b"chrLong", 6)                                # the last one lies across 2^29: bin 0 of a depth of 6
    rows += [(b"chrLong", (1 << 29) + 100 + 50 * i, (1 << 29) + 140 + 50 * i) for i in range(1300)]
    rows += [(b"chrLong", (1 << 29) + 69000, (1 << 29) + 70000), (b"chrOne", 10, 10), (b"chrOne", 20, 30000)]
    plain = _track(rows, head=b"")                                   # no header line: skip 0
    src = tmp_path / "s.bed"
    src.write_bytes(plain)
    r = _tabix(bam, src, tmp_path / "s.gz")
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "s.gz.tbi").exists()
    gz, csi = (tmp_path / "s.gz").read_bytes(), (tmp_path / "s.gz.csi").read_bytes()
    tr.check_file(gz, csi, plain, seed=5)
    ix = tr.parse(csi)                                               # (parse checks l_aux == 28 + l_nm and that the aux block's names end the block)
    assert ix["depth"] == cr.depth_for(lens) == 6 and ix["skip"] == 0 and ix["names"] == [b"chrLong", b"chrOne"]
    bins = set(ix["refs"][0]["bins"])
    assert 0 in bins and all(any(cr.first_bin(l) <= b < cr.first_bin(l + 1) for b in bins) for l in range(7))
    assert len(tr.query(gz, csi, b"chrLong", (1 << 29) + 100, (1 << 29) + 200)) == 2


def test_header_only_and_empty_track(tmp_path):
    bam = tmp_path / "h.bam"
    _write_bam(bam, ["chrA"], [1000])
    for name, plain in (("h", b"track type=bedGraph\n"), ("e", b"")):
        src = tmp_path / (name + ".bedgraph")
        src.write_bytes(plain)
        r = _tabix(bam, src, tmp_path / (name + ".gz"))
        assert r.returncode == 0, r.stderr
        gz, tbi = (tmp_path / (name + ".gz")).read_bytes(), (tmp_path / (name + ".gz.tbi")).read_bytes()
        assert tr.inflate(gz) == plain and gz[-28:] == tr.EOF_MEMBER
        ix = tr.parse(tbi)
        assert ix["names"] == [] and ix["refs"] == [] and ix["skip"] == tr.skip_of(plain)
        assert tr.index_bytes(tbi) == tr.expected_index(gz, ix["skip"])


def test_older_files_are_removed_and_unsorted_input_is_refused(tmp_path):
    bam = tmp_path / "h.bam"
    _write_bam(bam, ["chrA", "chrB"], [1 << 20, 1 << 20])
    for stale in ("o.gz", "o.gz.tbi", "o.gz.csi"):
        (tmp_path / stale).write_bytes(b"stale")
    src = tmp_path / "u.bedgraph"
    src.write_bytes(_track([(b"chrA", 10, 20), (b"chrA", 30, 40), (b"chrA", 25, 50)]))
    r = _tabix(bam, src, tmp_path / "o.gz")
    assert r.returncode == 1 and "line 4" in r.stderr and "out of order" in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.gz")]                    # nothing of a refused track, old or new
    src.write_bytes(_track([(b"chrB", 10, 20), (b"chrA", 30, 40)], head=b""))
    r = _tabix(bam, src, tmp_path / "o.gz")
    assert r.returncode == 1 and "line 2" in r.stderr, r.stderr
    src.write_bytes(_track([(b"chrA", 10, 20), (b"chrA", 10, 15), (b"chrB", 0, 5)]))        # equal starts are in order
    r = _tabix(bam, src, tmp_path / "o.gz")
    assert r.returncode == 0, r.stderr
    src.write_bytes(_track([(b"chrA", 10, (1 << 20) + 20000)]))                              # behind its reference's last window
    r = _tabix(bam, src, tmp_path / "o.gz")
    assert r.returncode == 1 and "outside" in r.stderr, r.stderr


# ---- the command lines' refusals: before a device is touched --------------------------------------------------------------------------
def _run(exe, args, tmp_path):
    env = dict(os.environ, TBK_PYTHON=str(tmp_path / "no-such-python"))
    return subprocess.run([os.path.join(BIN, exe)] + args, capture_output=True, text=True, timeout=60, env=env)


T1 = os.path.join(GOLDEN, "t1", "t1.bam")


@pytest.mark.parametrize("cov", ["-", "stdout"])
def test_tiecov_tabix_refuses_coverage_to_stdout(tmp_path, cov):
    r = _run("tiecov", ["--tabix", "-c", cov, T1], tmp_path)
    assert r.returncode == 1 and "--tabix needs a coverage file" in r.stderr, r.stderr
    assert "GPU" not in r.stderr and r.stdout == ""


def test_tiecov_tabix_needs_a_track(tmp_path):
    r = _run("tiecov", ["--tabix", T1], tmp_path)
    assert r.returncode == 1 and "--tabix needs at least one of -c / -j / -s" in r.stderr, r.stderr
    assert "GPU" not in r.stderr


def test_tiecov_usage_lists_tabix(tmp_path):
    r = _run("tiecov", ["-h"], tmp_path)
    assert "--tabix" in r.stderr + r.stdout


@pytest.mark.parametrize("cov", ["-", "stdout"])
def test_tiebrush_tabix_refuses_coverage_to_stdout(tmp_path, cov):
    out = tmp_path / "o.bam"
    r = _run("tiebrush", ["--tabix", "--cov", cov, "-o", str(out), os.path.join(GOLDEN, "t12.bam")], tmp_path)
    assert r.returncode == 1 and "--tabix needs a coverage file" in r.stderr, r.stderr
    assert "GPU" not in r.stderr and not out.exists()


def test_tiebrush_tabix_needs_a_track(tmp_path):
    out = tmp_path / "o.bam"
    r = _run("tiebrush", ["--tabix", "-o", str(out), os.path.join(GOLDEN, "t12.bam")], tmp_path)
    assert r.returncode == 1 and "--tabix needs at least one of --cov / --junc / --samp" in r.stderr, r.stderr
    assert "GPU" not in r.stderr and not out.exists()


@pytest.mark.parametrize("opt", [["--cov", "c"], ["--junc", "j"], []])
def test_tiebrush_tabix_is_refused_with_ranks(tmp_path, opt):
    out = tmp_path / "o.bam"
    args = ["--ranks", "2", "--tabix"] + [str(tmp_path / a) if a in ("c", "j") else a for a in opt]
    r = _run("tiebrush", args + ["-o", str(out), os.path.join(GOLDEN, "t12.bam")], tmp_path)
    assert r.returncode == 1 and "--tabix is not available with --ranks" in r.stderr, r.stderr
    assert "GPU" not in r.stderr and "cannot start" not in r.stderr and not out.exists()
    assert not list(tmp_path.glob("*.gz"))


def test_tiebrush_usage_lists_tabix(tmp_path):
    r = _run("tiebrush", ["-h"], tmp_path)
    assert r.returncode == 0 and "--tabix" in r.stdout


def test_track_bgzf_symbol_is_bound():
    from tiebrush_amd import _lib
    assert "tbk_track_bgzf" in _lib.SYMBOLS
    L = _lib.load()
    assert hasattr(L, "tbk_track_bgzf")
