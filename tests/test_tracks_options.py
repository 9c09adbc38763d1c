"""CPU-side checks of `tiebrush --cov / --junc / --samp / --bigwig`: option errors are reported before any device is touched, and the
new track entry points are declared and exported."""
import os
import subprocess

import pytest

from helpers import GOLDEN
from tiebrush_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")


def _tiebrush(args, tmp_path):
    exe = os.path.join(BIN, "tiebrush")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    # (TBK_PYTHON: a --ranks launcher that started anyway would fail differently, not with the message below)
    env = dict(os.environ, TBK_PYTHON=str(tmp_path / "no-such-python"))
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)


def test_bigwig_needs_cov(tmp_path):
    out = tmp_path / "o.bam"
    r = _tiebrush(["--bigwig", "--junc", str(tmp_path / "j"), "-o", str(out), os.path.join(GOLDEN, "t12.bam")], tmp_path)
    assert r.returncode == 1 and "--bigwig needs --cov" in r.stderr, r.stderr
    assert "GPU" not in r.stderr
    assert not out.exists() and not (tmp_path / "j.bed").exists()   # refused before the output or a track file is opened


@pytest.mark.parametrize("opt", [["--cov", "c"], ["--junc", "j"], ["--samp", "s"], ["--cov=c", "--bigwig"]])
def test_track_options_are_refused_with_ranks(tmp_path, opt):
    out = tmp_path / "o.bam"
    args = ["--ranks", "2"] + [str(tmp_path / a) if a in ("c", "j", "s") else a for a in opt]
    r = _tiebrush(args + ["-o", str(out), os.path.join(GOLDEN, "t12.bam")], tmp_path)
    assert r.returncode == 1, r.stderr
    assert "not available with --ranks" in r.stderr, r.stderr
    assert "GPU" not in r.stderr and "cannot start" not in r.stderr
    assert not out.exists()


def test_usage_lists_the_track_options(tmp_path):
    r = _tiebrush(["-h"], tmp_path)
    assert r.returncode == 0
    for o in ("--cov PREFIX", "--junc PREFIX", "--samp PREFIX", "--bigwig"):
        assert o in r.stdout


def test_track_symbols_are_bound():
    assert "tbk_track_names" in _lib.SYMBOLS and "tbk_format_track" in _lib.SYMBOLS
    L = _lib.load()
    assert L.tbk_abi_version() == 9
    assert hasattr(L, "tbk_track_names") and hasattr(L, "tbk_format_track")
    fields = [f for f, _ in _lib.TrackRows._fields_]
    assert fields[:4] == ["mem", "kind", "n", "reserved"] and fields[-1] == "first_junc"
