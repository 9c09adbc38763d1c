"""The scenes of tests/bam_craft.py before the GPU sees them.  Every scene is what it claims to be (the claims are computed again from
its bytes), and every hand-written expectation is the host loaders' reading too: the streaming reader (`tbh_tool soa`: bam.cpp
index_records + TInputFiles::load_tile), the whole-input loader (`tbh_tool fastsoa`: fastload.cpp) and, on the scenes whose every
record it reads as they do, the Python decoder.  The malformed scenes are refused by both loaders with a message and a clean exit."""
import os
import subprocess

import numpy as np
import pytest

import bam_craft as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tiebrush_amd", "_build", "tbh_tool")
DTYPES = {"file_off": np.uint32, "tid": np.int32, "pos": np.int32, "flag": np.uint16, "mapq": np.uint8, "strand": np.uint8, "nh": np.int32,
          "cig_off": np.uint32, "cig": np.uint32, "md_off": np.uint32, "md": np.uint8, "md_has": np.uint8, "qname_off": np.uint32,
          "qname": np.uint8, "qname_hash": np.uint64, "yc_in": np.float64, "yx_in": np.int64, "yd_in": np.int64, "tbmerged": np.uint8}
FAST = ("file_off", "tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")


def _write(scene, d):
    paths = []
    for i, f in enumerate(scene.files):
        paths.append(os.path.join(d, "in%d.bam" % i))
        with open(paths[-1], "wb") as fh:
            fh.write(f)
    return paths


def _tool(cmd, scene, tmp_path):
    d = str(tmp_path / cmd)
    os.makedirs(d)
    r = subprocess.run([TOOL, cmd, d] + _write(scene, str(tmp_path)), capture_output=True, text=True)
    return r, (lambda name: np.fromfile(os.path.join(d, name), dtype=DTYPES[name]))


def _carried_equal(scene, want, rd):
    tb = scene.tb_mask()
    for name in bc.CARRIED:
        got = rd(name)
        assert got.shape == want[name].shape, name
        assert np.array_equal(got[tb], want[name][tb]), name


@pytest.mark.parametrize("name", list(bc.well_formed()))
def test_claims_hold_and_the_host_loaders_read_the_expectation(tmp_path, name):
    scene = bc.well_formed()[name]
    assert bc.check_claims(scene) == []
    assert all(len(f) <= 1 << 20 and bc.layout(f).n < 1 << 20 for f in scene.files)
    want = scene.expect()
    r, rd = _tool("soa", scene, tmp_path)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(rd("tbmerged"), scene.tbmerged)
    for a in ("file_off",) + bc.ARRAYS:
        got = rd(a)
        assert got.dtype == want[a].dtype and np.array_equal(got, want[a]), a
    if scene.tbmerged.any():
        _carried_equal(scene, want, rd)
    if not scene.unplaced:
        r, rd = _tool("fastsoa", scene, tmp_path)
        assert r.returncode == 0, r.stderr
        for a in FAST:
            assert np.array_equal(rd(a), want[a]), a
        if scene.tbmerged.any():
            _carried_equal(scene, want, rd)
    if scene.python:
        from tiebrush_amd import bamio
        lo = 0
        for f, recs in zip(scene.files, scene.recs):
            b = bamio.parse_bam(bamio.bgzf_decompress(f), keep_md=True)
            hi = lo + len(recs)
            assert b.n == len(recs)
            for a, mine in (("tid", b.tid), ("pos", b.pos), ("flag", b.flag), ("mapq", b.mapq), ("strand", b.strand), ("nh", b.nh), ("yc_in", b.yc),
                            ("yx_in", b.yx), ("yd_in", b.yd)):
                assert np.array_equal(np.asarray(mine).astype(want[a].dtype), want[a][lo:hi]) and np.array_equal(mine, want[a][lo:hi].astype(mine.dtype)), a
            assert [bytes(q) for q in b.qname] == [r.name for r in recs] and b.md == [r.md for r in recs]
            assert np.array_equal(b.cig, want["cig"][int(want["cig_off"][lo]):int(want["cig_off"][hi])])
            assert np.array_equal(b.has_yc, [bool(r.seen & bc.SEEN_YC) for r in recs])
            lo = hi


def test_files_without_records(tmp_path):
    """headers and nothing else: an empty tile from both loaders"""
    scene = bc.scene_all_empty()
    for cmd in ("soa", "fastsoa"):
        r, rd = _tool(cmd, scene, tmp_path / cmd)
        assert r.returncode == 0, r.stderr
        assert rd("file_off").tolist() == [0, 0, 0] and rd("tbmerged").tolist() == [0, 1] and rd("tid").size == 0


def test_the_scenes_cross_the_constants_they_are_placed_against():
    """a change of a builder cannot hollow the set out: between them the scenes hold the shortest record, one longer than a chunk of
    the chain kernel, one longer than two members, a member of 65536 bytes, every cut of a block_size field, and enough records for
    several blocks of the per-record kernels"""
    wf = bc.well_formed()
    sizes = set()
    for s in wf.values():
        for f in s.files:
            lay = bc.layout(f)
            sizes |= {e - o for o, e in zip(lay.offs, lay.ends)}
    assert min(sizes) == 37 and any(bc.IDX_CH < z < bc.MEMBER_MAX for z in sizes) and any(z > 2 * bc.MEMBER_MAX for z in sizes)
    assert any(90000 < z < 110000 for z in sizes)
    assert any(z % 64 for z in sizes) and any(z < 64 for z in sizes)
    assert {s.index for s in wf.values()} == {"member", "chain"}
    assert max(sum(len(f) for f in s.recs) for s in wf.values()) >= 3000
    for base in ("field_cut_member", "field_cut_48k", "end_48k", "long_record", "big_header", "member_edges"):   # two framings, one payload
        a, b = wf[base + "/member"], wf[base + "/hand"]
        assert [bc.layout(f).stream for f in a.files] == [bc.layout(f).stream for f in b.files] and (a.index, b.index) == ("member", "chain")
    assert bc.MALFORMED_KINDS == tuple(dict.fromkeys(bc.MALFORMED_KINDS)) and len(bc.malformed()) == 3 * len(bc.MALFORMED_KINDS)


def test_the_chunk_model_is_the_kernels():
    """bam_craft.Layout.chunks() restates how bam_index_k stages the stream: its constants are the kernel's"""
    src = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "bamdev.hip")).read()
    assert "constexpr uint32_t IDX_CH = 48 * 1024;" in src and "const uint64_t c0 = p & ~(uint64_t)15;" in src
    assert "fbytes[f] / 36 + 1" in src and "list[IDX_CH / 36 + 2]" in src


@pytest.mark.parametrize("name", list(bc.malformed()))
def test_malformed_scenes_are_refused_by_the_host_loaders(tmp_path, name):
    scene = bc.malformed()[name]
    for cmd in ("soa", "fastsoa"):
        r, _ = _tool(cmd, scene, tmp_path / cmd)
        assert r.returncode > 0, (name, cmd, r.returncode, r.stderr)      # a clean error exit, not a signal
        assert r.stderr.strip() != ""
