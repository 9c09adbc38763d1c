"""The host index builder in CSI mode (csrc/host/bai.h: what `tiebrush --csi` uses for everything the host writer deflates, and all of
`tbh_tool csi`) against the restatement of the CSI contract in csi_reader.py: the inflated .csi bytes, the validator's invariants, region
queries through the index against a brute-force scan, and — where the depth is 5 — the .bai of the same file.  CPU only."""
import os
import shutil
import subprocess

import pytest

import bai_reader as br
import csi_reader as cr
from helpers import GOLDEN

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiebrush_amd", "_build")
TOOL = os.environ.get("TBK_TEST_TBH_TOOL") or os.path.join(BIN, "tbh_tool")   # (the sanitizer builds of tools/san_check.sh)


def _index(path, what="csi"):
    r = subprocess.run([TOOL, what, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(path + "." + what + ".tmp")
    return open(path + "." + what, "rb").read()


@pytest.mark.parametrize("name", ["t1/t1.bam", "t2/t2.bam", "t12.bam"])
def test_goldens_csi_equals_the_restatement_and_the_bai(tmp_path, name):
    bam = str(tmp_path / os.path.basename(name))
    shutil.copy(os.path.join(GOLDEN, name), bam)
    data = open(bam, "rb").read()
    csi = _index(bam)
    assert cr.inflate(csi) == cr.expected_csi(data)
    cr.validate(data, csi)
    assert cr.region_checks(data, csi, seed=hash(name) & 0xffff) > 200
    # depth 5 is the BAI's binning: the same bins and chunks, the meta bin = the pseudo-bin, every loff = the .bai's ioffset of the bin's
    # first window
    depth, refs, _ = cr.parse_csi(csi)
    assert depth == 5 and cr.meta_bin(5) == br.PSEUDO_BIN
    bai_refs, _ = br.parse_bai(_index(bam, "bai"))
    assert len(refs) == len(bai_refs)
    for bins, B in zip(refs, bai_refs):
        assert [(b, ch) for b, _, ch in bins] == B["bins"]
        for b, loff, _ in bins:
            assert loff == (0 if b == br.PSEUDO_BIN else B["lin"][cr.bin_first_window(b, 5)]), b


def _levels(bins, depth):
    return set(cr.bin_level(b, depth) for b, _, _ in bins if b != cr.meta_bin(depth))


@pytest.fixture(scope="module")
def bai_synthetic(tmp_path_factory):
    """the BAI tests' synthetic file: its longest reference is 2^29, and 2^29 + 256 > 2^29 gives depth 6"""
    path = str(tmp_path_factory.mktemp("csi_syn") / "syn.bam")
    return path, cr.write_bam(path, br.SYN_NAMES, br.SYN_LENS, br.synthetic_records())


def test_bai_synthetic_file_at_depth_6(bai_synthetic):
    path, data = bai_synthetic
    csi = _index(path)
    assert cr.inflate(csi) == cr.expected_csi(data)
    cr.validate(data, csi)
    cr.region_checks(data, csi, seed=7, extra=[(0, (1 << 29) - 300, 1 << 29), (0, (1 << 29) - 1, 1 << 29), (2, 0, 1000000)])
    depth, refs, n_no_coor = cr.parse_csi(csi)
    assert depth == 6 and n_no_coor == 0
    assert refs[1] == []                                             # the empty reference: n_bin = 0
    assert [b for b, _, _ in refs[2]] == [cr.first_bin(6), cr.meta_bin(6)] and refs[2][-1][2][1] == (1, 0)
    a = {b: ch for b, _, ch in refs[0]}
    assert len(a[cr.first_bin(6) + 1]) == 1                          # interrupted by one parent-bin record inside a member: merged
    assert len(a[cr.first_bin(6) + 3]) == 2                          # interrupted across a member boundary: not merged
    assert _levels(refs[0], 6) == {1, 2, 3, 4, 5, 6}                 # (nothing crosses 2^29 here: the long file has level 0)
    assert _index(path, "bai") == br.expected_bai(data)              # (and the .bai of the same file still comes out)


@pytest.fixture(scope="module")
def long_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("csi_long") / "long.bam")
    return path, cr.write_bam(path, cr.LONG_NAMES, cr.LONG_LENS, cr.long_records())


def test_long_file(long_file):
    path, data = long_file
    _, lens, recs, _ = br.read_bam(data)
    assert lens == cr.LONG_LENS and len(recs) > 5500 and len(br.members(data)) >= 10   # (nine members and more, and the EOF member)
    csi = _index(path)
    assert cr.inflate(csi) == cr.expected_csi(data)
    cr.validate(data, csi)
    top = (1 << 31) - 1
    n = cr.region_checks(data, csi, seed=9, extra=[(0, (1 << 29) - 100, (1 << 29) + 100), (0, (3 << 29) - 50, (3 << 29) + 50), (0, 3 << 29, top),
                                                   (0, top - 1, top), (0, top - 200, top), (0, 0, top), (0, 1 << 30, top),
                                                   (2, (1 << 29) - 20, (1 << 29) + 1), (2, 1 << 29, (1 << 29) + 1), (2, 0, 1 << 29), (1, 0, 100000)])
    assert n > 200
    assert cr.query(data, csi, 0, top - 1, top) == [recs[-2]] and recs[-2][2] == top              # the record that ends on the last base
    assert cr.query(data, csi, 2, 1 << 29, (1 << 29) + 1) == [recs[-1]]                           # across 2^29 on the last reference
    depth, refs, _ = cr.parse_csi(csi)
    assert depth == 6
    assert refs[1] == []                                             # the empty reference: n_bin = 0
    assert _levels(refs[0], 6) == {0, 1, 2, 3, 4, 5, 6}              # one bin at every one of the seven levels
    nums = [b for b, _, _ in refs[0]]
    assert nums[-1] == cr.meta_bin(6) == 299594 and nums[-2] == cr.LONG_LAST_LEAF == cr.reg2bin(top - 100, top + 1, 6)
    assert any(b < 1 << 16 for b in nums if b >= cr.first_bin(6)) and sum(b >= 1 << 16 for b in nums) >= 20
    a = {b: ch for b, _, ch in refs[0]}
    moved = cr.first_bin(6) + (cr.LONG_SHIFT >> 14)
    assert len(a[moved + 1]) == 1 and len(a[moved + 3]) == 2         # the merged and the split interrupted bin, moved up
    assert [b for b, _, _ in refs[2]] == [0, cr.meta_bin(6)]         # 2^29 - 10 + 50M crosses the 512 Mb boundary: bin 0


def test_both_tools_on_the_long_file(long_file, tmp_path):
    path = str(tmp_path / "long.bam")
    shutil.copy(long_file[0], path)
    r = subprocess.run([TOOL, "bai", path], capture_output=True, text=True)
    assert r.returncode != 0 and "chrLong" in r.stderr
    assert os.listdir(str(tmp_path)) == ["long.bam"]                 # no .bai, no temporary file
    r = subprocess.run([TOOL, "csi", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["long.bam", "long.bam.csi"]
    from tiebrush_amd import _lib
    H = _lib.load_host()
    assert H.tbh_bai_index_file(path.encode(), None) == -1 and b"chrLong" in H.tbh_last_error()
    other = str(tmp_path / "other.csi")
    assert H.tbh_csi_index_file(path.encode(), other.encode()) == 0
    assert cr.inflate(open(other, "rb").read()) == cr.inflate(open(path + ".csi", "rb").read())


@pytest.mark.parametrize("ref_len,depth,meta", [(10000, 0, 2), (100000, 1, 10)])
def test_depth_0_and_1(tmp_path, ref_len, depth, meta):
    path = str(tmp_path / "small.bam")
    data = cr.write_bam(path, ["chrS"], [ref_len], cr.small_records(ref_len))
    csi = _index(path)
    assert cr.inflate(csi) == cr.expected_csi(data)
    cr.validate(data, csi)
    cr.region_checks(data, csi, seed=depth, n_random=50, extra=[(0, 0, ref_len), (0, ref_len - 1, ref_len)])
    d, refs, _ = cr.parse_csi(csi)
    assert d == depth and refs[0][-1][0] == meta == cr.meta_bin(depth)
    assert _levels(refs[0], depth) == set(range(depth + 1))


def test_depth_of_the_library_equals_the_rule():
    from tiebrush_amd import _lib
    H = _lib.load_host()
    for max_len, depth in ((0, 0), (16128, 0), (16129, 1), (100000, 1), (248956422, 5), ((1 << 29) - 256, 5), ((1 << 29) - 255, 6), (1 << 29, 6), ((1 << 31) - 1, 6)):
        assert H.tbh_csi_depth(max_len) == depth == cr.depth_for([max_len]), max_len
    assert [cr.meta_bin(d) for d in range(7)] == [2, 10, 74, 586, 4682, 37450, 299594]


def test_reg2bin_of_the_library_equals_the_restatement():
    from tiebrush_amd import _lib
    H = _lib.load_host()
    n = 0
    for depth in range(7):
        top = 1 << (14 + 3 * depth)
        assert H.tbh_csi_reg2bin(0, top, depth) == 0 and H.tbh_csi_reg2bin(top - 1, top, depth) == cr.first_bin(depth) + (1 << (3 * depth)) - 1
        for level in range(depth + 1):                              # every level's boundaries: the first ones and the last below the top
            shift = 14 + 3 * (depth - level)
            for k in sorted(set([1, 3, (1 << (3 * level)) - 1])):
                e = k << shift
                if not 0 < e < top:
                    continue
                for beg, end in ((e - 1, e), (e - 1, e + 1), (e, e + 1), (max(0, e - 50), min(top, e + 50)), (0, e), (e, top)):
                    assert H.tbh_csi_reg2bin(beg, end, depth) == cr.reg2bin(beg, end, depth), (beg, end, depth)
                    assert cr.reg2bin(beg, end, depth) in cr.reg2bins(beg, end, depth)
                    n += 1
    assert n > 300
    assert H.tbh_csi_reg2bin((1 << 31) - 101, 1 << 31, 6) == cr.LONG_LAST_LEAF == cr.reg2bin((1 << 31) - 100, 1 << 31, 6) == 168520
    import random                                                   # depth 5 is the BAI's reg2bin
    rng = random.Random(5)
    for _ in range(2000):
        beg = rng.randrange(1 << 29)
        end = min(1 << 29, beg + 1 + rng.choice([0, 30, 5000, 200000, 1 << 24]))
        assert H.tbh_csi_reg2bin(beg, end, 5) == br.reg2bin(beg, end) == H.tbh_bai_reg2bin(beg, end)
