"""The host index builder (csrc/host/bai.h: what `tiebrush --index` uses for everything the host writer deflates, and all of
`tbh_tool bai`) against the restatement of the index contract in bai_reader.py: the .bai bytes, the validator's invariants, and
region queries through the index against a brute-force scan of the file.  CPU only."""
import os
import shutil
import subprocess

import pytest

import bai_reader as br
from helpers import GOLDEN

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiebrush_amd", "_build")
TOOL = os.environ.get("TBK_TEST_TBH_TOOL") or os.path.join(BIN, "tbh_tool")   # (the sanitizer builds of tools/san_check.sh)


def _index(path):
    r = subprocess.run([TOOL, "bai", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(path + ".bai", "rb").read()


@pytest.mark.parametrize("name", ["t1/t1.bam", "t2/t2.bam", "t12.bam"])
def test_goldens_index_equals_the_restatement(tmp_path, name):
    bam = str(tmp_path / os.path.basename(name))
    shutil.copy(os.path.join(GOLDEN, name), bam)
    data = open(bam, "rb").read()
    bai = _index(bam)
    assert bai == br.expected_bai(data)
    br.validate(data, bai)
    assert br.region_checks(data, bai, seed=hash(name) & 0xffff) > 200
    if name == "t1/t1.bam":        # (the regions that end on a multiple of 16384 have records on both sides here)
        _, _, recs, _ = br.read_bam(data)
        w = sorted(set(r[1] >> 14 for r in recs if r[0] == recs[0][0]))
        assert any(b == a + 1 for a, b in zip(w, w[1:]))


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    from tiebrush_amd import bamio
    path = str(tmp_path_factory.mktemp("bai") / "syn.bam")
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(br.SYN_NAMES, br.SYN_LENS))
    bamio.write_bam(path, text, br.SYN_NAMES, br.SYN_LENS, b"".join(br.synthetic_records()), level=6)
    return path, open(path, "rb").read()


def test_synthetic_file(synthetic):
    path, data = synthetic
    bai = _index(path)
    _, _, recs, _ = br.read_bam(data)
    assert len(recs) > 5500 and len(br.members(data)) >= 10      # (nine members and more, and the EOF member)
    assert bai == br.expected_bai(data)
    br.validate(data, bai)
    br.region_checks(data, bai, seed=7)
    refs, n_no_coor = br.parse_bai(bai)
    assert n_no_coor == 0
    assert refs[1] == {"bins": [], "lin": []}                     # the empty reference: n_bin = 0, n_intv = 0
    one = dict(refs[2]["bins"])
    assert sorted(one) == [4681, br.PSEUDO_BIN] and one[br.PSEUDO_BIN][1] == (1, 0) and len(refs[2]["lin"]) == 1
    a = dict(refs[0]["bins"])
    assert len(a[br.SYN_MERGE_BIN]) == 1                          # interrupted by one parent-bin record inside a member: merged
    assert len(a[br.SYN_SPLIT_BIN]) == 2                          # interrupted across a member boundary: not merged
    levels = {0: 0, 1: 1, 9: 2, 73: 3, 585: 4, 4681: 5}
    seen = set(max(v for f, v in levels.items() if b >= f) for b in a if b != br.PSEUDO_BIN)
    assert seen == {0, 1, 2, 3, 4, 5}                             # one bin at every level
    assert len(refs[0]["lin"]) == 1 << 15                         # the record that ends on 2^29
    spliced = [r for r in recs if r[2] - r[1] > 700000][0]
    w0 = spliced[1] >> 14
    assert refs[0]["lin"][w0 + 1:w0 + 41] == [spliced[3]] * 40   # every window the intron spans points at the spliced record
    zero = [r for r in recs if r[0] == 0 and r[1] == 60 * 16384 + 5][0]
    assert zero[2] == zero[1] + 1 and br.query(data, bai, 0, zero[1], zero[1] + 1)[-1] == zero


def test_long_contig_is_refused_by_name(tmp_path):
    from tiebrush_amd import _lib, bamio
    path = str(tmp_path / "long.bam")
    names, lens = ["short", "chrTooLong"], [1000, (1 << 29) + 1]
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens))
    bamio.write_bam(path, text, names, lens, bamio.encode_record(0, 10, 0, 60, [50 << 4], b"r"))
    r = subprocess.run([TOOL, "bai", path], capture_output=True, text=True)
    assert r.returncode != 0 and "chrTooLong" in r.stderr and not os.path.exists(path + ".bai")
    H = _lib.load_host()
    assert H.tbh_bai_index_file(path.encode(), None) == -1 and b"chrTooLong" in H.tbh_last_error()
    lens[1] = 1 << 29                                                # exactly 2^29 is addressable
    bamio.write_bam(path, text.replace(str((1 << 29) + 1), str(1 << 29)), names, lens, bamio.encode_record(0, 10, 0, 60, [50 << 4], b"r"))
    assert H.tbh_bai_index_file(path.encode(), None) == 0
    br.validate(open(path, "rb").read(), open(path + ".bai", "rb").read())


def test_reg2bin_of_the_library_equals_the_specification():
    from tiebrush_amd import _lib
    H = _lib.load_host()
    for shift in (14, 17, 20, 23, 26, 29):
        for k in (1, 3):
            e = k << shift
            if e > 1 << 29:
                continue
            for beg, end in ((e - 1, e), (e - 1, e + 1), (e, e + 1), (max(0, e - 50), min(1 << 29, e + 50)), (0, e)):
                assert H.tbh_bai_reg2bin(beg, end) == br.reg2bin(beg, end), (beg, end)
