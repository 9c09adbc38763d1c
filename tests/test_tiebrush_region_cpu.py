"""`tiebrush -r REGION`, the refusals that come before the device is brought up: exit status 1, a message that names the
file concerned, and nothing created — no OUT.bam, no index, no track file.  They run without a GPU.  The tiebrush tests fail on a
build without the feature (-r is an unknown option there); the tiecov test holds its behaviour still while its repeat count moves to the
counter both tools share."""
import os
import shutil
import struct
import subprocess

import pytest

import csi_reader as cr
import region_fixtures as rf
from helpers import GOLDEN

BIN = rf.BIN


def _tiebrush(args):
    return subprocess.run([os.path.join(BIN, "tiebrush")] + [str(a) for a in args], capture_output=True, text=True, stdin=subprocess.DEVNULL)


def _pack_bai(n_ref, tid, chunks):
    """a .bai of n_ref references that holds nothing but `chunks` [(beg, end) virtual offsets], in bin 0 of `tid`: no linear table, so a
    query of any region of tid gives these chunks (those that meet in one compressed offset joined)"""
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for t in range(n_ref):
        if t == tid:
            out += struct.pack("<iIi", 1, 0, len(chunks)) + b"".join(struct.pack("<QQ", b, e) for b, e in chunks)
        else:
            out += struct.pack("<i", 0)
        out += struct.pack("<i", 0)
    return out


N_MANY = 65536                                                      # one more chunk than the device decode takes spans


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two indexed golden samples, a copy without an index, a copy cut short under the whole file's index, a copy under another file's
    index, a SAM text file, hand-built files whose reference lists differ (one lacks the last reference, one has another name at a
    position, one the same names at other positions), and copies of a golden sample under hand-packed indexes: two with N_MANY chunks between them,
    one whose chunk ends inside something that is no BGZF member, one whose second chunk begins inside the first one's last member"""
    from tiebrush_amd import bamio
    d = tmp_path_factory.mktemp("tb_region_cpu")
    f = {}
    f["a"] = rf.Fixture(rf.golden_copy(d, "t1/t1s0.bam"), kinds=("bai",))
    f["b"] = rf.Fixture(rf.golden_copy(d, "t1/t1s1.bam"), kinds=("csi",))
    f["bare"] = str(d / "bare.bam")
    shutil.copy(f["a"].path, f["bare"])
    f["half"] = str(d / "half.bam")
    cut = sorted(f["a"].msize)[len(f["a"].msize) // 2]                # (at a member that begins with a record, or not: the reads never happen)
    open(f["half"], "wb").write(f["a"].data[:cut] + cr.EOF_MEMBER)
    shutil.copy(f["a"].indexes["bai"], f["half"] + ".bai")
    recs = [bamio.encode_record(t, 100 + 10 * i, 0, 60, [50 << 4], b"r%d_%d" % (t, i), aux=b"NHC\x01") for t in (0, 1) for i in range(5)]
    f["two"] = str(d / "two.bam")
    cr.write_bam(f["two"], ["chrA", "chrB"], [10000, 20000], recs)
    rf.index(f["two"], "bai")
    f["one"] = str(d / "one.bam")
    cr.write_bam(f["one"], ["chrA"], [10000], recs[:5])
    rf.index(f["one"], "bai")
    f["renamed"] = str(d / "renamed.bam")                           # another name at the same position
    cr.write_bam(f["renamed"], ["chrA", "chrC"], [10000, 20000], recs)
    rf.index(f["renamed"], "bai")
    f["swapped"] = str(d / "swapped.bam")                           # the same names at other positions
    cr.write_bam(f["swapped"], ["chrB", "chrA"], [20000, 10000], recs)
    rf.index(f["swapped"], "bai")
    a = f["a"]
    t12 = a.names.index("chr12")
    mem = sorted(a.msize)                                           # (member offsets; mem[0] holds the header)
    assert 4 * (40000 - 1) + 2 + 18 <= len(a.data) and a.msize[mem[1]] > 2
    packed = {"many_a": [((4 * i) << 16, (4 * i + 2) << 16) for i in range(40000)],   # 2-byte chunks that do not touch: none is joined;
              "many_b": [((4 * i) << 16, (4 * i + 2) << 16) for i in range(N_MANY - 40000)],   # each file's are few enough, the sum is not
              "nomember": [(mem[1] << 16, ((mem[1] + 5) << 16) | 1)],
              "inside": [(mem[1] << 16, (mem[2] << 16) | 1), ((mem[2] + 1) << 16, (mem[2] + 2) << 16)]}
    for name, chunks in packed.items():
        f[name] = str(d / (name + ".bam"))
        shutil.copy(a.path, f[name])
        open(f[name] + ".bai", "wb").write(_pack_bai(len(a.names), t12, chunks))
    f["foreign"] = str(d / "foreign.bam")                           # a golden sample under the index of a file with two references
    shutil.copy(f["a"].path, f["foreign"])
    shutil.copy(f["two"] + ".bai", f["foreign"] + ".bai")
    f["sam"] = str(d / "t2.sam")
    shutil.copy(os.path.join(GOLDEN, "t2", "t2.sam"), f["sam"])
    return f


def _cases(f):
    a, b = f["a"].path, f["b"].path
    return [
        (["-r", "chr12:5-10", "-r", "chr12:7-9", a, b], ["more than once"]),
        (["-r", "chr12:5-10", "--region=chr12:7-9", a, b], ["more than once"]),
        (["--region", "chr12:5-10", "-Ar", "chr12:7-9", a, b], ["more than once"]),
        (["-r", "chr12:5-10", "--ranks", "2", a, b], ["--ranks"]),
        (["-r", "chr12:5-10", a, f["sam"]], ["not a BGZF", f["sam"]]),                    # SAM text
        (["-r", "chr12:5-10", a, "-"], ["standard input"]),
        (["-r", "chr12:5-10", a, f["bare"], b], ["no index found", f["bare"] + ".csi", f["bare"] + ".bai", f["bare"][:-4] + ".bai"]),
        (["-r", "chr12:5-10", a, f["foreign"]], ["references", f["foreign"]]),            # the index's n_ref is not its file's
        (["-r", "chrB:1-500", f["two"], f["one"]], ["chrB", f["one"]]),                   # the region's reference is not in every input's list
        (["-r", "chrA:1-500", f["two"], f["renamed"]], ["chrC", f["renamed"]]),            # ... another name at the region's reference's side
        (["-r", "chrB:1-500", f["renamed"], f["two"]], ["chrB", f["two"]]),
        (["-r", "chrA:1-500", f["two"], f["swapped"]], ["chrB", f["swapped"]]),            # ... the same name at another position
        (["-r", "chrZ", a, b], ["unknown reference name"]),
        (["-r", "chr12:x-y", a, b], ["malformed region"]),
        (["-r", "chr12:10-5", a, b], ["BEG > END"]),
        (["-r", "", a, b], ["malformed region"]),
        (["-r", "chr12", b, f["half"]], ["outside", f["half"]]),                           # a chunk that points outside its file
        (["-r", "chr12", b, f["nomember"]], ["does not end in a BGZF member", f["nomember"]]),   # ... the last member's header is read
        (["-r", "chr12", b, f["inside"]], ["outside", f["inside"]]),                      # ... a chunk inside the one before it
        # more spans in all than the decode takes: both numbers
        (["-r", "chr12", f["many_a"], f["many_b"]], ["2 inputs name %d chunks" % N_MANY, "takes 65535", f["many_a"]]),
    ]


def test_refusals_come_before_anything_exists(inputs, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    pre = str(out / "t")
    for k, (args, msgs) in enumerate(_cases(inputs)):
        extra = [["--index"], ["--csi"], ["--cov", pre + ".c", "--junc", pre + ".j"], ["--writer", "host", "--cov", pre, "--bigwig"]][k % 4]
        r = _tiebrush(["-o", str(out / "o.bam")] + extra + args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        for m in msgs:
            assert m in r.stderr, (args, m, r.stderr)
        assert "libtbk" not in r.stderr and "GPU" not in r.stderr, (args, r.stderr)      # (the device was never asked for)
        assert os.listdir(str(out)) == [], (args, os.listdir(str(out)))


def test_the_good_inputs_pass_every_refusal(inputs, tmp_path):
    """the same command line with nothing to refuse gets as far as the device: whatever it ends with there, it is not one of -r's refusals"""
    r = _tiebrush(["-o", str(tmp_path / "o.bam"), "-r", "chr12:98,595,000-98,596,000", inputs["a"].path, inputs["b"].path])
    assert "Error: -r" not in r.stderr and "invalid argument" not in r.stderr, r.stderr


def test_usage_names_the_option():
    r = subprocess.run([os.path.join(BIN, "tiebrush"), "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "-r,--region REGION" in r.stdout


def test_tiecov_still_refuses_a_second_region(inputs, tmp_path):
    """tiecov's repeat count is the shared counter now: -r twice in every spelling, values of other options that look like -r left alone"""
    tc = os.path.join(BIN, "tiecov")
    a = inputs["a"].path
    pre = str(tmp_path / "x")
    for args in (["-r", "chr12:5-10", "-r", "chr12:7-9"], ["-r", "chr12:5-10", "--region=chr12:7-9"], ["--region", "chr12:5-10", "-Wr", "chr12:7-9"]):
        r = subprocess.run([tc, "-c", pre] + args + ["--index-file", inputs["a"].indexes["bai"], a], capture_output=True, text=True)
        assert r.returncode == 1 and "more than once" in r.stderr, (args, r.stderr)
        assert os.listdir(str(tmp_path)) == []
    r = subprocess.run([tc, "-c", "-r", "-r", "chrZ", "--index-file", "--region", a], capture_output=True, text=True)   # one -r: -c's value is "-r"
    assert r.returncode == 1 and "more than once" not in r.stderr and "unknown reference name" in r.stderr, r.stderr
