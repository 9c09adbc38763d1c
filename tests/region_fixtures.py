"""Fixtures and the restated contract of `tiecov -r`, shared by test_index_query_cpu.py and test_gpu_region.py: the
synthetic files of bai_reader.py / csi_reader.py written two ways and indexed, the goldens copied and indexed, the regions, the chunk
reads a caller makes, and the clip of whole-file rows in numpy."""
import os
import random
import shutil
import subprocess

import numpy as np

import bai_reader as br
import csi_reader as cr
from helpers import GOLDEN

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiebrush_amd", "_build")
TOOL = os.path.join(BIN, "tbh_tool")
W = 16384
SYN_SAMPLES = 3


def tool(*args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True)


def index(path, what):
    r = tool(what, path)
    assert r.returncode == 0, r.stderr
    return path + "." + what


def write_syn(path, names, lens, records, aligned):
    """the records under a header with SYN_SAMPLES sample lines.  Not `aligned`: bamio.write_bam, whose members are cut at a fixed size, so
    records straddle members (the chain indexer).  `aligned`: members cut as htslib cuts them — the header in a member of its own, a new
    member whenever the next record does not fit — so every member begins with a record (the lane-per-member indexer)"""
    from tiebrush_amd import bamio
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens)) + \
        "".join("@CO\tSAMPLE:s%d\n" % i for i in range(SYN_SAMPLES))
    if not aligned:
        bamio.write_bam(path, text, names, lens, b"".join(records), level=6)
        return path
    eof = bamio.bgzf_compress(b"", 6)
    assert len(eof) == 28

    def member(payload):
        z = bamio.bgzf_compress(payload, 6)
        assert len(payload) <= 0xff00 and z.endswith(eof)
        return z[:-28]
    parts, cur = [member(bamio.build_bam(text, names, lens, b""))], b""
    for r in records:
        if len(cur) + len(r) > 0xff00 - 40000:                    # (short members: more of them, more chunk ends inside members)
            parts.append(member(cur))
            cur = b""
        cur += r
    parts.append(member(cur))
    with open(path, "wb") as fh:
        fh.write(b"".join(parts) + eof)
    return path


class Fixture:
    """one BAM with its indexes: .path, .data, .names, .lens, .recs (tid, beg, end, vbeg), .indexes = {"bai": path, "csi": path}"""

    def __init__(self, path, kinds=("bai", "csi")):
        self.path = path
        self.data = open(path, "rb").read()
        self.names, self.lens, self.recs, self.vend = br.read_bam(self.data)
        self.indexes = {k: index(path, k) for k in kinds}
        self.msize = {}
        mem = br.members(self.data)
        for (at, _), nxt in zip(mem, [m[0] for m in mem[1:]] + [len(self.data)]):
            self.msize[at] = nxt - at
        self.starts = np.array([r[3] for r in self.recs], dtype=np.uint64)
        self.ends = set(r[3] for r in self.recs) | {self.vend}

    def spans(self, chunks):
        """[(bytes, first_uoff, last_uoff)]: what a caller reads for the chunks (whole members; the last member's size from the file)"""
        out = []
        for cb, ce in chunks:
            c0, c1, u1 = cb >> 16, ce >> 16, ce & 0xffff
            stop = c1 + (self.msize[c1] if u1 else 0)
            out.append((self.data[c0:stop], cb & 0xffff, u1))
        return out

    def in_chunks(self, chunks):
        """indices of the records inside the chunks, in file order; asserts the chunks are sorted, disjoint and cut at record starts"""
        idx, prev = [], None
        ends = self.ends
        for cb, ce in chunks:
            assert cb < ce, (cb, ce)
            assert prev is None or (cb >> 16) > (prev >> 16), "chunks are not sorted, or two of them meet in one member"
            assert cb in ends and ce in ends, "a chunk end is not a record start"
            a, b = np.searchsorted(self.starts, [cb, ce])
            idx.extend(range(int(a), int(b)))
            prev = ce
        return idx

    def brute(self, tid, beg, end):
        return br.brute(self.recs, tid, beg, end)


def random_regions(fx, seed, n):
    """drawn as bai_reader.region_checks draws them, cut to the reference"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        r = fx.recs[rng.randrange(len(fx.recs))]
        b = max(0, r[1] + rng.randrange(-40000, 40000))
        e = min(fx.lens[r[0]], b + rng.choice([1, 50, 1000, 20000, 200000, 3000000]))
        if b < e:
            out.append((r[0], b, e))
    return out


def syn_regions():
    """the hand-picked regions on the synthetic file (bai_reader.synthetic_records)"""
    iso = 50 * W - 20                                   # an isolated record [iso, iso + 50) across a 16 kb boundary
    intron = 70 * W + 10 + 50                           # the 700 kb intron starts here
    R = [(0, iso + 50, iso + 120), (0, iso - 100, iso),              # begins at a record's end / ends at a record's pos: both excluded
         (0, intron + 1000, intron + 2000),                          # inside the intron: no coverage row, the junction kept
         (0, 60 * W, 60 * W + 10), (0, 60 * W + 5, 60 * W + 6),       # the record of reference length 0
         (0, 30 * W + 1005, 30 * W + 1015), (0, 30 * W + 500, 30 * W + 5003),   # cuts interval rows in the middle at both ends
         (0, W + 150, W + 250), (0, 3 * W + 100, 4 * W), (0, 4 * W - 60, 4 * W - 45),   # parent-bin records inside leaf runs
         (0, 0, 1 << 29), (1, 0, 100000), (2, 0, 1000000),           # whole references: chrA, chrEmpty (zero rows), chrOne
         (2, 6000, 7000), (2, 500000, 600000), (0, 100, 200),        # behind the last record; beyond the linear table; before the first
         (0, (1 << 29) - 100, 1 << 29), (0, (1 << 29) - 1, 1 << 29), (2, 5049, 5050), (2, 5050, 5051)]
    for e in (4 * W, 31 * W, 50 * W):
        R += [(0, e, e + 1), (0, e - 1, e), (0, e - W, e)]
    for x in (50 * W, 7 << 17, 2 << 20, 1 << 23, 1 << 26):           # the record of every bin level
        R += [(0, x - 30, x + 40), (0, x - 1, x), (0, x, x + 1), (0, x + 29, x + 31)]
    return R


def golden_copy(tmp, name):
    path = os.path.join(str(tmp), os.path.basename(name))
    shutil.copy(os.path.join(GOLDEN, name), path)
    return path


# ---- the contract on rows ------------------------------------------------------------------------------------------------------------
def clip_cov(w, tid, beg, end):
    """whole-file rows (dict of numpy arrays as oracle_ffi.coverage returns them) -> the rows `-r` must give"""
    m = (w["iv_tid"] == tid) & (w["iv_start"] < end) & (w["iv_end"] > beg)
    j = (w["j_tid"] == tid) & (w["j_start"] < end) & (w["j_end"] > beg)
    out = dict(iv_tid=w["iv_tid"][m], iv_start=np.maximum(w["iv_start"][m], beg).astype(np.int32), iv_end=np.minimum(w["iv_end"][m], end).astype(np.int32),
               iv_val=w["iv_val"][m])
    out.update({k: w[k][j] for k in ("j_tid", "j_start", "j_end", "j_strand", "j_val")})
    return out


def clip_sample(w, tid, beg, end):
    m = (w["s_tid"] == tid) & (w["s_start"] < end) & (w["s_end"] > beg)
    return dict(s_tid=w["s_tid"][m], s_start=np.maximum(w["s_start"][m], beg).astype(np.int32), s_end=np.minimum(w["s_end"][m], end).astype(np.int32),
                s_count=w["s_count"][m], s_heat=w["s_heat"][m])


def clip_track_lines(lines, name, beg, end, junc=False):
    """the lines of a whole-file track file (header line first) -> the file `-r` must write, byte for byte"""
    out = [lines[0]]
    k = 0
    for ln in lines[1:]:
        f = ln.split("\t")
        a, b = int(f[1]), int(f[2])
        if f[0] != name or a >= end or b <= beg:
            continue
        if junc:
            k += 1
            f[3] = "JUNC%08d" % k
        else:
            f[1], f[2] = str(max(a, beg)), str(min(b, end))
        out.append("\t".join(f))
    return out
