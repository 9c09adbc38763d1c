"""A plain-Python CSI reader, region query, validator, and the restatement of the CSI contract that the tests hold
`tiebrush --csi`, `tbh_tool csi` and tbk_bam_encode_indexed(csi_depth=...) against.  The BAI contract of bai_reader.py with three
changes: bins of a depth taken from the longest reference, a loff per bin in place of the linear table, and the meta bin.  Indexes are
compared on their INFLATED bytes: the compression level and the member cuts of a .csi are not part of the contract."""
import bisect
import functools
import struct

import numpy as np

import bai_reader as br

MIN_SHIFT = 14
MAX_DEPTH = 6
NONE = br.NONE
EOF_MEMBER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def depth_for(lens):
    """the smallest depth whose bins cover the longest reference + 256"""
    d = 0
    while max(lens, default=0) + 256 > 1 << (MIN_SHIFT + 3 * d):
        d += 1
    return d


def first_bin(level):
    return (8 ** level - 1) // 7


def meta_bin(depth):
    return (8 ** (depth + 1) - 1) // 7 + 1


def reg2bin(beg, end, depth):
    end -= 1
    s, t = MIN_SHIFT, first_bin(depth)
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 8 ** (l - 1)
    return 0


def reg2bins(beg, end, depth):
    end -= 1
    out = [0]
    for l in range(1, depth + 1):
        s = MIN_SHIFT + 3 * (depth - l)
        out.extend(range(first_bin(l) + (beg >> s), first_bin(l) + (end >> s) + 1))
    return out


def bin_level(b, depth):
    return max(l for l in range(depth + 1) if b >= first_bin(l))


def bin_first_window(b, depth):
    l = bin_level(b, depth)
    return (b - first_bin(l)) << (3 * (depth - l))


# ---- the restatement of the contract -------------------------------------------------------------------------------------------------
def restate(recs, vend_last, n_ref, depth):
    """bai_reader.restate with the depth's binning (a copy: that file stays as it is)"""
    refs = [{"bins": {}, "lin": [], "n": 0, "first": None, "last": None} for _ in range(n_ref)]
    vends = [r[3] for r in recs[1:]] + [vend_last]
    bins = [reg2bin(r[1], r[2], depth) for r in recs]
    i = 0
    while i < len(recs):                       # a run: consecutive records with equal (tid, bin) -> one chunk
        tid, b = recs[i][0], bins[i]
        j = i
        while j + 1 < len(recs) and recs[j + 1][0] == tid and bins[j + 1] == b:
            j += 1
        refs[tid]["bins"].setdefault(b, []).append((recs[i][3], vends[j]))
        i = j + 1
    for R in refs:
        for b, ch in R["bins"].items():          # sorted by beg; neighbours that meet in one member are merged
            ch.sort()
            out = [ch[0]]
            for c in ch[1:]:
                if out[-1][1] >> 16 >= c[0] >> 16:
                    out[-1] = (out[-1][0], c[1])
                else:
                    out.append(c)
            R["bins"][b] = out
    for k, (tid, beg, end, vbeg) in enumerate(recs):
        R = refs[tid]
        R["n"] += 1
        R["first"] = vbeg if R["first"] is None else R["first"]
        R["last"] = vends[k]
        if len(R["lin"]) < ((end - 1) >> 14) + 1:         # window w: the first record, in file order, with end > w << 14
            R["lin"].extend([vbeg] * (((end - 1) >> 14) + 1 - len(R["lin"])))
    return refs


def serialize(refs, depth):
    """the CSI's bytes before compression; loff(bin) = lin[first 16 kb window of the bin]"""
    o = [b"CSI\x01", struct.pack("<iiii", MIN_SHIFT, depth, 0, len(refs))]
    for R in refs:
        if not R["n"]:
            o.append(struct.pack("<i", 0))
            continue
        o.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            o.append(struct.pack("<IQi", b, R["lin"][bin_first_window(b, depth)], len(R["bins"][b])))
            o.extend(struct.pack("<QQ", *c) for c in R["bins"][b])
        o.append(struct.pack("<IQiQQQQ", meta_bin(depth), 0, 2, R["first"], R["last"], R["n"], 0))
    o.append(struct.pack("<Q", 0))
    return b"".join(o)


def expected_csi(bam_bytes):
    names, lens, recs, vend = br.read_bam(bam_bytes)
    depth = depth_for(lens)
    return serialize(restate(recs, vend, len(lens), depth), depth)


def expected_part(run, ref_len, depth):
    """bai_reader.expected_part with the depth's bins"""
    recs, vend = br.read_run(run)
    refs = restate(recs, vend, len(ref_len), depth)
    base = np.concatenate([[0], np.cumsum([(int(x) + 16383) >> 14 for x in ref_len])]).astype(np.int64)
    chunks = [(t, b, c[0], c[1]) for t, R in enumerate(refs) for b in sorted(R["bins"]) for c in R["bins"][b]]
    touched = [t for t, R in enumerate(refs) if R["n"]]
    lin_first = int(base[touched[0]])
    lin = np.full(int(base[touched[-1]]) + len(refs[touched[-1]]["lin"]) - lin_first, NONE, dtype=np.uint64)
    for t in touched:
        o = int(base[t]) - lin_first
        lin[o:o + len(refs[t]["lin"])] = refs[t]["lin"]
    return {"chunks": chunks, "lin": lin, "lin_first": lin_first, "refs": [(t, refs[t]["n"], refs[t]["first"], refs[t]["last"]) for t in touched],
            "rec_vbeg": np.array([r[3] for r in recs] + [vend], dtype=np.uint64)}


# ---- reader, query, validator --------------------------------------------------------------------------------------------------------
def inflate(csi_file):
    """the bytes inside a .csi file: whole BGZF members, the last one the 28-byte EOF member"""
    assert csi_file[-28:] == EOF_MEMBER, "no EOF member"
    mem = br.members(csi_file)
    assert len(mem) >= 2 and all(pay for _, pay in mem[:-1]) and not mem[-1][1]
    return b"".join(pay for _, pay in mem)


@functools.lru_cache(maxsize=8)
def parse_csi(csi_file):
    """(depth, per reference [(bin, loff, [(beg, end)])], n_no_coor) of a .csi file's bytes"""
    b = inflate(csi_file)
    assert b[:4] == b"CSI\x01", "magic"
    min_shift, depth, l_aux, n_ref = struct.unpack_from("<iiii", b, 4)
    assert min_shift == MIN_SHIFT and 0 <= depth <= MAX_DEPTH and l_aux == 0
    p, refs = 20, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, p)[0]
        p += 4
        bins = []
        for _ in range(n_bin):
            bn, loff, nc = struct.unpack_from("<IQi", b, p)
            p += 16
            bins.append((bn, loff, [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(nc)]))
            p += 16 * nc
        refs.append(bins)
    n_no_coor = struct.unpack_from("<Q", b, p)[0]
    assert p + 8 == len(b), "trailing bytes"
    return depth, refs, n_no_coor


@functools.lru_cache(maxsize=8)
def _bam(bam_bytes):
    names, lens, recs, vend = br.read_bam(bam_bytes)
    return names, lens, recs, vend, [r[3] for r in recs]


def query(bam_bytes, csi_file, tid, beg, end):
    """the records (tid, beg, end, vbeg) overlapping [beg, end) that a reader finds THROUGH the index: the chunks of reg2bins(beg, end) that
    end behind min_off = the loff of the lowest existing ancestor-or-self of the leaf bin that holds beg (0: none), read record by record"""
    depth, refs, _ = parse_csi(csi_file)
    _, _, recs, vend, starts = _bam(bam_bytes)
    bins = {b: (loff, ch) for b, loff, ch in refs[tid] if b != meta_bin(depth)}
    b, min_off = first_bin(depth) + (beg >> MIN_SHIFT), 0
    while True:
        if b in bins:
            min_off = bins[b][0]
            break
        if b == 0:
            break
        b = (b - 1) >> 3
    found = set()
    for b in reg2bins(beg, end, depth):
        for cb, ce in bins.get(b, (0, []))[1]:
            if ce <= min_off:
                continue
            k = bisect.bisect_left(starts, cb)
            assert k < len(starts) and starts[k] == cb, "a chunk does not begin at a record"
            while k < len(recs) and starts[k] < ce:
                r = recs[k]
                if r[0] == tid and r[1] < end and r[2] > beg:
                    found.add(r)
                k += 1
    return sorted(found, key=lambda r: r[3])


def validate(bam_bytes, csi_file):
    """the invariants of bai_reader.validate with the depth's bins and meta bin, and every loff against a scan of the records"""
    names, lens, recs, vend, _ = _bam(bam_bytes)
    depth, refs, n_no_coor = parse_csi(csi_file)
    assert depth == depth_for(lens), "depth"
    assert len(refs) == len(lens), "n_ref"
    assert n_no_coor == 0
    starts = set(r[3] for r in recs)
    where = {}
    META = meta_bin(depth)
    for tid, bins in enumerate(refs):
        nums = [b for b, _, _ in bins]
        assert nums == sorted(set(nums)), "bins ascending"
        mine = [r for r in recs if r[0] == tid]
        by_bin = {}
        for r in mine:
            by_bin.setdefault(reg2bin(r[1], r[2], depth), []).append(r)
        for b, loff, ch in bins:
            if b == META:
                assert loff == 0 and len(ch) == 2 and ch[1] == (len(mine), 0), "meta bin counts"
                assert ch[0] == (mine[0][3], ([r[3] for r in recs] + [vend])[recs.index(mine[-1]) + 1]), "meta bin range"
                continue
            assert b < META - 1, "bin number"
            assert ch == sorted(ch) and all(c[0] < c[1] for c in ch), "chunks sorted"
            assert all(a[1] <= c[0] for a, c in zip(ch, ch[1:])), "chunks overlap"
            start = bin_first_window(b, depth) << MIN_SHIFT
            assert loff == min(r[3] for r in mine if r[2] > start), "loff"
            for c in ch:
                assert c[0] in starts and (c[1] in starts or c[1] == vend), "chunk ends are record starts"
                for r in by_bin.get(b, []):
                    if c[0] <= r[3] < c[1]:
                        where[r[3]] = where.get(r[3], 0) + 1
        assert (META in nums) == bool(mine)
        assert set(by_bin) == set(nums) - {META}, "the bins with records"
    assert all(where.get(r[3], 0) == 1 for r in recs), "every record in exactly one chunk of its own bin"


def region_checks(bam_bytes, csi_file, seed, n_random=200, extra=()):
    """bai_reader.region_checks through the CSI: random regions around the records, regions that start or end exactly on a multiple of
    16384, and the caller's own, against a brute-force scan"""
    import random
    _, lens, recs, _, _ = _bam(bam_bytes)
    rng = random.Random(seed)
    regions = list(extra)
    for _ in range(n_random):
        r = recs[rng.randrange(len(recs))]
        b = max(0, r[1] + rng.randrange(-40000, 40000))
        regions.append((r[0], b, b + rng.choice([1, 50, 1000, 20000, 200000, 3000000])))
    edges = sorted(set((r[0], (r[2] >> 14) << 14) for r in recs if (r[2] >> 14) << 14 > 0))[:40]
    for tid, e in edges:
        regions += [(tid, e, e + 1), (tid, e - 1, e), (tid, e - 16384, e), (tid, e, e + 16384), (tid, max(0, e - 100), e + 100)]
    depth = parse_csi(csi_file)[0]
    for tid, b, e in regions:
        e = min(e, 1 << (MIN_SHIFT + 3 * depth))
        if b < e:
            assert query(bam_bytes, csi_file, tid, b, e) == br.brute(recs, tid, b, e), (tid, b, e)
    return len(regions)


# ---- the "long" synthetic file: a reference of 2^31 - 1, records in bins above 2^16 --------------------------------------------------
LONG_NAMES, LONG_LENS = ["chrLong", "chrEmpty", "chrOver"], [(1 << 31) - 1, 100000, (1 << 29) + 1]
LONG_SHIFT = 5 << 28                                    # every leaf bin of the shifted shapes: 37449 + 81920 and above
LONG_LAST_LEAF = 168520                                 # the leaf bin of position 2^31 - 100


def moved(raw, tid, pos):
    """a raw record (block_size first) at another place; its bin field as htslib stores it (bam_reg2bin cut to 16 bits)"""
    bs, _, old, l_qname, mapq, _, n_cig = struct.unpack_from("<IiiBBHH", raw, 0)
    cig = struct.unpack_from("<%dI" % n_cig, raw, 36 + l_qname)
    rl = sum(c >> 4 for c in cig if (br.CONSUMES_REF >> (c & 15)) & 1)
    return raw[:4] + struct.pack("<iiBBH", tid, pos, l_qname, mapq, reg2bin(pos, pos + (rl or 1), 5) & 0xffff) + raw[16:]


def long_records():
    """~6,000 raw records (block_size first) in coordinate order on the references LONG_LENS (depth 6): bai_reader.synthetic_records' shapes
    on reference 0 moved up by LONG_SHIFT, records across a boundary of every level, a few near position 0 (bins below 2^16), one that
    ends on the last base of the 2^31 - 1 reference; reference 1 empty; reference 2 with one record across 2^29"""
    from tiebrush_amd import bamio
    M = 0
    rows = []
    for raw in br.synthetic_records():
        tid, pos = struct.unpack_from("<ii", raw, 4)
        if tid == 0:
            rows.append((pos + LONG_SHIFT, raw))
    seq, qual = bytes([0x12, 0x48] * 25), bytes([30 + (i % 11) for i in range(100)])

    def rec(pos, length, name):
        return (pos, bamio.encode_record(0, 0, 0, 60, [(length << 4) | M], name, aux=b"NHC\x01", l_seq=100, seq=seq, qual=qual))
    W = 16384
    rows += [rec(10, 50, b"n0"), rec(20, 50, b"n1"), rec(W - 10, 50, b"n2"), rec(2 * W + 5, 50, b"n3"), rec(28000 * W + 7, 50, b"n4")]
    far = 3 << 29                                              # clear of the moved shapes: a boundary of every level, 512 Mb first
    rows += [rec(far - 20, 50, b"b5"), rec(far + (1 << 26) - 20, 50, b"b4"), rec(far + (1 << 26) + (1 << 23) - 20, 50, b"b3"),
             rec(far + (1 << 26) + (1 << 23) + (1 << 20) - 20, 50, b"b2"), rec(far + (1 << 26) + (1 << 23) + (1 << 20) + (1 << 17) - 20, 50, b"b1"),
             rec(far + (1 << 26) + (1 << 23) + (1 << 20) + (1 << 17) + W - 20, 50, b"b0")]
    rows += [rec((1 << 31) - 101, 100, b"last")]              # ends on the last base: end = 2^31 - 1, the reference's length
    rows.sort(key=lambda r: r[0])
    return [moved(raw, 0, pos) for pos, raw in rows] + [moved(rec(0, 50, b"over")[1], 2, (1 << 29) - 10)]


def small_records(ref_len):
    """a handful of records on one short reference (depth 0 for 10000, depth 1 for 100000): inside a window, across one, up to the end"""
    from tiebrush_amd import bamio
    pos = [(5, 50), (100, 50), (100, 2000), (3000, 1)] + [(p, 60) for p in range(16350, ref_len - 100, 9000)] + [(ref_len - 40, 40)]
    pos.sort()
    return [bamio.encode_record(0, p, 0, 60, [l << 4], b"q%d" % i, aux=b"NHC\x01") for i, (p, l) in enumerate(pos)]


def write_bam(path, names, lens, records, level=6):
    from tiebrush_amd import bamio
    text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens))
    bamio.write_bam(path, text, names, lens, b"".join(records), level=level)
    return open(path, "rb").read()
