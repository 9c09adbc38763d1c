"""A plain-Python BAI reader, region query, validator, and the restatement of the index contract that the tests hold
`tiebrush --index`, `tbh_tool bai` and tbk_bam_encode_indexed against.  No htslib: BGZF and BAM are read with zlib and struct."""
import functools
import struct
import zlib

import numpy as np

NONE = (1 << 64) - 1
PSEUDO_BIN = 37450
CONSUMES_REF = 0x18D  # M D N = X


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


@functools.lru_cache(maxsize=8)
def members(data):
    """[(file offset, payload bytes)] of every BGZF member of `data`"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04", "not a BGZF member at %d" % at
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si, sl = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0] + 1
            x += 4 + sl
        pay = zlib.decompress(data[at + 12 + xlen:at + bsize - 8], -15)
        assert len(pay) == struct.unpack_from("<I", data, at + bsize - 4)[0]
        out.append((at, pay))
        at += bsize
    return out


def _voffsets(mem, total_size):
    """payload offset -> virtual offset: the member that holds the byte; the payload's end: the EOF member, else the end of the data"""
    starts, p = [], 0
    for at, pay in mem:
        starts.append((p, p + len(pay), at))
        p += len(pay)

    def voff(q):
        for p0, p1, at in starts:
            if p0 <= q < p1:
                return at << 16 | (q - p0)
        assert q == p
        return (mem[-1][0] if mem and not mem[-1][1] else total_size) << 16
    return voff


def _records(payload, p, voff):
    """(tid, beg, end, vbeg) of the records from payload offset p on, and the vend of the last"""
    recs = []
    while p < len(payload):
        bs, tid, pos, l_qname = struct.unpack_from("<IiiB", payload, p)
        n_cig = struct.unpack_from("<H", payload, p + 16)[0]
        cig = struct.unpack_from("<%dI" % n_cig, payload, p + 36 + l_qname)
        rl = sum(c >> 4 for c in cig if (CONSUMES_REF >> (c & 15)) & 1)
        recs.append((tid, pos, pos + (rl or 1), voff(p)))
        p += 4 + bs
    return recs, voff(len(payload))


def read_bam(data):
    """(reference names, reference lengths, records (tid, beg, end, vbeg), vend of the last record) of a BAM file's bytes"""
    mem = members(data)
    payload = b"".join(pay for _, pay in mem)
    assert payload[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<I", payload, 4)[0]
    n_ref = struct.unpack_from("<I", payload, p)[0]
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        ln = struct.unpack_from("<I", payload, p)[0]
        names.append(payload[p + 4:p + 4 + ln - 1].decode())
        lens.append(struct.unpack_from("<I", payload, p + 4 + ln)[0])
        p += 8 + ln
    recs, vend = _records(payload, p, _voffsets(mem, len(data)))
    return names, lens, recs, vend


def read_run(run):
    """the records and final vend of a run of whole members that holds records only (what tbk_bam_encode returns)"""
    mem = members(run)
    return _records(b"".join(pay for _, pay in mem), 0, _voffsets([(at, pay) for at, pay in mem] + [(len(run), b"")], len(run)))


# ---- the restatement of the contract -------------------------------------------------------------------------------------------------
def restate(recs, vend_last, n_ref):
    """per reference: {"bins": {bin: [(beg, end)]}, "lin": [ioffset per window], "n", "first", "last"} from (tid, beg, end, vbeg) in file order"""
    refs = [{"bins": {}, "lin": [], "n": 0, "first": None, "last": None} for _ in range(n_ref)]
    vends = [r[3] for r in recs[1:]] + [vend_last]
    i = 0
    while i < len(recs):                       # a run: consecutive records with equal (tid, bin) -> one chunk
        tid, b = recs[i][0], reg2bin(recs[i][1], recs[i][2])
        j = i
        while j + 1 < len(recs) and recs[j + 1][0] == tid and reg2bin(recs[j + 1][1], recs[j + 1][2]) == b:
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
        while len(R["lin"]) < ((end - 1) >> 14) + 1:   # window w: the first record, in file order, with end > w << 14
            R["lin"].append(vbeg)
    return refs


def serialize(refs):
    o = [b"BAI\x01", struct.pack("<i", len(refs))]
    for R in refs:
        if not R["n"]:
            o.append(struct.pack("<ii", 0, 0))
            continue
        o.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            o.append(struct.pack("<Ii", b, len(R["bins"][b])))
            o.extend(struct.pack("<QQ", *c) for c in R["bins"][b])
        o.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["first"], R["last"], R["n"], 0))
        o.append(struct.pack("<i%dQ" % len(R["lin"]), len(R["lin"]), *R["lin"]))
    o.append(struct.pack("<Q", 0))
    return b"".join(o)


def expected_bai(bam_bytes):
    names, lens, recs, vend = read_bam(bam_bytes)
    return serialize(restate(recs, vend, len(lens)))


def expected_part(run, ref_len):
    """the index part of a run (tbk_ix_part) as the arrays Context.bam_encode_indexed returns"""
    recs, vend = read_run(run)
    refs = restate(recs, vend, len(ref_len))
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
def parse_bai(b):
    assert b[:4] == b"BAI\x01", "magic"
    n_ref = struct.unpack_from("<i", b, 4)[0]
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, p)[0]
        p += 4
        bins = []
        for _ in range(n_bin):
            bn, nc = struct.unpack_from("<Ii", b, p)
            p += 8
            bins.append((bn, [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(nc)]))
            p += 16 * nc
        n_intv = struct.unpack_from("<i", b, p)[0]
        refs.append({"bins": bins, "lin": list(struct.unpack_from("<%dQ" % n_intv, b, p + 4))})
        p += 4 + 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", b, p)[0]
    assert p + 8 == len(b), "trailing bytes"
    return refs, n_no_coor


def query(bam_bytes, bai, tid, beg, end):
    """the records (tid, beg, end, vbeg) overlapping [beg, end) that a reader finds THROUGH the index"""
    refs, _ = parse_bai(bai)
    R = refs[tid]
    bins = dict(b for b in R["bins"] if b[0] != PSEUDO_BIN)
    lin = R["lin"]
    min_off = lin[beg >> 14] if (beg >> 14) < len(lin) else (lin[-1] if lin else 0)
    chunks = sorted(c for b in reg2bins(beg, end) for c in bins.get(b, []) if c[1] > min_off)
    mem = members(bam_bytes)
    payload = b"".join(pay for _, pay in mem)
    voff, pstart, q = _voffsets(mem, len(bam_bytes)), {}, 0
    for at, pay in mem:
        pstart[at] = q
        q += len(pay)
    found = []
    for cb, ce in chunks:
        q = pstart[cb >> 16] + (cb & 0xffff)
        while q < len(payload) and voff(q) < ce:
            bs, rt, pos, l_qname = struct.unpack_from("<IiiB", payload, q)
            n_cig = struct.unpack_from("<H", payload, q + 16)[0]
            rl = sum(c >> 4 for c in struct.unpack_from("<%dI" % n_cig, payload, q + 36 + l_qname) if (CONSUMES_REF >> (c & 15)) & 1)
            if rt == tid and pos < end and pos + (rl or 1) > beg:
                found.append((rt, pos, pos + (rl or 1), voff(q)))
            q += 4 + bs
    return sorted(set(found), key=lambda r: r[3])


def brute(recs, tid, beg, end):
    return [r for r in recs if r[0] == tid and r[1] < end and r[2] > beg]


def validate(bam_bytes, bai):
    names, lens, recs, vend = read_bam(bam_bytes)
    refs, n_no_coor = parse_bai(bai)
    assert len(refs) == len(lens), "n_ref"
    assert n_no_coor == 0
    starts = set(r[3] for r in recs)
    where = {}
    for tid, R in enumerate(refs):
        nums = [b for b, _ in R["bins"]]
        assert nums == sorted(set(nums)), "bins ascending"
        mine = [r for r in recs if r[0] == tid]
        for b, ch in R["bins"]:
            if b == PSEUDO_BIN:
                assert len(ch) == 2 and ch[1] == (len(mine), 0), "pseudo-bin counts"
                assert ch[0][0] == mine[0][3]
                continue
            assert ch == sorted(ch) and all(c[0] < c[1] for c in ch), "chunks sorted"
            assert all(a[1] <= c[0] for a, c in zip(ch, ch[1:])), "chunks overlap"
            for c in ch:
                assert c[0] in starts and (c[1] in starts or c[1] == vend), "chunk ends are record starts"
                for r in mine:
                    if c[0] <= r[3] < c[1] and reg2bin(r[1], r[2]) == b:
                        where[r[3]] = where.get(r[3], 0) + 1
        assert (PSEUDO_BIN in nums) == bool(mine)
        assert len(R["lin"]) == (((max(r[2] for r in mine) - 1) >> 14) + 1 if mine else 0), "n_intv"
    assert all(where.get(r[3], 0) == 1 for r in recs), "every record in exactly one chunk of its own bin"


# ---- the synthetic file ---------------------------------------------------------------------------------------------------------------
SYN_NAMES, SYN_LENS = ["chrA", "chrEmpty", "chrOne"], [1 << 29, 100000, 1000000]
SYN_RUNS = {10: 63, 12: 64, 14: 65, 16: 255, 18: 256, 20: 257}       # window -> records of one bin in a row (wave and block edges)
SYN_MERGE_BIN, SYN_SPLIT_BIN = 4681 + 1, 4681 + 3


def synthetic_records():
    """~6,000 raw records (block_size first) in coordinate order with the shapes the index has to get right; three references, the middle
    one empty, the last with one record"""
    from tiebrush_amd import bamio
    M, I, N, S = 0, 1, 3, 4
    W = 16384
    rows = []                                                      # (pos, cigar)
    # one bin, one record of its parent bin in between, the bin again — inside the first member: ONE chunk
    rows += [(W + 100 + i, [(50, M)]) for i in range(5)] + [(W + 200, [(20000, M)])] + [(W + 300 + i, [(50, M)]) for i in range(5)]
    # the same with more than a member's worth of parent-bin records in between: TWO chunks
    rows += [(3 * W + 100 + i, [(50, M)]) for i in range(30)] + [(4 * W - 100 + i // 10, [(200, M)]) for i in range(400)] + [(4 * W - 50, [(10, M)])] * 30
    for w, k in SYN_RUNS.items():
        rows += [(w * W + i, [(50, M)]) for i in range(k)]
    rows += [(30 * W + 37 * i, [(75, M)]) for i in range(4600)]   # the bulk: now and then across a window
    rows += [(50 * W - 20, [(50, M)]), (7 * (1 << 17) - 20, [(50, M)]), (2 * (1 << 20) - 20, [(50, M)]), ((1 << 23) - 20, [(50, M)]),
             ((1 << 26) - 20, [(50, M)])]                        # across a 16 kb, 128 kb, 1 Mb, 8 Mb, 64 Mb boundary: one bin at each level
    rows += [(60 * W + 5, [(30, I), (20, S)])]                    # reference length 0
    rows += [(70 * W + 10, [(50, M), (700000, N), (50, M)])]      # spliced over 40 windows and more
    rows += [((1 << 29) - 100, [(100, M)])]                       # ends on the last base a BAI addresses
    rows.sort(key=lambda r: r[0])
    rows = [(0, p, c) for p, c in rows] + [(2, 5000, [(50, M)])]
    seq, qual = bytes([0x12, 0x48] * 25), bytes([30 + (i % 11) for i in range(100)])
    return [bamio.encode_record(t, p, 0, 60, [(l << 4) | o for l, o in c], b"s%d" % i, aux=b"NHC\x01", l_seq=100, seq=seq, qual=qual)
            for i, (t, p, c) in enumerate(rows)]


def region_checks(bam_bytes, bai, seed, n_random=200):
    """random regions around the records, and regions that start or end exactly on a multiple of 16384, against a brute-force scan"""
    import random
    names, lens, recs, _ = read_bam(bam_bytes)
    rng = random.Random(seed)
    regions = []
    for _ in range(n_random):
        r = recs[rng.randrange(len(recs))]
        b = max(0, r[1] + rng.randrange(-40000, 40000))
        regions.append((r[0], b, b + rng.choice([1, 50, 1000, 20000, 200000, 3000000])))
    edges = sorted(set((r[0], (r[2] >> 14) << 14) for r in recs if (r[2] >> 14) << 14 > 0))[:40]
    for tid, e in edges:
        regions += [(tid, e, e + 1), (tid, e - 1, e), (tid, e - 16384, e), (tid, e, e + 16384), (tid, max(0, e - 100), e + 100)]
    for tid, b, e in regions:
        assert query(bam_bytes, bai, tid, b, e) == brute(recs, tid, b, e), (tid, b, e)
    return len(regions)
