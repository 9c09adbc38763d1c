"""A plain-Python tabix reader (.tbi and tabix .csi), region query, and the restatement of the tabix contract that the tests
hold `tiecov --tabix`, `tiebrush --tabix`, `tbh_tool tabix` and tbk_track_bgzf against.  No htslib: BGZF is read with zlib and struct.

The contract is the BAM index's (bai_reader.py / csi_reader.py) with the track's lines in the records' place: beg = start,
end = max(end, start + 1), a line's vbeg = member offset << 16 | offset in the member's payload of its first byte, its vend = the next
line's vbeg, the last line's the EOF member's offset << 16.  The references are renumbered to those that have lines, in file order.
Indexes are compared on their INFLATED bytes: how a .tbi itself is compressed is not part of the contract."""
import struct
import zlib

import numpy as np

import bai_reader as br
import csi_reader as cr

EOF_MEMBER = cr.EOF_MEMBER
TBX_UCSC = 0x10000
NONE = br.NONE


def skip_of(text):
    """1 when the track starts with a `track` line"""
    return 1 if text.startswith(b"track") else 0


def inflate(gz):
    return b"".join(pay for _, pay in br.members(gz))


def _rows(text, p, voff, tid_of):
    """(tid, beg, end, vbeg) of the lines of `text` from offset p on, and the lines themselves"""
    recs, lines = [], []
    while p < len(text):
        e = text.index(b"\n", p) + 1
        f = text[p:e].split(b"\t")
        beg, end = int(f[1]), int(f[2])
        recs.append((tid_of(f[0]), beg, max(end, beg + 1), voff(p)))
        lines.append(text[p:e])
        p = e
    return recs, lines


def read_track(gz, skip):
    """(names in file order, rows (tid, beg, end, vbeg) with tid = the name's place in that list, vend of the last row, the rows' lines) from a
    .gz's own member table, its inflated text and skip"""
    assert gz[-28:] == EOF_MEMBER, "no EOF member"
    mem = br.members(gz)
    assert all(len(pay) <= 0xff00 for _, pay in mem)
    text = b"".join(pay for _, pay in mem)
    p = 0
    for _ in range(skip):
        p = text.index(b"\n", p) + 1
    names = []

    def tid_of(name):
        if not names or names[-1] != name:
            assert name not in names, "a reference comes back"
            names.append(name)
        return len(names) - 1
    voff = br._voffsets(mem, len(gz))
    recs, lines = _rows(text, p, voff, tid_of)
    return names, recs, voff(len(text)), lines


# ---- the restatement of the contract -------------------------------------------------------------------------------------------------
def restate(recs, vend, n_ref, depth=None):
    """bai_reader.restate (depth None: the BAI's bins) or csi_reader.restate with the lines as records"""
    return br.restate(recs, vend, n_ref) if depth is None else cr.restate(recs, vend, n_ref, depth)


def header_block(names, skip):
    nm = b"".join(n + b"\0" for n in names)
    return struct.pack("<7i", TBX_UCSC, 1, 2, 3, ord("#"), skip, len(nm)) + nm


def serialize(refs, names, skip, depth=None):
    """the inflated bytes of a .tbi (depth None) or of a tabix .csi; refs as restate gives them for the references WITH lines"""
    assert all(R["n"] for R in refs) and len(refs) == len(names)
    hb = header_block(names, skip)
    if depth is None:
        body = br.serialize(refs)
        assert body[:4] == b"BAI\x01"
        return b"TBI\x01" + struct.pack("<i", len(refs)) + hb + body[8:]
    body = cr.serialize(refs, depth)
    return b"CSI\x01" + struct.pack("<iii", cr.MIN_SHIFT, depth, len(hb)) + hb + body[16:]


def expected_index(gz, skip, depth=None):
    names, recs, vend, _ = read_track(gz, skip)
    return serialize(restate(recs, vend, len(names), depth), names, skip, depth)


def expected_part(run, head_len, names, ref_len, depth=None):
    """the index part of a run of tbk_track_bgzf (whole members, no EOF member) whose first head_len bytes are a header, as the arrays
    Context.track_bgzf returns; tid = the name's index in `names`"""
    mem = br.members(run)
    text = b"".join(pay for _, pay in mem)
    voff = br._voffsets([(at, pay) for at, pay in mem] + [(len(run), b"")], len(run))
    recs, _ = _rows(text, head_len, voff, lambda nm: names.index(nm))
    if not recs:
        return {"chunks": [], "lin": np.zeros(0, dtype=np.uint64), "lin_first": 0, "refs": []}
    refs = restate(recs, voff(len(text)), len(ref_len), depth)
    base = np.concatenate([[0], np.cumsum([(int(x) + 16383) >> 14 for x in ref_len])]).astype(np.int64)
    chunks = [(t, b, c[0], c[1]) for t, R in enumerate(refs) for b in sorted(R["bins"]) for c in R["bins"][b]]
    touched = [t for t, R in enumerate(refs) if R["n"]]
    lin_first = int(base[touched[0]])
    lin = np.full(int(base[touched[-1]]) + len(refs[touched[-1]]["lin"]) - lin_first, NONE, dtype=np.uint64)
    for t in touched:
        o = int(base[t]) - lin_first
        lin[o:o + len(refs[t]["lin"])] = refs[t]["lin"]
    return {"chunks": chunks, "lin": lin, "lin_first": lin_first, "refs": [(t, refs[t]["n"], refs[t]["first"], refs[t]["last"]) for t in touched]}


# ---- reader, query ---------------------------------------------------------------------------------------------------------------------
def index_bytes(index_file):
    """the bytes inside a .tbi / .csi file: whole BGZF members, the last one the EOF member"""
    return cr.inflate(index_file)


def parse(index_file):
    """{"depth": None (a .tbi) or the CSI's, "names", "skip", "format", "cols", "meta", "refs": [{"bins": {bin: (loff or None, chunks)}, "lin",
    "pseudo": (first, last, n, 0) or None}], "n_no_coor"} of a .tbi or tabix .csi file's bytes"""
    b = index_bytes(index_file)
    out = {}
    if b[:4] == b"TBI\x01":
        n_ref = struct.unpack_from("<i", b, 4)[0]
        p, depth = 8, None
    else:
        assert b[:4] == b"CSI\x01", "magic"
        min_shift, depth, l_aux = struct.unpack_from("<iii", b, 4)
        assert min_shift == cr.MIN_SHIFT and 0 <= depth <= cr.MAX_DEPTH
        p = 16
    fmt, c_seq, c_beg, c_end, meta, skip, l_nm = struct.unpack_from("<7i", b, p)
    nm = b[p + 28:p + 28 + l_nm]
    assert nm == b"" or nm[-1:] == b"\0"
    names = nm[:-1].split(b"\0") if nm else []
    p += 28 + l_nm
    if depth is not None:
        assert l_aux == 28 + l_nm, "l_aux"
        n_ref = struct.unpack_from("<i", b, p)[0]
        p += 4
    assert n_ref == len(names), "n_ref and the names"
    special = br.PSEUDO_BIN if depth is None else cr.meta_bin(depth)
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, p)[0]
        p += 4
        R = {"bins": {}, "lin": [], "pseudo": None}
        for _ in range(n_bin):
            if depth is None:
                bn, nc = struct.unpack_from("<Ii", b, p)
                loff, p = None, p + 8
            else:
                bn, loff, nc = struct.unpack_from("<IQi", b, p)
                p += 16
            ch = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(nc)]
            p += 16 * nc
            if bn == special:
                assert nc == 2
                R["pseudo"] = ch[0] + ch[1]
            else:
                assert bn not in R["bins"]
                R["bins"][bn] = (loff, ch)
        if depth is None:
            n_intv = struct.unpack_from("<i", b, p)[0]
            R["lin"] = list(struct.unpack_from("<%dQ" % n_intv, b, p + 4))
            p += 4 + 8 * n_intv
        refs.append(R)
    out["n_no_coor"] = struct.unpack_from("<Q", b, p)[0]
    assert p + 8 == len(b), "trailing bytes"
    out.update(depth=depth, names=names, skip=skip, format=fmt, cols=(c_seq, c_beg, c_end), meta=meta, refs=refs)
    return out


def _member(gz, at):
    """(payload, size) of the ONE member at file offset `at`"""
    assert gz[at:at + 4] == b"\x1f\x8b\x08\x04", "a chunk does not begin at a member"
    xlen = struct.unpack_from("<H", gz, at + 10)[0]
    x, bsize = at + 12, None
    while x < at + 12 + xlen:
        if gz[x:x + 2] == b"BC":
            bsize = struct.unpack_from("<H", gz, x + 4)[0] + 1
        x += 4 + struct.unpack_from("<H", gz, x + 2)[0]
    return zlib.decompress(gz[at + 12 + xlen:at + bsize - 8], -15), bsize


def _chunk_lines(gz, cb, ce):
    """the lines (vbeg, bytes) of one chunk, inflating only the members it names"""
    at, u = cb >> 16, cb & 0xffff
    pay, size = _member(gz, at)
    out = []
    while True:
        while u >= len(pay):                      # the line begins in the next member
            at, u = at + size, u - len(pay)
            if at >= len(gz):
                return out
            pay, size = _member(gz, at)
            if not pay:                            # the EOF member
                return out
        v = at << 16 | u
        if v >= ce:
            return out
        line = b""
        while True:                                # a line may straddle members
            e = pay.find(b"\n", u)
            if e >= 0:
                line += pay[u:e + 1]
                u = e + 1
                break
            line += pay[u:]
            at, u = at + size, 0
            pay, size = _member(gz, at)
            assert pay, "a line runs into the EOF member"
        out.append((v, line))


def _overlaps(line, name, beg, end):
    f = line.split(b"\t")
    b0 = int(f[1])
    return f[0] == name and b0 < end and max(int(f[2]), b0 + 1) > beg


def query(gz, index_file, name, beg, end):
    """the lines of reference `name` (bytes) that overlap [beg, end), found THROUGH the index: the bins of the region, the chunks behind the
    window table's (or the loff's) offset, only those chunks' members inflated"""
    ix = parse(index_file)
    if name not in ix["names"]:
        return []
    R = ix["refs"][ix["names"].index(name)]
    depth = ix["depth"]
    if depth is None:
        lin = R["lin"]
        min_off = lin[beg >> 14] if (beg >> 14) < len(lin) else (lin[-1] if lin else 0)
        bins = br.reg2bins(beg, end)
    else:
        b, min_off = cr.first_bin(depth) + (beg >> cr.MIN_SHIFT), 0
        while True:
            if b in R["bins"]:
                min_off = R["bins"][b][0]
                break
            if b == 0:
                break
            b = (b - 1) >> 3
        bins = cr.reg2bins(beg, end, depth)
    chunks = sorted(c for b in bins for c in R["bins"].get(b, (None, []))[1] if c[1] > min_off)
    found = {}
    for cb, ce in chunks:
        for v, line in _chunk_lines(gz, cb, ce):
            if _overlaps(line, name, beg, end):
                found[v] = line
    return [found[v] for v in sorted(found)]


def brute(lines, name, beg, end):
    """a linear filter of the inflated lines"""
    return [l for l in lines if _overlaps(l, name, beg, end)]


def region_checks(gz, index_file, seed, n_random=200):
    """n_random seeded regions around the rows, and every 16 kb window edge a row touches, through the index against the linear filter"""
    import random
    ix = parse(index_file)
    names, recs, _, lines = read_track(gz, ix["skip"])
    assert names == ix["names"]
    if not recs:
        return 0
    limit = 1 << (cr.MIN_SHIFT + 3 * (5 if ix["depth"] is None else ix["depth"]))
    rng = random.Random(seed)
    regions = []
    for _ in range(n_random):
        r = recs[rng.randrange(len(recs))]
        b = max(0, r[1] + rng.randrange(-40000, 40000))
        regions.append((r[0], b, b + rng.choice([1, 50, 1000, 20000, 200000, 3000000])))
    edges = sorted(set((r[0], w << 14) for r in recs for w in ((r[1] >> 14), ((r[2] - 1) >> 14) + 1) if w))
    for tid, e in edges:
        regions += [(tid, e, e + 1), (tid, e - 1, e), (tid, e - 16384, e), (tid, e, e + 16384), (tid, max(0, e - 100), e + 100)]
    for tid, b, e in regions:
        e = min(e, limit)
        if b < e:
            assert query(gz, index_file, names[tid], b, e) == brute(lines, names[tid], b, e), (names[tid], b, e)
    return len(regions)


def check_file(gz, index_file, plain, seed=1, n_random=200):
    """everything the tests ask of one track: the .gz inflates to the plain track, its index equals the restatement on its own bytes,
    and the region queries equal the linear filter"""
    assert inflate(gz) == plain, "the .gz does not inflate to the plain track"
    ix = parse(index_file)
    skip = skip_of(plain)
    assert (ix["format"], ix["cols"], ix["meta"], ix["skip"], ix["n_no_coor"]) == (TBX_UCSC, (1, 2, 3), ord("#"), skip, 0)
    assert index_bytes(index_file) == expected_index(gz, skip, ix["depth"]), "the index is not the restatement of its file"
    return region_checks(gz, index_file, seed, n_random)
