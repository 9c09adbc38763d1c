"""Hand-built BAM files for the device decode (the second half of tiebrush_amd/csrc/bamdev.hip: bam_header_k, the member walks
bam_imem_*_k, the chain bam_index_k, bam_fields_k, bam_fill_k, bam_compact_k, bam_recsize_k / bam_reccopy_k).  Scene builders only:
numpy, zlib and bamio's writer; importable without a GPU and without pytest.

A scene is a list of files (bytes), the tile those files must decode to, and `claims`: facts about its own bytes that make the
scene what its name says (which members begin inside a record, where a block_size field is cut, ...).  The tile is never read back
from a decoder: every record is described by a Rec, whose core fields are the ones it was encoded from and whose tag reading
(nh, strand, md, yc, yx, yd, seen) is written by hand beside its aux bytes.  check_claims() computes every claim again from the
bytes (test_bam_craft_cpu.py), where the host loader also has to agree with every expectation before the GPU is asked.

The constants the scenes are placed against: the chain kernel stages IDX_CH = 48 KiB of the inflated stream at a time, starting at
the next record's offset rounded down to 16 bytes; a BGZF member holds at most 65536 bytes; a record is at least 36 bytes in the
stream (37 with its empty name); bam_fields_k / bam_fill_k run 256 records to a block; bam_reccopy_k copies 64 bytes a step."""
import functools
import struct
import zlib

import numpy as np

from tiebrush_amd import bamio

NH_ABSENT = -(2**31)
IDX_CH = 48 * 1024
MEMBER_MAX = 65536
M, I, D, N, S = 0, 1, 2, 3, 4
REFS = (("chr1", 1000000), ("chr2", 500000), ("chrM", 16000))
HD = "@HD\tVN:1.6\tSO:coordinate\n"
PG = "@PG\tID:TieBrush\tPN:TieBrush\tVN:0.0.6\n@CO\tSAMPLE:hand_built.bam\n"
ARRAYS = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig", "md_off", "md", "md_has", "qname_off", "qname", "qname_hash")
CARRIED = ("yc_in", "yx_in", "yd_in")
SEEN_YC, SEEN_YX = 1, 2

_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f", "d": "d"}


# ---- aux bytes --------------------------------------------------------------------------------------------------------------------
def tag(name, ty, val=None):
    """one aux field: tag("NH", "C", 3), tag("XS", "A", "+"), tag("MD", "Z", b"10A5"), tag("XB", "B", ("s", [1, -2]))"""
    t = name.encode() + ty.encode()
    if ty in _FMT:
        return t + struct.pack("<" + _FMT[ty], val)
    if ty == "A":
        return t + val.encode()
    if ty in "ZH":
        return t + (val if isinstance(val, bytes) else val.encode()) + b"\0"
    assert ty == "B"
    sub, vals = val
    return t + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), _FMT[sub]), *vals)


def qname_hash(name: bytes, flag: int) -> int:
    """FNV-1a over the name bytes, then over pairOrder + 1 (tmerge.cpp tbh_qname_hash), restated"""
    h = 0xCBF29CE484222325
    for b in name:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    po = 1 if flag & 0x40 else (2 if flag & 0x80 else 0)
    return ((h ^ (po + 1)) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF


class Rec:
    """One record: what it is encoded from, and how its tags must be read (by hand, as a TieBrush-merged file's: yc / yx / yd and the
    seen bits are what a file flagged tbmerged, or a span, gives)."""

    def __init__(self, tid=0, pos=100, flag=0, mapq=60, cigar=((50, M),), name=b"r", aux=b"", l_seq=0, seqqual=None, mtid=-1, mpos=-1,
                 tlen=0, nh=NH_ABSENT, strand=".", md=None, yc=0.0, yx=1, yd=0, seen=0):
        self.tid, self.pos, self.flag, self.mapq, self.name = tid, pos, flag, mapq, name
        self.cig = [(l << 4) | o for l, o in cigar]
        if seqqual is None:
            seqqual = b"\x12" * ((l_seq + 1) // 2) + b"\x1e" * l_seq
        assert len(seqqual) == (l_seq + 1) // 2 + l_seq
        self.raw = bamio.encode_record(tid, pos, flag, mapq, self.cig, name, aux, l_seq, seqqual, b"", mtid, mpos, tlen)
        self.nh, self.strand, self.md, self.yc, self.yx, self.yd, self.seen = nh, strand, md, float(yc), yx, yd, seen


def header_bytes(pg=False, refs=REFS):
    """the BAM header (magic .. last reference)"""
    text = HD + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + (PG if pg else "")
    return bamio.build_bam(text, [r[0] for r in refs], [r[1] for r in refs], b"")


# ---- BGZF -------------------------------------------------------------------------------------------------------------------------
def frame(payload: bytes, cuts=(), level=6) -> bytes:
    """BGZF members of the pieces payload[a:b] between consecutive cuts (offsets into the payload; a repeated offset is an empty
    member), each of at most 65536 bytes, then the EOF member"""
    edges = [0] + sorted(cuts) + [len(payload)]
    assert edges[1] >= 0 and edges[-2] <= len(payload)
    out = []
    for a, b in zip(edges, edges[1:]):
        piece = payload[a:b]
        assert len(piece) <= MEMBER_MAX, (a, b)
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        c = co.compress(piece) + co.flush()
        bsize = len(c) + 25
        assert bsize <= 65535, "a piece that does not deflate into one member"
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, bsize) + c +
                   struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    out.append(bamio._BGZF_EOF)
    return b"".join(out)


def record_cuts(first, offs, n, limit=0xFF00, header_alone=True):
    """cuts as htslib's writer makes them: the header in members of its own (header_alone) or followed by the first records, a new
    member whenever the next record does not fit; every member begins with a record or inside the header"""
    cuts, start = [], 0
    hp = limit
    while hp < first:
        cuts.append(hp)
        start = hp
        hp += limit
    if header_alone and first > start:
        cuts.append(first)
        start = first
    ends = list(offs[1:]) + [n]
    for o, e in zip(offs, ends):
        if e - start > limit:
            assert o > start and e - o <= limit, "a record longer than a member cannot begin one"
            cuts.append(o)
            start = o
    return cuts


class Layout:
    """what the bytes of one file say: member boundaries in the inflated stream, the header's end, the record chain"""

    def __init__(self, data: bytes):
        self.mstart, self.msize = [], []
        off, tot = 0, 0
        while off < len(data):
            assert data[off:off + 4] == b"\x1f\x8b\x08\x04" and data[off + 12:off + 16] == b"BC\x02\x00"
            bsize = struct.unpack_from("<H", data, off + 16)[0]
            isize = struct.unpack_from("<I", data, off + bsize + 1 - 4)[0]
            self.mstart.append(tot)
            self.msize.append(isize)
            tot += isize
            off += bsize + 1
        self.stream = bamio.bgzf_decompress(data)
        self.n = len(self.stream)
        assert self.n == tot
        _, self.first = bamio.parse_header(self.stream)
        self.offs = []
        p = self.first
        while p < self.n:
            self.offs.append(p)
            p += 4 + struct.unpack_from("<I", self.stream, p)[0]
        assert p == self.n
        self.ends = self.offs[1:] + [self.n]

    def inside(self):
        """indices of the members (every member counts, empty ones and the EOF member too) that begin inside a record"""
        starts = set(self.offs)
        return [i for i, (s, z) in enumerate(zip(self.mstart, self.msize)) if z and self.first < s < self.n and s not in starts]

    def chunks(self):
        """(start, length) of the pieces bam_index_k stages: from the next record's offset rounded down to 16, IDX_CH bytes or what
        is left; the next piece begins at the first record whose block_size field is not wholly inside this one"""
        out, p = [], self.first
        while p < self.n:
            c0 = p & ~15
            cl = min(self.n - c0, IDX_CH)
            q = p - c0
            while q + 4 <= cl:
                q += 4 + struct.unpack_from("<I", self.stream, c0 + q)[0]
            out.append((c0, cl))
            assert c0 + q > p
            p = c0 + q
        return out

    def field_cut(self, edges):
        """{k}: a record's block_size field has k of its 4 bytes in front of one of `edges`"""
        e = set(edges)
        return sorted({x - o for o in self.offs for x in (o + 1, o + 2, o + 3) if x in e})

    def end_rel(self, edges):
        """{d}: a record ends d bytes behind (negative: in front of) one of `edges`, d in -1, 0, 1"""
        e = set(edges)
        return sorted({d for x in self.ends for d in (-1, 0, 1) if x - d in e})

    def member_edges(self):
        return [s for s, z in zip(self.mstart, self.msize) if z and s > 0]

    def multiples(self):
        return list(range(IDX_CH, self.n + 2, IDX_CH))

    def chunk_ends(self):
        return [c0 + cl for c0, cl in self.chunks()]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, files, recs, tbmerged=None, claims=None, python=True, malformed=False, n_ref=len(REFS)):
        self.name, self.files, self.recs = name, files, recs
        self.tbmerged = np.array(tbmerged if tbmerged is not None else [0] * len(files), np.uint8)
        self.claims = dict(claims or {})
        self.python = python            # bamio.parse_bam reads every record of it as the loaders do
        self.malformed = malformed
        self.n_ref = n_ref

    @property
    def index(self):
        """the record index that must run: the chain as soon as one member of one file begins inside a record"""
        return "chain" if any(layout(f).inside() for f in self.files) else "member"

    @property
    def unplaced(self):
        return any(r.tid < 0 for f in self.recs for r in f)

    def expect(self, oracle_defaults=False):
        """the tile, array for array.  oracle_defaults: the carried tags of files not flagged tbmerged at 0, 1, 0 (what a collapse
        must see of them)"""
        allr = [r for f in self.recs for r in f]
        tbr = [bool(self.tbmerged[i]) for i, f in enumerate(self.recs) for _ in f]
        n = len(allr)

        def offsets(lens):
            o = np.zeros(n + 1, np.uint32)
            o[1:] = np.cumsum(lens, dtype=np.int64)
            return o
        e = {"file_off": np.concatenate([[0], np.cumsum([len(f) for f in self.recs])]).astype(np.uint32),
             "tid": np.array([r.tid for r in allr], np.int32), "pos": np.array([r.pos for r in allr], np.int32),
             "flag": np.array([r.flag for r in allr], np.uint16), "mapq": np.array([r.mapq for r in allr], np.uint8),
             "strand": np.array([ord(r.strand) for r in allr], np.uint8), "nh": np.array([r.nh for r in allr], np.int32),
             "cig_off": offsets([len(r.cig) for r in allr]), "cig": np.array([c for r in allr for c in r.cig], np.uint32),
             "md_off": offsets([len(r.md or b"") for r in allr]),
             "md": np.frombuffer(b"".join(r.md or b"" for r in allr), np.uint8),
             "md_has": np.array([r.md is not None for r in allr], np.uint8),
             "qname_off": offsets([len(r.name) for r in allr]), "qname": np.frombuffer(b"".join(r.name for r in allr), np.uint8),
             "qname_hash": np.array([qname_hash(r.name, r.flag) for r in allr], np.uint64),
             "yc_in": np.array([r.yc if (t or not oracle_defaults) else 0.0 for r, t in zip(allr, tbr)], np.float64),
             "yx_in": np.array([r.yx if (t or not oracle_defaults) else 1 for r, t in zip(allr, tbr)], np.int64),
             "yd_in": np.array([r.yd if (t or not oracle_defaults) else 0 for r, t in zip(allr, tbr)], np.int64),
             "seen": np.array([r.seen for r in allr], np.uint8)}
        return e

    def tb_mask(self):
        """per record: its file is flagged tbmerged"""
        return np.repeat(self.tbmerged.astype(bool), [len(f) for f in self.recs])


def payload(recs, pg=False):
    return header_bytes(pg=pg) + b"".join(r.raw for r in recs)


def one_member(recs, pg=False, level=6):
    """a small file: header and records in one member"""
    p = payload(recs, pg)
    return frame(p, [], level)


def by_member(p, level=6, **kw):
    """the payload framed as htslib would: every member begins with a record"""
    first = bamio.parse_header(p)[1]
    offs, q = [], first
    while q < len(p):
        offs.append(q)
        q += 4 + struct.unpack_from("<I", p, q)[0]
    return frame(p, record_cuts(first, offs, len(p), **kw), level)


@functools.lru_cache(maxsize=None)
def layout(data: bytes) -> Layout:
    return Layout(data)


def _claim_funcs():
    L = layout
    return {
        "inside": lambda s: [L(f).inside() for f in s.files],
        "index": lambda s: s.index,
        "field_cut_member": lambda s: [L(f).field_cut(L(f).member_edges()) for f in s.files],
        "field_cut_48k": lambda s: [L(f).field_cut(L(f).multiples()) for f in s.files],
        "field_cut_chunk": lambda s: [L(f).field_cut(L(f).chunk_ends()) for f in s.files],
        "end_rel_48k": lambda s: [L(f).end_rel(L(f).multiples()) for f in s.files],
        "end_rel_chunk": lambda s: [L(f).end_rel(L(f).chunk_ends()[:-1]) for f in s.files],
        "last_chunk_full": lambda s: [L(f).chunks()[-1][1] == IDX_CH for f in s.files],
        "header_ends_member": lambda s: [L(f).first in L(f).member_edges() for f in s.files],
        "header_members": lambda s: [sum(1 for a, z in zip(L(f).mstart, L(f).msize) if z and a < L(f).first) for f in s.files],
        "first_mid_member": lambda s: [L(f).first not in [0] + L(f).member_edges() for f in s.files],
        "member_sizes_max": lambda s: [max(L(f).msize) for f in s.files],
        "empty_members_mid": lambda s: [sum(1 for z in L(f).msize[:-1] if z == 0) for f in s.files],
        "long_rec_mod16": lambda s: [sorted({o % 16 for o, e in zip(L(f).offs, L(f).ends) if e - o > IDX_CH}) for f in s.files],
        "members_inside_one_record": lambda s: [max([sum(1 for a, z in zip(L(f).mstart, L(f).msize) if z and o < a and a + z <= e)
                                                     for o, e in zip(L(f).offs, L(f).ends)] or [0]) for f in s.files],
        "record_bytes": lambda s: [sorted({e - o for o, e in zip(L(f).offs, L(f).ends)}) for f in s.files],
        "n_records": lambda s: [len(L(f).offs) for f in s.files],
        "impostor": lambda s: [_impostor(L(f)) for f in s.files],
        "stream_bytes_max": lambda s: max(L(f).n for f in s.files),
    }


def _impostor(lay):
    """members that begin inside a record and whose bytes, read as block_size fields from their first byte, are a chain of records
    (>= 32 bytes each) that ends exactly at the member's end"""
    out = []
    for i in lay.inside():
        p, end = lay.mstart[i], lay.mstart[i] + lay.msize[i]
        while p + 4 <= end:
            bs = struct.unpack_from("<I", lay.stream, p)[0]
            if bs < 32:
                break
            p += 4 + bs
        if p == end:
            out.append(i)
    return out


def check_claims(scene):
    """the claims that do not hold, as (name, claimed, found); a claim is one value per file, None where the file is not what the
    claim is about"""
    fn = _claim_funcs()
    bad = []
    for k, v in scene.claims.items():
        got = fn[k](scene)
        ok = got == v
        if isinstance(v, list) and isinstance(got, list) and len(v) == len(got):
            ok = all(a is None or a == b for a, b in zip(v, got))
        if not ok:
            bad.append((k, v, got))
    return bad


class Placer:
    """records laid down at chosen offsets of the inflated stream: filler records (a name, one Z tag of the length needed) take up the
    room between them"""
    MINF = 42

    def __init__(self, header: bytes):
        self.header, self.recs, self.off, self.pos = header, [], len(header), 10

    def add(self, **kw):
        self.pos += 3
        r = Rec(pos=self.pos, **kw)
        self.recs.append(r)
        self.off += len(r.raw)
        return r

    def filler(self, nbytes):
        assert nbytes >= self.MINF, nbytes
        r = self.add(name=b"f", cigar=(), aux=b"ZZZ" + b"x" * (nbytes - self.MINF) + b"\0")
        assert len(r.raw) == nbytes
        return r

    def pad_to(self, target):
        while self.off < target:
            gap = target - self.off
            self.filler(gap if gap < 300 + self.MINF else 300)
        assert self.off == target, (self.off, target)

    def start_at(self, target, **kw):
        self.pad_to(target)
        return self.add(**kw)

    def end_at(self, target, **kw):
        """a record (a filler unless described) whose last byte is just in front of `target`"""
        probe = len(Rec(**kw).raw) if kw else 200
        self.pad_to(target - probe)
        return self.add(**kw) if kw else self.filler(probe)

    def payload(self):
        return self.header + b"".join(r.raw for r in self.recs)


# ---- the tag scan -----------------------------------------------------------------------------------------------------------------
def _tagrec(i, aux, flag=0, **want):
    return Rec(pos=100 + 5 * i, flag=flag, name=b"t%d" % i, cigar=((30, M), (100, N), (20, M)), aux=aux, **want)


def _tagscene(name, cases, tb=0, python=True):
    """cases: (aux bytes, flag, expectation kwargs)"""
    recs = [_tagrec(i, aux, flag, **want) for i, (aux, flag, want) in enumerate(cases)]
    return Scene(name, [one_member(recs, pg=bool(tb))], [recs], [tb], python=python)


I32MIN, I32MAX = -(2**31), 2**31 - 1


def scene_nh_ints():
    c = [(tag("NH", t, v), 0, dict(nh=v)) for t, v in
         (("c", -128), ("c", 127), ("c", 0), ("C", 0), ("C", 255), ("s", -32768), ("s", 32767), ("S", 0), ("S", 65535),
          ("i", I32MIN), ("i", I32MAX), ("i", -1), ("I", 0), ("I", I32MAX))]          # NH:i:INT32_MIN is TBK_NH_ABSENT's value
    c.append((b"", 0, dict()))
    return _tagscene("nh_ints", c)


def scene_nh_wrap():
    """NH:I beyond int32 wraps in the tile's int32 field (the Python decoder keeps it: not its scene)"""
    return _tagscene("nh_wrap", [(tag("NH", "I", 2**31), 0, dict(nh=I32MIN)), (tag("NH", "I", 2**32 - 1), 0, dict(nh=-1)),
                                 (tag("NH", "I", 2**31 + 5), 0, dict(nh=I32MIN + 5))], python=False)


def scene_nh_nonint():
    """NH of a type that is no integer reads as 0 (bam_aux2i) and is the NH of the record: a later NH:C:5 does not count"""
    later = tag("NH", "C", 5)
    firsts = [tag("NH", "f", 1.5), tag("NH", "d", 3.0), tag("NH", "A", "4"), tag("NH", "Z", "7"), tag("NH", "H", "1AE3"),
              tag("NH", "B", ("C", [3, 4])), tag("NH", "B", ("i", []))]
    return _tagscene("nh_nonint", [(f + later, 0, dict(nh=0)) for f in firsts] + [(f, 0, dict(nh=0)) for f in firsts])


def scene_first_wins():
    every = (tag("NH", "C", 3) + tag("XS", "A", "+") + tag("ts", "A", "-") + tag("YC", "f", 2.5) + tag("YX", "C", 4) + tag("YD", "S", 300) +
             tag("MD", "Z", "10A5") +
             tag("NH", "i", 9) + tag("XS", "A", "-") + tag("ts", "A", "+") + tag("YC", "i", 7) + tag("YX", "s", -3) + tag("YD", "c", -1) +
             tag("MD", "Z", "99"))
    full = dict(nh=3, strand="+", md=b"10A5", yc=2.5, yx=4, yd=300, seen=3)
    c = [(every, 0, full),
         (tag("XS", "i", 5) + tag("XS", "A", "+") + tag("ts", "A", "-"), 0, dict(strand="-")),     # the first XS is no strand: ts decides
         (tag("ts", "A", "?") + tag("ts", "A", "+"), 0, dict(strand=".")),
         (tag("MD", "i", 5) + tag("MD", "Z", "7"), 0, dict()),                                       # the first MD is no string: no MD
         (tag("YC", "Z", "5") + tag("YC", "f", 9.0) + tag("YX", "A", "x") + tag("YX", "C", 8), 0, dict(yc=0.0, yx=0, seen=3)),
         (tag("NH", "C", 1) * 2 + tag("YD", "C", 0) + tag("YD", "C", 6), 0, dict(nh=1, yd=0))]
    return _tagscene("first_wins", c, tb=1)


def scene_in_front():
    """fields of every size in front of the tags of interest: a wrong size for any of them moves every tag behind it"""
    tail = tag("NH", "C", 2) + tag("XS", "A", "-") + tag("YC", "C", 3) + tag("YX", "C", 5) + tag("YD", "C", 7) + tag("MD", "Z", "5G4")
    want = dict(nh=2, strand="-", yc=3.0, yx=5, yd=7, md=b"5G4", seen=3)
    c = []
    for sub in "cCsSiIf":
        for cnt in (0, 1, 300):
            vals = [(k % 100) for k in range(cnt)] if sub != "f" else [0.5 * k for k in range(cnt)]
            c.append((tag("XB", "B", (sub, vals)) + tail, 0, want))
    c.append((tag("XD", "d", 2.75) + tag("XH", "H", "00FF") + tag("XE", "Z", "") + tag("XL", "Z", "l" * 600) + tag("XA", "A", "N") + tail, 0, want))
    fixed = (tag("Xc", "c", -1) + tag("XC", "C", 78) + tag("Xs", "s", -2) + tag("xs", "S", 72) + tag("Xi", "i", -3) + tag("XI", "I", 2**32 - 1) +
             tag("Xf", "f", 1.5) + tag("Xa", "A", "N"))                                               # (every fixed size; "xs" is not XS)
    c.append((fixed + tail, 0, want))
    for one in (tag("Xi", "i", 0x484E), tag("XI", "I", 0x484E4848), tag("Xf", "f", 0.0), tag("Xs", "s", 0x484E), tag("xs", "S", 1), tag("Xc", "c", 78)):
        c.append((one + tail, 0, want))
    # names one byte or one case away from a tag of interest, each with a value that would show
    near = (tag("Nh", "C", 9) + tag("nH", "C", 9) + tag("XT", "A", "+") + tag("tS", "A", "+") + tag("Yc", "C", 9) + tag("yX", "C", 9) +
            tag("YE", "C", 9) + tag("Md", "Z", "77") + tag("NI", "C", 9) + tag("XR", "A", "+"))
    c.append((near + tail, 0, want))
    c.append((near, 0, dict()))
    c.append((tag("XZ", "Z", b"NHC\x07") + tail, 0, want))                                           # tag-like bytes inside a string
    c.append((tag("XZ", "Z", b"NHC\x07"), 0, dict()))
    c.append((tag("XH", "H", b"XSA+") + tag("XB", "B", ("C", list(b"NHC\x09tsA+"))) + tail, 0, want))
    return _tagscene("in_front", c, tb=1)


def scene_strand():
    c = [(tag("XS", "Z", "") + tag("ts", "A", "+"), 0, dict(strand="+")),                            # empty XS:Z: ts decides
         (tag("XS", "Z", "") + tag("ts", "A", "+"), 16, dict(strand="-")),
         (tag("XS", "Z", ""), 0, dict()),
         (tag("XS", "Z", "+x"), 0, dict(strand="+")), (tag("XS", "Z", "-q"), 16, dict(strand="-")),
         (tag("XS", "i", 5), 0, dict()), (tag("XS", "i", 43), 0, dict()), (tag("XS", "i", 5) + tag("ts", "A", "-"), 0, dict(strand="-")),
         (tag("ts", "A", "+"), 16, dict(strand="-")), (tag("ts", "A", "-"), 16, dict(strand="+")), (tag("ts", "A", "+"), 0, dict(strand="+")),
         (tag("ts", "A", "-"), 0, dict(strand="-")), (tag("ts", "Z", "+"), 0x10 | 0x1, dict(strand="-")), (tag("ts", "C", 43), 0, dict()),
         (tag("XS", "A", ".") + tag("ts", "A", "+"), 0, dict()), (tag("XS", "A", "*") + tag("ts", "A", "-"), 0, dict()),
         (tag("ts", "A", "-") + tag("XS", "A", "+"), 16, dict(strand="+")),                          # XS wins wherever it stands
         (tag("XS", "A", "+"), 16, dict(strand="+")), (tag("XS", "A", "-"), 0, dict(strand="-")), (tag("ts", "A", "?"), 0, dict())]
    return _tagscene("strand", c)


def _carried_cases():
    c = [(tag("YC", "f", 2.5), dict(yc=2.5, seen=1)), (tag("YC", "f", 0.0), dict(yc=0.0, seen=1)), (tag("YC", "d", 1e10 + 0.5), dict(yc=1e10 + 0.5, seen=1)),
         (tag("YC", "f", 16777217.0), dict(yc=16777216.0, seen=1)),                                 # (a float's precision, not a double's)
         (tag("YC", "c", -3), dict(yc=-3.0, seen=1)), (tag("YC", "C", 200), dict(yc=200.0, seen=1)), (tag("YC", "s", -300), dict(yc=-300.0, seen=1)),
         (tag("YC", "S", 60000), dict(yc=60000.0, seen=1)), (tag("YC", "i", -70000), dict(yc=-70000.0, seen=1)),
         (tag("YC", "I", 3000000000), dict(yc=3e9, seen=1)), (tag("YC", "A", "x"), dict(yc=0.0, seen=1)), (tag("YC", "Z", "5"), dict(yc=0.0, seen=1)),
         (tag("YC", "B", ("f", [4.0])), dict(yc=0.0, seen=1))]
    for t, v in (("c", -1), ("C", 1), ("C", 255), ("s", -32768), ("S", 65535), ("i", I32MIN), ("I", 2**32 - 1)):
        c.append((tag("YX", t, v), dict(yx=v, seen=2)))
        c.append((tag("YD", t, v), dict(yd=v)))
    c.append((tag("YX", "f", 3.0) + tag("YD", "Z", "4"), dict(yx=0, yd=0, seen=2)))
    c.append((tag("NH", "C", 2) + tag("YC", "f", 7.0) + tag("YX", "S", 300) + tag("YD", "C", 2), dict(nh=2, yc=7.0, yx=300, yd=2, seen=3)))
    c.append((b"", dict()))
    c.append((tag("NH", "C", 1), dict(nh=1)))
    return c


def scene_carried():
    """the same records in a TieBrush-merged file and in a plain one, one call: the plain file's carried tags are not read"""
    def recs():
        return [_tagrec(i, aux, 0, **want) for i, (aux, want) in enumerate(_carried_cases())]
    a, b = recs(), recs()
    return Scene("carried", [one_member(a, pg=True), one_member(b)], [a, b], [1, 0])


def scene_md():
    big = (b"12A7^ACGT3T" * 80)[:777]
    c = [(tag("MD", "Z", ""), 0, dict(md=b"")), (tag("MD", "Z", big), 0, dict(md=big)), (tag("MD", "Z", "50"), 0, dict(md=b"50")),
         (tag("MD", "i", 5), 0, dict()), (tag("MD", "A", "5") + tag("MD", "Z", "8"), 0, dict()), (tag("MD", "H", "AB"), 0, dict()),
         (tag("XB", "B", ("i", list(range(300)))) + tag("XC", "B", ("c", [])) + tag("MD", "Z", "3C3"), 0, dict(md=b"3C3")),
         (tag("NH", "C", 4) + tag("XB", "B", ("S", [1, 2, 3])) + tag("MD", "Z", "1"), 0, dict(nh=4, md=b"1")),
         (b"", 0, dict()), (tag("MD", "Z", "") + tag("MD", "Z", "33"), 0, dict(md=b"")), (tag("MD", "Z", "9"), 0, dict(md=b"9"))]
    return _tagscene("md", c)


def _bad_bytes():
    """bytes no aux field begins with: the scan stops at them"""
    return {"unknown_type": b"XXq\x01\x02\x03\x04", "B_of_d": b"XBBd" + struct.pack("<Id", 1, 1.0), "B_of_A": b"XBBA" + struct.pack("<I", 2) + b"ab",
            "B_count_past": b"XBBi" + struct.pack("<I", 1000) + b"\x01\0\0\0\x02\0\0\0", "B_cut": b"XBBi\x01", "Z_no_nul": b"XZZabc",
            "stray_1": b"X", "stray_2": b"XY", "i_cut": b"XIi\x01\x02", "d_cut": b"XDd\x01\x02\x03\x04\x05\x06\x07", "s_cut": b"XSs\x01",
            "A_cut": b"XAA", "B_max_count": b"XBBC" + struct.pack("<I", 0xFFFFFFFF) + b"\x01\x02"}


def scene_bad_behind():
    """bad bytes behind good tags: the tags in front count, the record is no error"""
    good = tag("NH", "C", 3) + tag("XS", "A", "+") + tag("YX", "C", 6) + tag("MD", "Z", "12")
    want = dict(nh=3, strand="+", yx=6, md=b"12", seen=2)
    return _tagscene("bad_behind", [(good + b, 0, want) for b in _bad_bytes().values()], tb=1, python=False)


def scene_bad_front():
    """the same bytes in front: what stands behind them is not read as tags (where the bad bytes swallow some of what follows and the
    scan goes on, nothing of interest is left either)"""
    nul_free = tag("NH", "C", 3) + tag("XS", "A", "+") + tag("YC", "C", 6)
    with_md = nul_free + tag("MD", "Z", "12")
    c = []
    for b in _bad_bytes().values():
        c.append((b + nul_free, 0, dict()))
        c.append((b + with_md, 0, dict()))
    return _tagscene("bad_front", c, tb=1, python=False)


# ---- core fields and the fill -----------------------------------------------------------------------------------------------------
def scene_sizes():
    nref = len(REFS)
    recs = [Rec(pos=10, name=b"", cigar=()),                                                        # 37 bytes: the shortest record there is
            Rec(pos=11, name=b"a", cigar=(), l_seq=1), Rec(pos=12, name=b"n" * 254, l_seq=7), Rec(pos=13, name=b"e", l_seq=8, aux=tag("NH", "C", 1), nh=1),
            Rec(pos=14, name=b"z", cigar=(), l_seq=0, aux=tag("XS", "A", "-"), strand="-"), Rec(pos=15, flag=0xFFFF, mapq=255, name=b"all", aux=tag("ts", "A", "+"), strand="-"),
            Rec(pos=16, mtid=nref - 1, mpos=5, tlen=-7, name=b"mate", cigar=((5, S), (20, M), (3, I), (7, D), (20, M))),
            Rec(tid=nref - 1, pos=0, mapq=0, name=b"lastref", l_seq=63, cigar=((63, M),)),
            Rec(tid=nref - 1, pos=2**29 - 2, name=b"far", cigar=((1, M),), l_seq=129),
            Rec(tid=-1, pos=-1, flag=4, mapq=0, name=b"un", cigar=(), l_seq=3), Rec(tid=-1, pos=-1, flag=4, name=b"", cigar=())]
    p = payload(recs)
    return Scene("sizes", [by_member(p)], [recs], claims={"index": "member", "record_bytes": [sorted({len(r.raw) for r in recs})]})


def scene_cigar_max():
    """65535 CIGAR operations: 256 KiB of one record, through five members"""
    ops = tuple((1 + (i % 7), (M, I, M, D, M, N)[i % 6]) for i in range(65535))
    recs = [Rec(pos=10, name=b"before", aux=tag("NH", "C", 2), nh=2), Rec(pos=11, name=b"maxcig", cigar=ops, aux=tag("NH", "C", 1) + tag("MD", "Z", "7"), nh=1, md=b"7"),
            Rec(pos=12, name=b"after", aux=tag("XS", "A", "+"), strand="+")]
    p = payload(recs)
    cuts = list(range(60000, len(p), 60000))
    return Scene("cigar_max", [frame(p, cuts)], [recs], claims={"index": "chain", "members_inside_one_record": [3]})


def scene_qhash():
    recs = [Rec(pos=10 + i, flag=fl, name=nm) for i, (fl, nm) in enumerate(
        [(0x40, b"read/pair"), (0x80, b"read/pair"), (0xC0, b"read/pair"), (0, b"read/pair"), (0x1 | 0x10, b"read/pair"), (0, b"read/paiq"), (0, b"read/pai"),
         (0x40, b""), (0x80, b""), (0, b"\xff\x80\x01")])]
    assert len({qname_hash(r.name, r.flag) for r in recs}) == len(recs) - 2                           # (0x40 | 0x80 hashes as 0x40, 0x11 as no flag)
    return Scene("qhash", [one_member(recs)], [recs])


def scene_min3000(n=3000):
    """the densest a 48 KiB chunk and the record table can be: records of 37 bytes"""
    recs = [Rec(pos=7, name=b"", cigar=(), flag=(0x40 if i % 3 == 0 else 0), mapq=i % 256) for i in range(n)]
    p = payload(recs)
    return Scene("min3000", [by_member(p)], [recs], claims={"index": "member", "record_bytes": [[37]], "n_records": [n]})


def _plain(n, base, tagged=True, **kw):
    return [Rec(pos=base + 4 * i, name=b"p%d" % i, cigar=((25, M), (60 + i % 3, N), (25, M)), aux=tag("NH", "C", 1 + i % 2) if tagged else b"",
                nh=(1 + i % 2) if tagged else NH_ABSENT, **kw) for i in range(n)]


def scene_empty_between():
    """a file with a header and no record between two files with records, and an empty TieBrush-merged file behind them"""
    a, b = _plain(5, 100), _plain(7, 300)
    return Scene("empty_between", [one_member(a), one_member([]), one_member(b), one_member([], pg=True)], [a, [], b, []], [0, 0, 0, 1])


def scene_all_empty():
    return Scene("all_empty", [one_member([]), one_member([], pg=True)], [[], []], [0, 1])


# ---- the record index -------------------------------------------------------------------------------------------------------------
def _two_framings(name, p, recs, hand_cuts, claims_member, claims_hand, member_kw=None):
    """the same payload as htslib would frame it and cut by hand"""
    return [Scene(name + "/member", [by_member(p, **(member_kw or {}))], [recs], claims=dict(claims_member, index="member")),
            Scene(name + "/hand", [frame(p, hand_cuts, level=1)], [recs], claims=dict(claims_hand, index="chain"))]


def scenes_field_cut_member():
    """a block_size field cut 1 | 3, 2 | 2 and 3 | 1 by a member's end; the header ends exactly at a member's end"""
    recs = _plain(60, 100)
    p = payload(recs)
    lay_first = len(header_bytes())
    offs = np.concatenate([[0], np.cumsum([len(r.raw) for r in recs])])[:-1] + lay_first
    cuts = [lay_first, int(offs[10]) + 1, int(offs[25]) + 2, int(offs[40]) + 3]
    return _two_framings("field_cut_member", p, recs, cuts, {"field_cut_member": [[]], "header_ends_member": [True], "inside": [[]]},
                         {"field_cut_member": [[1, 2, 3]], "header_ends_member": [True], "inside": [[2, 3, 4]]}, dict(limit=1500))


def scenes_field_cut_48k():
    """a block_size field cut 1 | 3, 2 | 2, 3 | 1 by a multiple of 48 KiB of the stream (file 0) and by the end of a chunk as the chain
    kernel cuts them (file 1: every chunk begins at the record the one before could not finish, rounded down to 16)"""
    a = Placer(header_bytes())
    for m, k in ((1, 1), (2, 2), (3, 3)):
        a.start_at(m * IDX_CH - k, name=b"cut%d" % k, aux=tag("NH", "C", k), nh=k)
    a.pad_to(3 * IDX_CH + 500)
    b = Placer(header_bytes())
    e = (len(b.header) & ~15) + IDX_CH
    for k in (1, 2, 3):
        b.start_at(e - k, name=b"cut%d" % k, aux=tag("NH", "C", k), nh=k)
        e = ((e - k) & ~15) + IDX_CH
    b.pad_to(e + 500)
    pa, pb = a.payload(), b.payload()
    # by hand: cuts of 50000 bytes; file 1's chunk ends stay where they are (they depend on the stream alone)
    hand = lambda p: frame(p, list(range(50000, len(p), 50000)))
    cl = {"field_cut_48k": [[1, 2, 3], None], "field_cut_chunk": [None, [1, 2, 3]]}
    return [Scene("field_cut_48k/member", [by_member(pa), by_member(pb)], [a.recs, b.recs], claims=dict(cl, index="member")),
            Scene("field_cut_48k/hand", [hand(pa), hand(pb)], [a.recs, b.recs], claims=dict(cl, index="chain"))]


def scenes_end_48k():
    """records ending exactly on, 1 byte in front of and 1 byte behind a multiple of 48 KiB (file 0) and a chunk's end (file 1); file 2's
    stream ends exactly where a full chunk ends"""
    a = Placer(header_bytes())
    for m, d in ((1, 0), (2, -1), (3, 1)):
        a.end_at(m * IDX_CH + d)
        a.pad_to(m * IDX_CH + d)
    a.pad_to(3 * IDX_CH + 700)
    b = Placer(header_bytes())
    e = (len(b.header) & ~15) + IDX_CH
    b.end_at(e)
    b.pad_to(e)                      # ends on the chunk's end: the next chunk begins there
    e += IDX_CH
    b.end_at(e - 1)
    b.pad_to(e - 1)                  # 1 in front: the next record's field is cut 1 | 3, the next chunk begins 16 in front of e
    e = e - 16 + IDX_CH
    b.end_at(e + 1)
    b.pad_to(e + 1)                  # 1 behind
    b.pad_to(e + 900)
    c = Placer(header_bytes())
    e = (len(c.header) & ~15) + 2 * IDX_CH
    c.end_at(e - IDX_CH)
    c.pad_to(e - IDX_CH)
    c.end_at(e)
    c.pad_to(e)
    ps = [a.payload(), b.payload(), c.payload()]
    recs = [a.recs, b.recs, c.recs]
    hand = lambda p: frame(p, list(range(40001, len(p), 40001)))
    cl = {"end_rel_48k": [[-1, 0, 1], None, None], "end_rel_chunk": [None, [-1, 0, 1], None], "last_chunk_full": [None, None, True]}
    return [Scene("end_48k/member", [by_member(p) for p in ps], recs, claims=dict(cl, index="member")),
            Scene("end_48k/hand", [hand(p) for p in ps], recs, claims=dict(cl, index="chain"))]


def scenes_long_record():
    """records of about 50 KB, longer than a chunk of the chain kernel, beginning 0, 15, 1 and 8 bytes behind a multiple of 16"""
    a = Placer(header_bytes())
    base = 1024
    for j, m in enumerate((0, 15, 16, 1, 8)):
        base = (a.off + 200 + 15) & ~15
        a.start_at(base + m, name=b"long%d" % j, l_seq=33000 + j, aux=tag("NH", "C", j + 1) + tag("MD", "Z", "33000"), nh=j + 1, md=b"33000")
    a.pad_to(a.off + 400)
    p = a.payload()
    cl = {"long_rec_mod16": [[0, 1, 8, 15]]}
    return _two_framings("long_record", p, a.recs, list(range(30000, len(p), 30000)), cl, cl)


def scenes_huge_record():
    """a record of about 100 KB (l_seq 66000): whole members lie inside it, however the file is framed; the chain runs either way"""
    a = Placer(header_bytes())
    a.pad_to(3000)
    a.add(name=b"huge", l_seq=66000, cigar=((66000, M),), aux=tag("NH", "C", 1) + tag("XS", "A", "+") + tag("MD", "Z", "66000"), nh=1, strand="+", md=b"66000")
    a.pad_to(a.off + 2000)
    p = a.payload()
    cuts1 = [3000] + list(range(3000 + 30000, len(p), 30000))          # a member begins with the record; three lie inside it
    cuts2 = list(range(2000, len(p), 45000))
    return [Scene("huge_record/a", [frame(p, cuts1)], [a.recs], claims={"index": "chain", "members_inside_one_record": [2]}),
            Scene("huge_record/b", [frame(p, cuts2)], [a.recs], claims={"index": "chain", "members_inside_one_record": [1]})]


def _many_refs(n=820):
    return tuple(("contig_%04d_" % i + "abcdefghij" * 7, 1000 + i) for i in range(n))


def scenes_big_header():
    """a header of 150 KB (many @SQ lines with long names): through three members, the first record in the middle of the third"""
    refs = _many_refs()
    nref = len(refs)
    recs = [Rec(tid=0, pos=5, name=b"h0", aux=tag("NH", "C", 1), nh=1), Rec(tid=1, pos=6, name=b"h1", mtid=nref - 1, mpos=3),
            Rec(tid=nref - 1, pos=7, name=b"h2", mtid=0, mpos=9), Rec(tid=nref - 1, pos=9, name=b"h3", aux=tag("XS", "A", "-"), strand="-")]
    recs += [Rec(tid=nref - 1, pos=20 + i, name=b"h%d" % (4 + i)) for i in range(40)]
    p = header_bytes(refs=refs) + b"".join(r.raw for r in recs)
    first = len(header_bytes(refs=refs))
    assert 150000 <= first < 3 * 0xFF00
    cl = {"header_members": [3], "first_mid_member": [True]}
    hand = [50000, 100000, first + 100, first + 1000]
    return [Scene("big_header/member", [by_member(p, header_alone=False)], [recs], claims=dict(cl, index="member"), n_ref=nref),
            Scene("big_header/hand", [frame(p, hand)], [recs], claims=dict(cl, index="chain"), n_ref=nref)]


def scenes_member_edges():
    """empty members (ISIZE 0) in the middle of the file and a member of exactly 65536 payload bytes"""
    a = Placer(header_bytes())
    first = a.off
    a.pad_to(first + 65536)
    a.pad_to(first + 65536 + 3000)
    p = a.payload()
    offs = np.cumsum([first] + [len(r.raw) for r in a.recs])
    later = int(offs[np.searchsorted(offs, first + 65536 + 1500)])           # (a record boundary: every member begins with a record)
    m_cuts = [first, first, first + 65536, first + 65536, first + 65536, later]
    h_cuts = [first + 10, first + 10, first + 10 + 65536, first + 10 + 65536, first + 10 + 65536 + 700]
    cl = {"member_sizes_max": [65536]}
    return [Scene("member_edges/member", [frame(p, m_cuts)], [a.recs], claims=dict(cl, index="member", empty_members_mid=[3], inside=[[]])),
            Scene("member_edges/hand", [frame(p, h_cuts)], [a.recs], claims=dict(cl, index="chain", empty_members_mid=[2]))]


def scene_impostor():
    """The member walk's adversary.  A record's SEQ / QUAL bytes are themselves well-formed records, and a member begins at the first
    of them and ends with the record: walked from its first byte, that member looks like any other.  Only the member in front, whose
    last record runs past its end, shows that the file needs the chain; the tile is the chain's (one record, not the five inside it)."""
    fakes = b"".join(Rec(pos=900 + i, name=b"fake%d" % i, aux=tag("NH", "C", 9)).raw for i in range(5))
    lead = b"\x21" * (3 - len(fakes) % 3 + 30)                      # SEQ + QUAL of l_seq bases are 3 l_seq / 2 bytes (l_seq even)
    sq = lead + fakes
    assert len(sq) % 3 == 0
    before, after = _plain(6, 100), _plain(6, 400)
    host = Rec(pos=200, name=b"host", l_seq=2 * len(sq) // 3, seqqual=sq, cigar=((40, M),))
    assert host.raw.endswith(fakes)
    recs = before + [host] + after
    p = payload(recs)
    first = len(header_bytes())
    o_host = first + sum(len(r.raw) for r in before)
    b0 = o_host + len(host.raw) - len(fakes)
    b1 = o_host + len(host.raw) + sum(len(r.raw) for r in after[:2])
    return Scene("impostor", [frame(p, [first, b0, b1])], [recs], claims={"index": "chain", "inside": [[2]], "impostor": [[2]], "n_records": [13]})


# ---- one of everything, for the collapse and the command line ------------------------------------------------------------------------
def scene_mixed(tb=False):
    """two sorted files with duplicates across and within them, tags of every width, arrays in front of NH, both strands and carried
    tags (read when the first file is TieBrush-merged, tb, and not otherwise); file 0 cut by hand, file 1 framed by record"""
    def one(f):
        recs = []
        for i in range(420):
            pos = 1000 + 40 * (i // 3) + (0 if f == 0 else (i % 2))
            tid = 0 if i < 300 else 1
            cig = ((20 + i % 2, M), (100 + (i // 3) % 4, N), (30, M)) if i % 5 else ((51, M),)
            nhv = 1 + i % 3
            st = "+-."[i % 3]
            aux = b""
            if i % 4 == 0:
                aux += tag("XB", "B", ("sSiIfcC"[i % 7], [1] * (i % 9)))
            aux += tag("NH", "CSsIic"[i % 6], nhv)
            if st != ".":
                aux += tag("XS", "A", st) if i % 2 else tag("ts", "A", st)
            want = dict(nh=nhv, strand=st)
            if i % 6 == 1:
                aux += tag("YC", "f", 2.0 + i % 4) + tag("YX", "C", 1 + i % 3) + tag("YD", "C", i % 2)
                want.update(yc=2.0 + i % 4, yx=1 + i % 3, yd=i % 2, seen=3)
            aux += tag("MD", "Z", "%d" % (50 + i % 2))
            recs.append(Rec(tid=tid, pos=pos, name=b"m%d_%d" % (f, i), cigar=cig, aux=aux, l_seq=50 + i % 2, md=b"%d" % (50 + i % 2), **want))
        recs.sort(key=lambda r: (r.tid, r.pos))
        return recs
    a, b = one(0), one(1)
    pa, pb = payload(a, pg=tb), payload(b)
    return Scene("mixed_tb" if tb else "mixed", [frame(pa, list(range(7777, len(pa), 7777))), by_member(pb, limit=9000)], [a, b], [1 if tb else 0, 0],
                 claims={"index": "chain"})


# ---- malformed --------------------------------------------------------------------------------------------------------------------
MALFORMED_KINDS = ("block_size_31", "block_size_past_file", "trailing_bytes", "l_read_name_0", "name_no_nul", "l_read_name_past", "n_cigar_past",
                   "l_seq_negative", "l_seq_past", "tid_n_ref", "tid_minus_2", "mtid_n_ref", "bad_magic", "l_text_past", "ref_names_past", "only_eof")
MALFORMED_STAGE = {"block_size_31": "chain", "block_size_past_file": "chain", "trailing_bytes": "chain", "bad_magic": "header", "l_text_past": "header",
                   "ref_names_past": "header", "only_eof": "header"}         # every other kind: bam_fields_k
POSITIONS = ("first", "middle", "last")


def _mutate(raw: bytearray, kind, o, pos_index):
    """raw: the inflated file; o: offset of the victim's block_size field"""
    r = o + 4
    bs = struct.unpack_from("<I", raw, o)[0]
    if kind == "block_size_31":
        raw[o:o + 4] = struct.pack("<I", 31)
    elif kind == "block_size_past_file":
        raw[o:o + 4] = struct.pack("<I", len(raw) - o - 4 + 1)
    elif kind == "trailing_bytes":
        raw += b"\x25\0\0"[:pos_index + 1]                            # 1, 2 or 3 bytes: not even a block_size field
    elif kind == "l_read_name_0":
        raw[r + 8] = 0
    elif kind == "name_no_nul":
        raw[r + 32 + raw[r + 8] - 1] = ord("x")
    elif kind == "l_read_name_past":
        raw[r + 8] = 255
        assert 32 + 255 > bs
    elif kind == "n_cigar_past":
        raw[r + 12:r + 14] = struct.pack("<H", 60000)
    elif kind == "l_seq_negative":
        raw[r + 16:r + 20] = struct.pack("<i", -5)
    elif kind == "l_seq_past":
        raw[r + 16:r + 20] = struct.pack("<i", bs)
    elif kind == "tid_n_ref":
        raw[r:r + 4] = struct.pack("<i", len(REFS))
    elif kind == "tid_minus_2":
        raw[r:r + 4] = struct.pack("<i", -2)
    elif kind == "mtid_n_ref":
        raw[r + 20:r + 24] = struct.pack("<i", len(REFS))
    elif kind == "bad_magic":
        raw[3] = 2
    elif kind == "l_text_past":
        raw[4:8] = struct.pack("<i", len(raw))
    elif kind == "ref_names_past":
        first = bamio.parse_header(bytes(raw))[1]
        l_last = len(REFS[-1][0]) + 1
        raw[first - 8 - l_last:first - 4 - l_last] = struct.pack("<i", len(raw))   # l_name of the last reference
    else:
        raise KeyError(kind)


def scene_malformed(kind, position):
    """three files of 120 records; the bad record is the tile's first, the last, or one in the middle of the second file (the bad
    header: the first, the last or the second file's).  Every other byte is as in good_scene()."""
    per = 120
    recs = [_plain(per, 100 + 1000 * f, l_seq=20) for f in range(3)]
    f = POSITIONS.index(position)
    i = {"first": 0, "middle": per // 2, "last": per - 1}[position]
    files = []
    for g in range(3):
        raw = bytearray(payload(recs[g]))
        if g == f:
            if kind == "only_eof":
                files.append(bamio._BGZF_EOF)
                continue
            o = len(header_bytes()) + sum(len(r.raw) for r in recs[g][:i])
            _mutate(raw, kind, o, f)
        by_record = g != f or (kind not in MALFORMED_STAGE and position != "middle")     # (a chain that still holds can be framed by it)
        files.append(by_member(bytes(raw), limit=3000) if by_record else frame(bytes(raw), list(range(3000, len(raw), 3000))))
    return Scene("bad/%s/%s" % (kind, position), files, recs, malformed=True)


def good_scene():
    recs = [_plain(120, 100 + 1000 * f, l_seq=20) for f in range(3)]
    return Scene("good", [by_member(payload(r), level=lv, limit=3000) for r, lv in zip(recs, (0, 6, 9))], recs, claims={"index": "member"})


# ---- the lists the tests go through ---------------------------------------------------------------------------------------------------
TAG_SCENES = (scene_nh_ints, scene_nh_wrap, scene_nh_nonint, scene_first_wins, scene_in_front, scene_strand, scene_carried, scene_md,
              scene_bad_behind, scene_bad_front)
CORE_SCENES = (scene_sizes, scene_cigar_max, scene_qhash, scene_min3000, scene_empty_between)
INDEX_SCENES = (scenes_field_cut_member, scenes_field_cut_48k, scenes_end_48k, scenes_long_record, scenes_huge_record, scenes_big_header,
                scenes_member_edges)

_CACHE = {}


def well_formed():
    """every well-formed scene with at least one record, by name (built once)"""
    if "wf" not in _CACHE:
        out = [f() for f in TAG_SCENES + CORE_SCENES]
        for f in INDEX_SCENES:
            out += f()
        out += [scene_impostor(), scene_mixed(False), scene_mixed(True), good_scene()]
        _CACHE["wf"] = {s.name: s for s in out}
    return _CACHE["wf"]


def malformed():
    if "bad" not in _CACHE:
        _CACHE["bad"] = {s.name: s for s in (scene_malformed(k, p) for k in MALFORMED_KINDS for p in POSITIONS)}
    return _CACHE["bad"]
