"""Hand-built output records for the record layer of the output writer (bgzdef.hip: enc_plan_k, enc_emit_k, enc_maxlen_k, enc_strip_k,
enc_cuts_k, enc_members_k) and its consumer in the index (baix.hip: ix_rec_k).  Scene builders only: numpy, struct, bamio's record
encoder and the model (enc_model.py); importable without a GPU and without pytest.

A scene is a function that returns (records, yc, yx, yd, ref_len, claims): raw records without block_size in coordinate order on
reference 0, the tag values of each, the reference lengths an index of them needs, and `claims`: facts about the input, computed with
the model, that make the scene what its name says.  check_claims() computes each of them again.  Lengths called "tagged" include the
record's 4-byte block_size; L is a scene's longest tagged record, B = 0xff00 - L the span in which a member's records begin.

The constants the scenes are placed against are the code's: 0xff00 payload bytes a member, the 256-byte margin (so 65024 is the longest
record the encoder takes), 16 lanes per record in the fresh-record copy and in the CIGAR sum, the widths' boundaries of an integer tag."""
import struct

import numpy as np

import enc_model as em
from tiebrush_amd import bamio

M, I, D, N, S, H, P, EQ, X = range(9)
CONSUMES = (M, D, N, EQ, X)
REF_LEN = [1 << 22]
WINDOW = 1 << 14


def ref_span(cigar):
    return sum(l for l, o in cigar if o in CONSUMES)


def sized(raw_len, pos, name=b"r", cigar=((50, M),), aux=b""):
    """a record of exactly raw_len bytes: the sequence takes up what the name, the CIGAR and the aux bytes leave (with a 4-byte pad tag
    in front of the aux bytes when the rest is no length SEQ + QUAL can have)"""
    rest = raw_len - 32 - (len(name) + 1) - 4 * len(cigar) - len(aux)
    if rest % 3 == 1:
        aux, rest = b"XPAp" + aux, rest - 4
    assert rest >= 0, raw_len
    l_seq = 2 * rest // 3 if rest % 3 == 0 else (2 * rest - 1) // 3
    sq = bytes((17 * i + 3) & 0xFF for i in range((l_seq + 1) // 2)) + bytes(30 + i % 11 for i in range(l_seq))
    r = bamio.encode_record(0, pos, 0, 60, [(l << 4) | o for l, o in cigar], name, aux=aux, l_seq=l_seq, seq=sq)[4:]
    assert len(r) == raw_len, (len(r), raw_len)
    return r


FRESH_TAGS = 15                    # block_size + YC:f + YX:C of a fresh record with a small YX and no YD


def plain(tagged_len, pos, **kw):
    """a fresh record whose tagged length (YC, a YX below 255, no YD) is tagged_len"""
    return sized(tagged_len - FRESH_TAGS, pos, **kw)


def _scene(records, ref_len=None, yc=None, yx=None, yd=None):
    n = len(records)
    return (records, [2.0 + i % 5 for i in range(n)] if yc is None else list(yc), [1 + i % 200 for i in range(n)] if yx is None else list(yx),
            [0] * n if yd is None else list(yd), list(ref_len or REF_LEN))


def lengths(scene):
    return em.tagged_lengths(*scene[:4])


# ---- member cuts ----------------------------------------------------------------------------------------------------------------------
ON_CUT_T, ON_CUT_N = 1020, 190     # 0xff00 = 64 * 1020: B = 63 records exactly


def on_the_cut(first=0):
    """equal records whose tagged length divides B: the records 63 k begin at k B exactly.  first = +1 / -1: the first record one byte
    longer / shorter by its name, and no later record begins on a multiple of B"""
    recs = [plain(ON_CUT_T + (first if i == 0 else 0), 100 + 10 * i, name=b"c" * (6 + (first if i == 0 else 0))) for i in range(ON_CUT_N)]
    sc = _scene(recs)
    return sc + ({"on_cut": [63, 126, 189] if first == 0 else [], "B": 0xFF00 - ON_CUT_T - (first == 1), "written": 3 if first == -1 else 4,
                  "empty": 1 if first == -1 else 0},)     # (shorter: the last record begins one byte in front of 3 B, so nothing begins in the last range)


def _shorts(k, pos0, tag):
    bare, named = (48, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60), (53, 55, 56, 57, 58, 59, 60)   # (tagged lengths SEQ + QUAL can fill)
    return [plain(bare[(7 * i) % 12], pos0 + 10 * i, name=b"", cigar=()) if i % 3 else plain(named[i % 7], pos0 + 10 * i, name=tag, cigar=((30, M),))
            for i in range(k)]


def long_between_short(where="middle"):
    """one record of tagged length 65024, the longest accepted, among 60 records of 48 to 60 bytes: B = 256, and some 250 ranges lie
    inside the long record"""
    a, b = {"first": (0, 60), "middle": (30, 30), "last": (60, 0)}[where]
    recs = _shorts(a, 100, b"a") + [plain(em.LONGEST, 1000, name=b"long", cigar=((40000, M),))] + _shorts(b, 2000, b"b")
    sc = _scene(recs)
    return sc + ({"B": 256, "L": em.LONGEST, "empty_min": 250, "payload_at_most": 0xFF00 - 1, "empty": 254, "written": 14},)


FULL_L, FULL_F = 30000, 980        # B = 35280 = 36 * 980


def fullest_member():
    """member 1 begins with the record at B and ends with a record of L bytes that begins at 2 B - 1: B - 1 + L = 0xff00 - 1 bytes, the
    largest payload the cut rule allows"""
    sizes = [FULL_F] * 36 + [FULL_F] * 35 + [FULL_F - 1] + [FULL_L] + [FULL_F] * 3
    recs = [plain(t, 100 + 10 * i, name=b"f%d" % (i % 10)) for i, t in enumerate(sizes)]
    sc = _scene(recs)
    return sc + ({"B": 0xFF00 - FULL_L, "L": FULL_L, "fullest": (1, 0xFF00 - 1), "written": 3, "payload_at_most": 0xFF00 - 1},)


def one_record(long=False):
    recs = [plain(em.LONGEST, 100, name=b"only", cigar=((40000, M),)) if long else plain(48, 100, name=b"", cigar=())]
    sc = _scene(recs)
    return sc + ({"L": em.LONGEST if long else 48, "written": 1, "empty": 253 if long else 0},)


MIXED_LONG = 63500


def mixed_sizes(seed=5):
    """300 records, lengths drawn by seed from minimal, about 1 kB and about 20 kB — and one long read of 63.5 kB among them: no range can be
    empty unless a record is longer than B, and B is at least 45 kB while the longest record has 20 kB"""
    rng = np.random.default_rng(seed)
    kind = rng.choice(3, 299, p=[0.92, 0.08, 0.0])
    kind[rng.choice(299, 3, replace=False)] = 2                      # (three of the 20 kB records whatever the draw)
    at = int(rng.integers(100, 200))
    recs = []
    for i in range(300):
        k = 3 if i == at else int(kind[i - (i > at)])
        t = (48, 1000 + int(rng.integers(0, 60)), 20000 + int(rng.integers(0, 300)), MIXED_LONG)[k]
        recs.append(plain(t, 100 + 10 * i, name=b"" if k == 0 else b"m%d" % i, cigar=() if k == 0 else ((60, M),)))
    sc = _scene(recs)
    return sc + ({"L": MIXED_LONG, "B": 0xFF00 - MIXED_LONG, "empty_min": 1, "written_min": 20, "n": 300},)


def one_over():
    """tagged length 65025: one byte more than the encoder takes"""
    sc = _scene([plain(em.LONGEST + 1, 100, name=b"over", cigar=((40000, M),))])
    return sc + ({"L": em.LONGEST + 1, "refused": True},)


def tags_push_it_over():
    """a fresh record whose raw bytes and block_size fit (65020) and whose appended YC / YX / YD (7 + 7 + 7 bytes) do not"""
    sc = _scene([sized(em.LONGEST - 8, 100, name=b"push", cigar=((40000, M),))], yx=[70000], yd=[70000])
    return sc + ({"raw_fits": True, "L": em.LONGEST - 4 + 21, "refused": True},)


# ---- copy lanes -----------------------------------------------------------------------------------------------------------------------
ALIGN_LENS = range(33, 163)
_TAG_FORMS = ((1, 0), (300, 0), (70000, 0), (1, 1), (300, 1), (1, 300), (300, 70000), (70000, 300))   # appended bytes 11, 12, 14, 15, 16, 16, 19, 19


def _align_record(raw_len, pos):
    """a record of raw_len bytes: the length comes from the name's length, l_seq (odd and even) and a padding tag"""
    avail = raw_len - 33
    cigar = ((20, M),) if avail >= 12 else ()
    avail -= 4 * len(cigar)
    aux = b"XZZ" + b"p" * ((raw_len // 4) % 9) + b"\0" if avail >= 27 else b""
    avail -= len(aux)
    nm = min(avail, (raw_len * 7) % 6)
    if avail - nm == 1:                                              # (SEQ + QUAL cannot be one byte)
        nm += 1
    return sized(raw_len, pos, name=b"n" * nm, cigar=cigar, aux=aux)


def alignments():
    """130 fresh records of raw lengths 33 .. 162, one each, in an order (and with appended tags of such sizes) that every triple
    (destination mod 4, source mod 4, raw length mod 4) of the 16-lane copy occurs: the order is chosen greedily, a record and a tag form at
    a time, for the triple not seen yet"""
    left = list(ALIGN_LENS)
    src, dst, seen, order = 4, 4, set(), []                         # (where the first record's bytes lie in the blob / the stream)
    while left:
        best = None
        for ln in left:
            for f, (x, d) in enumerate(_TAG_FORMS):
                add = 7 + 3 + em.int_form(x)[1] + (3 + em.int_form(d)[1] if d > 0 else 0)
                nsrc, ndst = (src + 4 + ln) % 4, (dst + 4 + ln + add) % 4
                score = ((dst % 4, src % 4, ln % 4) not in seen) * 100 + sum((ndst, nsrc, r) not in seen for r in range(4))
                if best is None or score > best[0]:
                    best = (score, ln, f, add)
        _, ln, f, add = best
        seen.add((dst % 4, src % 4, ln % 4))
        order.append((ln, f))
        left.remove(ln)
        src, dst = src + 4 + ln, dst + 4 + ln + add
    recs = [_align_record(ln, 100 + 10 * i) for i, (ln, _) in enumerate(order)]
    sc = _scene(recs, yc=[1.5 + i for i in range(len(recs))], yx=[_TAG_FORMS[f][0] for _, f in order], yd=[_TAG_FORMS[f][1] for _, f in order])
    return sc + ({"triples": 64, "raw_lengths": list(ALIGN_LENS), "all_fresh": True},)


def copy_triples(scene):
    """the (destination mod 4, source mod 4, raw length mod 4) of every record's copy: the record's bytes behind its block_size in the
    blob the host hands over (records in order, each behind its length) and in the model's stream"""
    recs = scene[0]
    src = em.offsets([4 + len(r) for r in recs])
    dst = em.offsets(lengths(scene))
    return {((dst[i] + 4) % 4, (src[i] + 4) % 4, len(r) % 4) for i, r in enumerate(recs)}


# ---- tag edits ------------------------------------------------------------------------------------------------------------------------
YX_VALUES = (-2**31 - 1, -2**31, -32769, -32768, -129, -128, -1, 0, 254, 255, 256, 65534, 65535, 65536, 2**32 - 1, 2**32)
YD_VALUES = (-5, 0, 1, 254, 255, 65534, 65535, 2**31 - 1)
FORMS = ("absent", "c", "C", "s", "S", "i", "I", "f", "Z", "A")
_PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f", "d": "<d"}


def field(name, form, val=7):
    if form == "absent":
        return b""
    if form == "Z":
        return name + b"Zab\0"
    if form == "A":
        return name + b"Ax"
    return name + form.encode() + struct.pack(_PACK[form], val)


def _tagged(i, aux, l_seq=4):
    return bamio.encode_record(0, 100 + 10 * i, 0, 60, [30 << 4], b"t", aux=aux, l_seq=l_seq, seq=b"\x12\x48"[:(l_seq + 1) // 2], qual=b"IIII"[:l_seq])[4:]


def int_widths():
    """every YX value at a width or range boundary against every form the record's YX can have, and the same for YD: 16 x 10 + 8 x 10
    records (the tag the record is not about cycles through its own values and forms beside it)"""
    recs, yx, yd = [], [], []
    for vx in YX_VALUES:
        for fx in FORMS:
            k = len(recs)
            recs.append(_tagged(k, b"NHC\x01" + field(b"YX", fx) + field(b"YD", FORMS[k % 10], 9) + b"XSA+"))
            yx.append(vx), yd.append(YD_VALUES[k % 8])
    for vd in YD_VALUES:
        for fd in FORMS:
            k = len(recs)
            recs.append(_tagged(k, field(b"YD", fd) + b"NHC\x01" + field(b"YX", FORMS[(k // 3) % 10], 9)))
            yx.append(YX_VALUES[(k * 5) % 16]), yd.append(vd)
    sc = _scene(recs, yx=yx, yd=yd)
    return sc + ({"appended_letters": "CIScis", "rewritten_letters": "CIScis", "n": 240},)


YC_VALUES = (0.5, 2.0**24 + 1, 1e39, -1e39, 1e-46, 0.0)


def yc_forms():
    """the record's YC absent, `f`, `d`, `i` and `Z` against values a float holds, rounds (2^24 + 1), cannot hold (+-1e39: +-inf) and
    flushes to zero (1e-46).  No NaN: the bits of its payload are not pinned by the reference."""
    recs, yc = [], []
    for v in YC_VALUES:
        for form in ("absent", "f", "d", "i", "Z"):
            recs.append(_tagged(len(recs), b"NHC\x02" + field(b"YC", form, 3) + b"XSA-"))
            yc.append(v)
    sc = _scene(recs, yc=yc)
    return sc + ({"float_words": sorted({0x3F000000, 0x4B800000, 0x7F800000, 0xFF800000, 0}), "n": 30},)


MALFORMED = {"fixed_cut_short": b"XIi\x01\x02\x03", "Z_without_NUL": b"XZZabc", "B_count_past_the_end": b"XBBC" + struct.pack("<I", 1000) + b"\x01\x02",
             "B_unknown_subtype": b"XBBd" + struct.pack("<I", 1) + b"\x01\x02\x03\x04\x05\x06\x07\x08", "unknown_type": b"XXq\x01\x02\x03\x04"}
_BEHIND = b"YDC\x05" + b"YCf\x01\x01\x81\x3f"                       # (no NUL byte: a Z in front of them finds no end)
# a B whose count ends three bytes behind the record: once seven bytes of YC:f are appended it ends behind their "YCf", and a walk of the
# record as it is THEN would take the float's four bytes for the next field.  With this value they read YD:C:5.
MALFORMED["B_count_ends_inside_what_is_appended"] = b"XBBC" + struct.pack("<I", len(_BEHIND) + 3)
YC_READS_AS_YD = struct.unpack("<f", b"YDC\x05")[0]


def after_a_malformed_field():
    """a well-formed YX, a malformed field of each kind, a YD and a YC behind it — twice: with a YX that widens and a positive YD, and
    with a YX that keeps its width and a YD of 0 (nothing to delete: the walk has not seen the YD)"""
    recs, yc, yx, yd = [], [], [], []
    for kind, bad in MALFORMED.items():
        for x, d in ((300, 7), (5, 0)):
            recs.append(_tagged(len(recs), b"NHC\x01" + b"YXC\x04" + bad + _BEHIND))
            yc.append(YC_READS_AS_YD if kind.endswith("appended") else 1.5), yx.append(x), yd.append(d)
    sc = _scene(recs, yc=yc, yx=yx, yd=yd)
    return sc + ({"tail_kept": True, "kinds": len(MALFORMED)},)


def malformed_at(rec):
    """where the malformed bytes of an after_a_malformed_field record begin"""
    return em.aux_start(rec) + len(b"NHC\x01YXC\x04")


def odd_fields():
    """B arrays of every subtype with 0 and 3 elements, H, an empty Z, duplicates of all three tags, an odd l_seq with no aux at all, a
    name of 254 characters"""
    auxes = [b"XB" + b"B" + s.encode() + struct.pack("<I", c) + bytes(range(1, 1 + c * em._BSUB[s])) + tail
             for s in "cCsSiIf" for c in (0, 3) for tail in (b"", b"YXC\x02")]
    auxes += [b"XHH1AE3\0", b"XHH1AE3\0YDS\x00\x01", b"XEZ\0", b"XEZ\0YCf\0\0\x80\x3f",
              b"YXC\x01YXC\x02YDC\x09YDC\x08YCf" + struct.pack("<f", 2.0) + b"YCd" + struct.pack("<d", 9.0),
              b"YDC\x09YDC\x08YXs\x01\x00YXI\x02\0\0\0YCd" + struct.pack("<d", 2.0) + b"YCf" + struct.pack("<f", 9.0)]
    recs = [_tagged(i, a) for i, a in enumerate(auxes)]
    k = len(recs)
    recs.append(_tagged(k, b"", l_seq=3))
    recs.append(bamio.encode_record(0, 100 + 10 * (k + 1), 0, 60, [30 << 4], b"q" * 254, aux=b"", l_seq=0)[4:])
    recs.append(bamio.encode_record(0, 100 + 10 * (k + 2), 0, 60, [30 << 4], b"Q" * 254, aux=b"YXC\x01", l_seq=1, seq=b"\x10", qual=b"I")[4:])
    n = len(recs)
    sc = _scene(recs, yx=[(3, 300, 70000, -2)[i % 4] for i in range(n)], yd=[(0, 4, 300, 0, 70000)[i % 5] for i in range(n)])
    return sc + ({"l_read_name_max": 255, "odd_l_seq_no_aux": True, "n": n},)


# ---- index front end ------------------------------------------------------------------------------------------------------------------
CIGAR_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 100)
_FIRST_OP = (0, 0, 2, 3, 2, 5, 6, 7, 8)   # the code of each CIGAR's first operation: the one M of 1 M, and operation 16 of 17 and 32 of 33 consume the reference


def cigar_lanes():
    """CIGARs of 0 .. 100 operations cycling through all nine codes MIDNSHP=X (the reference length is the sum over exactly M D N = X, summed
    by 16 lanes: operations 16, 17, 32, 33 and on fall to a lane's second and third round), twice: with lengths of tens of bases and with
    lengths that carry the record across 16 kb windows; one record of I and S only (reference length 0: end = pos + 1)"""
    recs, pos = [], 16000
    for scale in (1, 400):
        for k, nc in enumerate(CIGAR_COUNTS):
            cig = [((3 + 7 * j + k) % 60 * scale + 1, (j + _FIRST_OP[k]) % 9) for j in range(nc)]
            recs.append(bamio.encode_record(0, pos, 0, 60, [(l << 4) | o for l, o in cig], b"g%d_%d" % (scale, nc), aux=b"NHC\x01", l_seq=8, seq=b"\x12\x48\x12\x48",
                                            qual=b"IIIIIIII")[4:])
            pos += 37
    recs.append(bamio.encode_record(0, pos, 0, 60, [(5 << 4) | I, (3 << 4) | S] * 9, b"is_only", l_seq=0)[4:])
    sc = _scene(recs, ref_len=[1 << 21])
    return sc + ({"codes": list(range(9)), "counts": list(CIGAR_COUNTS), "cross_window_min": 2, "zero_span_with_cigar": 1, "consuming_past_lane_16": True},)


def parse_cigar(rec):
    l_qname, n_cig = rec[8], struct.unpack_from("<H", rec, 12)[0]
    return [(c >> 4, c & 15) for c in struct.unpack_from("<%dI" % n_cig, rec, 32 + l_qname)]


# ---- the lists the tests go through -----------------------------------------------------------------------------------------------------
SCENES = {
    "on_the_cut": on_the_cut, "on_the_cut/longer": lambda: on_the_cut(1), "on_the_cut/shorter": lambda: on_the_cut(-1),
    "long_between_short/first": lambda: long_between_short("first"), "long_between_short/middle": long_between_short,
    "long_between_short/last": lambda: long_between_short("last"),
    "fullest_member": fullest_member, "one_record/short": one_record, "one_record/long": lambda: one_record(True), "mixed_sizes": mixed_sizes,
    "alignments": alignments, "int_widths": int_widths, "yc_forms": yc_forms, "after_a_malformed_field": after_a_malformed_field,
    "odd_fields": odd_fields, "cigar_lanes": cigar_lanes,
}
REFUSALS = {"one_over": one_over, "tags_push_it_over": tags_push_it_over}
DEVICE_TILE = ("alignments", "mixed_sizes", "long_between_short/first", "long_between_short/middle", "long_between_short/last")
WITH_CSI = ("long_between_short/first", "long_between_short/middle", "long_between_short/last", "cigar_lanes")

_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = (SCENES.get(name) or REFUSALS[name])()
    return _CACHE[name]


def check_claims(name):
    """the claims of a scene that do not hold, as (claim, claimed, found)"""
    sc = get(name)
    recs, yc, yx, yd, ref_len, claims = sc
    ln = lengths(sc)
    off = em.offsets(ln)
    found = {"L": max(ln), "n": len(recs), "refused": em.refused(ln)}
    if not em.refused(ln):
        b, at, sizes = em.cuts(ln)
        empty = em.empty_ranges(ln)
        found.update(B=b, written=len(sizes), empty=empty, payload_at_most=claims.get("payload_at_most") if max(sizes) <= claims.get("payload_at_most", 0) else max(sizes), on_cut=[i for i, o in enumerate(off[:-1]) if o and o % b == 0],
                     empty_min=claims.get("empty_min") if empty >= claims.get("empty_min", 0) else empty,
                     written_min=claims.get("written_min") if len(sizes) >= claims.get("written_min", 0) else len(sizes))
        if "fullest" in claims:
            m = claims["fullest"][0]
            found["fullest"] = (m, sizes[m]) if at[m] == m * b and off[off.index(at[m + 1]) - 1] == (m + 1) * b - 1 and abs(sizes[m] - (b - 1 + max(ln))) <= 4 \
                else ("not the layout", at[m], sizes[m])
    ev = [em.tag_events(r, c, x, d)[1] for r, c, x, d in zip(recs, yc, yx, yd)]
    found["raw_fits"] = all(4 + len(r) <= em.LONGEST for r in recs)
    found["triples"] = len(copy_triples(sc))
    found["raw_lengths"] = sorted(len(r) for r in recs)
    found["all_fresh"] = all(em.is_fresh(r, x) for r, x in zip(recs, yx))
    found["appended_letters"] = "".join(sorted({t for e in ev for nm, what, t in e if what == "append" and nm != "YC"}))
    found["rewritten_letters"] = "".join(sorted({t for e in ev for nm, what, t in e if what == "rewrite" and nm != "YC"}))
    if "float_words" in claims:
        out = em.stream(recs, yc, yx, yd)
        words, o = set(), 0
        for r, c, x, d in zip(recs, yc, yx, yd):
            t = em.tag(r, c, x, d)
            for a, sz in em.walk(t)[0]:
                if t[a:a + 3] == b"YCf":
                    words.add(struct.unpack_from("<I", t, a + 3)[0])
                    break
            o += 4 + len(t)
        assert o == len(out)
        found["float_words"] = sorted(words)
    if "tail_kept" in claims:
        ok = True
        for r, c, x, d, e in zip(recs, yc, yx, yd, ev):
            at_bad = malformed_at(r)
            stop = em.walk(r)[1]
            t = em.tag(r, c, x, d)
            tail = r[stop:]
            grown = 1 if x >= 255 else 0                             # (the YX:C in front widens to S)
            want_app = b"YCf" + em.float_bytes(c) + (b"YDC" + bytes([d]) if d > 0 else b"")
            ok = ok and at_bad <= stop < len(r) and t[stop + grown:stop + grown + len(tail)] == tail and t[stop + grown + len(tail):] == want_app \
                and ("YC", "append", "f") in e and not any(nm == "YD" and what in ("rewrite", "delete") for nm, what, _ in e)
        found["tail_kept"] = ok
        found["kinds"] = len({bytes(r[malformed_at(r):]) for r in recs})
    found["l_read_name_max"] = max(r[8] for r in recs)
    found["odd_l_seq_no_aux"] = any(struct.unpack_from("<I", r, 16)[0] % 2 == 1 and em.aux_start(r) == len(r) for r in recs)
    if "codes" in claims:
        cigs = [parse_cigar(r) for r in recs]
        pos = [struct.unpack_from("<i", r, 4)[0] for r in recs]
        found["codes"] = sorted({o for c in cigs for _, o in c})
        found["counts"] = sorted({len(c) for c in cigs[:-1]})
        cross = sum(1 for p, c in zip(pos, cigs) if p // WINDOW != (p + max(ref_span(c), 1) - 1) // WINDOW)
        found["cross_window_min"] = claims["cross_window_min"] if cross >= claims["cross_window_min"] else cross
        found["zero_span_with_cigar"] = sum(1 for c in cigs if c and ref_span(c) == 0)
        found["consuming_past_lane_16"] = all(any(o in CONSUMES for _, o in c[16:]) for c in cigs[:-1] if len(c) >= 17) and \
            any(o in CONSUMES for c in cigs for _, o in c[32:])
    return [(k, v, found.get(k)) for k, v in claims.items() if found.get(k) != v]
