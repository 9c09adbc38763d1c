"""A plain model of the record layer of the output writer: what one output record looks like once it carries its YC / YX /
YD tags, where the record stream is cut into BGZF members, and the stream itself.  struct and numpy only; nothing here is shared with
the host writer (tagwrite.cpp, bam.cpp), bamio's writer or the kernels (enc_plan_k, enc_emit_k, enc_cuts_k in bgzdef.hip).

The tag rule is flushPData's (the reference's tiebrush.cpp:506-525 through GSam.h:300-305: bam_aux_update_float, bam_aux_update_int,
bam_aux_del, each on the first occurrence of its tag, return values ignored):

  YC  set as a float on the first occurrence when that is `f` or `d` (`d` shrinks to `f`); an occurrence of any other type is left alone;
      absent: appended.
  YX  updated on the first occurrence when that is an integer type: the width never shrinks and the signedness of the type letter follows
      the value; a non-integer occurrence is left alone; absent: appended in the narrowest form.  Nothing at all is edited when the
      value is outside [-2^31, 2^32 - 1].
  YD  the integer rule of YX when the value is positive; otherwise the first occurrence is deleted.

The aux walk stops at the first malformed field: the bytes from there on are copied unchanged, and the tags the walk did not see are
appended behind them.

The cut rule: with L the longest tagged record (its 4-byte block_size included) and B = 0xff00 - L, member m takes the records that
begin in [m B, (m + 1) B); a member nothing begins in is not written.  A stream whose L exceeds 0xff00 - 256 = 65024 is refused."""
import struct

import numpy as np

MAXPAY = 0xFF00                    # payload bytes of a member at most
MARGIN = 256                       # the smallest B the encoder accepts
LONGEST = MAXPAY - MARGIN          # 65024: the longest tagged record (block_size included) it accepts
EUNSUPPORTED = -5

_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
_BSUB = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_INTW = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4}


def aux_start(rec: bytes) -> int:
    """offset of the aux region of a raw record (no block_size in front)"""
    l_qname = rec[8]
    n_cig = struct.unpack_from("<H", rec, 12)[0]
    l_seq = struct.unpack_from("<I", rec, 16)[0]
    return 32 + l_qname + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def field_size(rec: bytes, a: int) -> int:
    """bytes of the aux field that begins at a, 0 when it is malformed (does not end inside the record, unknown type or subtype)"""
    end = len(rec)
    if a + 3 > end:
        return 0
    t = chr(rec[a + 2])
    if t in _FIXED:
        return 3 + _FIXED[t] if a + 3 + _FIXED[t] <= end else 0
    if t in "ZH":
        z = rec.find(b"\0", a + 3)
        return z + 1 - a if z >= 0 else 0
    if t == "B":
        if a + 8 > end:
            return 0
        es = _BSUB.get(chr(rec[a + 3]))
        if es is None:
            return 0
        tot = 8 + es * struct.unpack_from("<I", rec, a + 4)[0]
        return tot if a + tot <= end else 0
    return 0


def walk(rec: bytes):
    """([(offset, size) of every well-formed field in order], the offset the walk stops at: the record's end or the first malformed field)"""
    a, out = aux_start(rec), []
    while a + 3 <= len(rec):
        sz = field_size(rec, a)
        if not sz:
            break
        out.append((a, sz))
        a += sz
    return out, a


def int_form(val: int):
    """(type letter, width) of a new integer tag"""
    if val < -32768:
        return "i", 4
    if val < -128:
        return "s", 2
    if val < 0:
        return "c", 1
    if val < 255:
        return "C", 1
    if val < 65535:
        return "S", 2
    return "I", 4


def _int_bytes(name: bytes, letter: str, width: int, val: int) -> bytes:
    return name + letter.encode() + (val & 0xFFFFFFFF).to_bytes(4, "little")[:width]


def float_bytes(yc) -> bytes:
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(np.float64(yc)).tobytes()


def tag_events(rec: bytes, yc, yx: int, yd: int):
    """(the tagged record, [(tag, what, type letter)]) with what in "append", "rewrite", "delete", "left" (an occurrence of a type the rule does
    not touch) and "none" (a value the rule does not write)"""
    rec = bytes(rec)
    fields, stop = walk(rec)
    yx, yd = int(yx), int(yd)
    x_ok = -(1 << 31) <= yx <= (1 << 32) - 1
    out, seen, events = [rec[:aux_start(rec)]], set(), []

    def int_edit(name, a, val):
        old = _INTW.get(chr(rec[a + 2]))
        if old is None:
            events.append((name, "left", chr(rec[a + 2])))
            return None
        letter, w = int_form(val)
        if old >= w:                                   # the width never shrinks; the sign class follows the value
            w = old
            letter = {1: "cC", 2: "sS", 4: "iI"}[old][0 if val < 0 else 1]
        events.append((name, "rewrite", letter))
        return _int_bytes(name.encode(), letter, w, val)

    for a, sz in fields:
        name = rec[a:a + 2].decode("latin-1")
        new = None
        if name in ("YC", "YX", "YD") and name not in seen:
            seen.add(name)
            t = chr(rec[a + 2])
            if name == "YC":
                if t in "fd":
                    new = b"YCf" + float_bytes(yc)
                    events.append(("YC", "rewrite", "f"))
                else:
                    events.append(("YC", "left", t))
            elif name == "YX":
                if x_ok:
                    new = int_edit("YX", a, yx)
                else:
                    events.append(("YX", "none", t))
            elif yd > 0:
                new = int_edit("YD", a, yd)
            else:
                new = b""
                events.append(("YD", "delete", t))
        out.append(rec[a:a + sz] if new is None else new)
    out.append(rec[stop:])                             # from the first malformed field on: as it is
    if "YC" not in seen:
        out.append(b"YCf" + float_bytes(yc))
        events.append(("YC", "append", "f"))
    if "YX" not in seen:
        if x_ok:
            letter, w = int_form(yx)
            out.append(_int_bytes(b"YX", letter, w, yx))
            events.append(("YX", "append", letter))
        else:
            events.append(("YX", "none", ""))
    if "YD" not in seen and yd > 0:
        letter, w = int_form(yd)
        out.append(_int_bytes(b"YD", letter, w, yd))
        events.append(("YD", "append", letter))
    return b"".join(out), events


def tag(rec: bytes, yc, yx: int, yd: int) -> bytes:
    return tag_events(rec, yc, yx, yd)[0]


def is_fresh(rec: bytes, yx: int) -> bool:
    """the record takes the encoder's 16-lane copy: none of the three tags among the fields the walk sees, and a YX value that is written"""
    fields, _ = walk(rec)
    return -(1 << 31) <= int(yx) <= (1 << 32) - 1 and not any(rec[a:a + 2] in (b"YC", b"YX", b"YD") for a, _ in fields)


def tagged_lengths(records, yc, yx, yd):
    """bytes of every tagged record in the stream, block_size included"""
    return [4 + len(tag(r, c, x, d)) for r, c, x, d in zip(records, yc, yx, yd)]


def offsets(lengths):
    o = [0]
    for ln in lengths:
        o.append(o[-1] + ln)
    return o


def cuts(lengths):
    """(B, [offset of every written member's first byte, then the stream's length], [payload bytes of every written member])"""
    big = max(lengths)
    b = MAXPAY - big
    assert b >= MARGIN, "a stream the encoder refuses"
    off = offsets(lengths)
    at, last = [], -1
    for o in off[:-1]:
        if o // b != last:
            last = o // b
            at.append(o)
    at.append(off[-1])
    return b, at, [q - p for p, q in zip(at, at[1:])]


def empty_ranges(lengths):
    """how many ranges [m B, (m + 1) B) below the stream's end no record begins in"""
    b, at, _ = cuts(lengths)
    return -(-offsets(lengths)[-1] // b) - (len(at) - 1)


def refused(lengths) -> bool:
    return max(lengths) > LONGEST


def stream(records, yc, yx, yd) -> bytes:
    out = []
    for r, c, x, d in zip(records, yc, yx, yd):
        t = tag(r, c, x, d)
        out.append(struct.pack("<I", len(t)) + t)
    return b"".join(out)
