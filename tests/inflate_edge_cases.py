"""The hand-built deflate streams for the device inflate's edges (bgz_inflate_wave_k, bamdev.hip), family by family.

Shared by test_deflate_craft_cpu.py, which pins every case against zlib, and test_gpu_inflate_edges.py, which feeds them to the
kernel.  The cases are laid out for the kernel's constants below; the CPU suite reads them from bamdev.hip and fails when they move.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from deflate_craft import (DIST_BASE, DIST_EXTRA, FLUSH, LEN_BASE, LEN_EXTRA, Stream, canonical_codes, complete_lens, expand_header,
                           member, subfield)

# what the cases are laid out for (bamdev.hip: IW_WIN_BYTES, IW_FLUSH, IW_CIN, IW_LBITS, IW_DBITS)
WIN, CIN, LBITS, DBITS = 8192, 2048, 10, 9
assert FLUSH == WIN // 4

Case = namedtuple("Case", "name deflate payload member info")
Bad = namedtuple("Bad", "name deflate member isize")       # isize: the ISIZE written when that is what is wrong, else None


def _case(name, s, info=None, **kw):
    d, p = s.finish()
    return Case(name, d, p, member(d, p, **kw), info or {})


# ---- 1. the near / far threshold -----------------------------------------------------------------------------------------------
# Distances on both sides of IW_WIN - 64 and of IW_WIN itself.  (The ring holds the last IW_WIN bytes and a chunk of 64 is read before
# it is written, so the ring copy is right for every distance up to IW_WIN: moving the threshold anywhere in (IW_WIN - 64, IW_WIN]
# changes no byte.  What the family pins is that both copies give the same bytes where they meet, and the far read beyond IW_WIN.)
THRESH_DISTS = (8064, 8127, 8128, 8129, 8130, 8191, 8192, 8193, 8256)
THRESH_LENS = (3, 63, 64, 65, 128, 129, 257, 258)
POSITIONS = ("early", "wrap", "flush")


def _place(dist, pos):
    """the output offset of the token under test: the earliest place, a copy that wraps the ring, a copy that crosses a flush"""
    if pos == "early":
        return dist + 3
    if pos == "wrap":
        return dist + (WIN - 1 - dist) % WIN              # the first o >= dist with o % IW_WIN == IW_WIN - 1
    return dist + (FLUSH - 1 - dist) % FLUSH              # likewise o % IW_FLUSH == IW_FLUSH - 1 (the prefix is one stored run)


@functools.lru_cache(None)
def threshold():
    rng = np.random.default_rng(101)
    out = []
    for dist in THRESH_DISTS:
        for ln in THRESH_LENS:
            for pos in POSITIONS:
                o = _place(dist, pos)
                s = Stream().stored(rng.bytes(o))
                assert s.o == o >= dist
                assert pos != "wrap" or o % WIN == WIN - 1
                assert pos != "flush" or o - s.flushed == FLUSH - 1
                s.fixed([("match", ln, dist), ("lit", 0x5a), ("lit", 0xa5), ("lit", 0x3c)], final=True)
                out.append(_case("thresh-d%d-l%d-%s" % (dist, ln, pos), s, {"dist": dist, "len": ln, "o": o}))
    for dist in (16384, 32767):
        s = Stream().stored(rng.bytes(dist + 3))
        s.fixed([("match", 258, dist), ("lit", 1)], final=True)
        out.append(_case("thresh-d%d-l258" % dist, s))
    s = Stream().stored(rng.bytes(65536 - 258))                  # the BGZF maximum, the match ends on its last byte
    s.fixed([("match", 258, 32768)], final=True)
    assert s.o == 65536
    out.append(_case("thresh-d32768-l258-isize65536", s))
    return out


# ---- 2. short distances --------------------------------------------------------------------------------------------------------
SHORT_DISTS = tuple(range(1, 67))
# consecutive bytes distinct over any 251: byte j of a match and byte j % dist of its source never agree by accident
PATTERN = bytes((k * 89 + 17) % 251 for k in range(65536 + 4096))
PAD = 80                                                          # bytes of PATTERN in front of every match: more than any distance here


def short_lens(dist):
    return sorted({l for l in (3, dist - 1, dist, dist + 1, 64, 65, 127, 128, 129, 192, 193, 256, 257, 258) if 3 <= l <= 258})


def _pad_to(s, n):
    s.stored(PATTERN[s.o:s.o + n])


@functools.lru_cache(None)
def short():
    out = []
    for dist in SHORT_DISTS:
        lens = short_lens(dist)
        # o small
        s = Stream()
        for ln in lens:
            _pad_to(s, PAD)
            s.fixed([("match", ln, dist)])
        s.fixed([("lit", 7)], final=True)
        out.append(_case("short-d%d-small" % dist, s, {"dist": dist, "lens": lens}))
        # across a flush: o - flushed one short of IW_FLUSH when the match is decoded
        s = Stream()
        for ln in lens:
            n = (FLUSH - 1 - (s.o - s.flushed)) % FLUSH
            _pad_to(s, n if n >= PAD else n + FLUSH)
            assert s.o - s.flushed == FLUSH - 1
            s.fixed([("match", ln, dist)])
        s.fixed([("lit", 7)], final=True)
        out.append(_case("short-d%d-flush" % dist, s, {"dist": dist, "lens": lens}))
        # wrapping the ring: the destination from the ring's last byte on, or the source across the ring's end
        s, part, todo = Stream(), 0, list(enumerate(lens))
        while todo:
            i, ln = todo[0]
            res = WIN - 1 if i % 2 == 0 else dist // 2
            o = s.o + PAD + (res - (s.o + PAD)) % WIN
            if o + ln + 1 > 60000:                              # (stored padding does not shrink: the member must stay under 64 KiB)
                s.fixed([("lit", 7)], final=True)
                out.append(_case("short-d%d-wrap%d" % (dist, part), s, {"dist": dist}))
                s, part = Stream(), part + 1
                continue
            _pad_to(s, o - s.o)
            assert s.o % WIN == res and (res == WIN - 1 or (s.o - dist) // WIN < s.o // WIN or dist == 1)
            s.fixed([("match", ln, dist)])
            todo.pop(0)
        s.fixed([("lit", 7)], final=True)
        out.append(_case("short-d%d-wrap%d" % (dist, part), s, {"dist": dist}))
    return out


# ---- 3. every length and distance code -----------------------------------------------------------------------------------------
def _every_code_tokens():
    toks = []
    for c in range(29):
        for ex in sorted({0, (1 << LEN_EXTRA[c]) - 1}):
            toks += [("match", LEN_BASE[c] + ex, 1000 + 37 * c, c), ("lit", 0x30 + c % 16)]
    for c in range(30):
        for ex in sorted({0, (1 << DIST_EXTRA[c]) - 1}):
            toks += [("match", 5, DIST_BASE[c] + ex), ("lit", 0x30 + c % 16)]
    return toks


@functools.lru_cache(None)
def every_code():
    rng = np.random.default_rng(303)
    pre = rng.bytes(32768)                                        # distance code 29 with all 13 extra bits set reaches all of it
    toks = _every_code_tokens()
    s = Stream().stored(pre).fixed(toks, final=True)
    out = [_case("codes-fixed", s)]
    lit = complete_lens(286, {}, list(range(0x30, 0x40)) + list(range(256, 286)))
    dst = complete_lens(30, {}, list(range(30)))
    s = Stream().stored(pre).dynamic(toks, True, lit, dst)
    assert {y for _, y in s.lit_used} >= set(range(257, 286)) and {y for _, y in s.dist_used} == set(range(30))
    out.append(_case("codes-dynamic", s))
    return out


# ---- 4. code lengths against the table widths ----------------------------------------------------------------------------------
DEEP_LIT = {1: 9, 260: 9, 2: 10, 265: 10, 3: 11, 270: 11, 4: 15, 285: 15}        # first and last code of every depth
DEEP_DIST = {0: 8, 20: 8, 1: 9, 21: 9, 2: 10, 22: 10, 3: 15, 29: 15}


@functools.lru_cache(None)
def table_widths():
    rng = np.random.default_rng(404)
    # the fill symbols lie between the placed ones, so the placed ones stay the first and the last of their depth
    lit = complete_lens(286, DEEP_LIT, list(range(32, 64)) + [256, 257, 258])
    dst = complete_lens(30, DEEP_DIST, list(range(4, 20)))
    lc, dc = canonical_codes(lit), canonical_codes(dst)
    zero_l = next(y for y in range(286) if lit[y] and lc[y] == 0)                # the all-zeros codes: the first of the shortest
    zero_d = next(y for y in range(30) if dst[y] and dc[y] == 0)
    assert lc[285] == (1 << 15) - 1 and dc[29] == (1 << 15) - 1                  # the all-ones codes: the last of the longest
    assert zero_l < 256
    for table, deep in ((lit, DEEP_LIT), (dst, DEEP_DIST)):
        for d in set(deep.values()):
            at = [y for y, l in enumerate(table) if l == d]
            assert table[at[0]] == table[at[-1]] == d and at[0] in deep and at[-1] in deep
    deep_len = {260: 6, 265: 11, 270: 23, 285: 258}
    deep_dst = {y: DIST_BASE[y] + (1 << DIST_EXTRA[y]) - 1 for y in DEEP_DIST}
    shallow_d = DIST_BASE[zero_d]
    toks = []
    for rep in range(3):
        for y in sorted(DEEP_LIT):
            if y < 256:
                toks += [("lit", y), ("lit", zero_l)]
            else:                                                # a deep length symbol with a shallow distance, and the other way
                toks += [("match", deep_len[y], shallow_d + rep), ("lit", zero_l), ("match", 3 + (rep & 1), 700 + y), ("lit", 33)]
        for y in sorted(DEEP_DIST):
            toks += [("match", 4, DIST_BASE[y] + min(rep, (1 << DIST_EXTRA[y]) - 1)), ("lit", zero_l), ("match", deep_len[265] + (rep & 1), deep_dst[y]), ("lit", 34)]
    s = Stream().stored(rng.bytes(32768)).dynamic(toks, True, lit, dst)
    assert {y for _, y in s.lit_used} >= set(DEEP_LIT) | {zero_l} and {y for _, y in s.dist_used} >= set(DEEP_DIST) | {zero_d}
    return [_case("widths", s, {"lit": lit, "dist": dst})]


# ---- 5. header spellings -------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def headers():
    out = []
    text = [("lit", b) for b in b"the quick brown fox"]

    # 16 with counts 3 and 6 (and 5): literals 0..254 at 8 bits, 255 and the end-of-block code at 9; no distance code (ndist 1, 0)
    lit = [8] * 255 + [9, 9]
    hdr = [8] + [(16, 6)] * 41 + [(16, 3), (16, 5), 9, 9, 0]
    s = Stream().dynamic(text + [("lit", 255), ("lit", 0)], True, lit, [0], header=hdr)
    out.append(_case("hdr-16x3-16x6-nodist", s))

    # 16 that carries the end-of-block code's length over the last literal/length length (257) into the four distance lengths
    lit = complete_lens(286, {256: 2, 257: 2}, list(range(97, 123)))
    hdr = lit[:257] + [(16, 5)]
    toks = [("lit", 97), ("lit", 98), ("lit", 99), ("lit", 100), ("match", 3, 1), ("match", 3, 2), ("match", 3, 3), ("match", 3, 4)]
    s = Stream().dynamic(toks, True, lit, [2, 2, 2, 2], header=hdr)
    out.append(_case("hdr-16-crosses-into-dist", s))

    # 17 with counts 3 and 10, 18 with counts 11 and 138; a single distance code of length 1, used, and behind it a run of zeros
    # that ends exactly at nlen + ndist (ndist 30)
    syms = [0, 4, 15, 27, 166, 167, 168, 256]
    hdr = [3, (17, 3), 3, (17, 10), 3, (18, 11), 3, (18, 138), 3, 3, 3, (18, 87), 3, 1, (18, 29)]
    toks = [("lit", y) for y in syms[:-1]] + [("lit", 4), ("lit", 166)]
    s = Stream().dynamic(toks, True, {y: 3 for y in syms}, [1], header=hdr, ndist=30)
    out.append(_case("hdr-17-18-trailing-zeros", s))
    lit3 = {y: 3 for y in [0, 4, 15, 27, 166, 167, 257, 256]}
    hdr = [3, (17, 3), 3, (17, 10), 3, (18, 11), 3, (18, 138), 3, 3, (18, 88), 3, 3, 1]
    toks = [("lit", 0), ("lit", 4), ("lit", 15), ("lit", 27), ("match", 3, 1), ("lit", 166), ("match", 3, 1), ("match", 3, 1)]
    s = Stream().dynamic(toks, True, lit3, [1], header=hdr)
    out.append(_case("hdr-single-dist-code-used", s))

    # nlen 286 and ndist 30, every symbol coded; all 19 code-length code lengths sent
    lit = complete_lens(286, {}, list(range(286)))
    dst = complete_lens(30, {}, list(range(30)))
    toks = text + [("match", 258, 19), ("match", 227, 5, 27), ("lit", 200), ("match", 3, 200)]
    s = Stream().dynamic(toks, True, lit, dst, ncode=19)
    out.append(_case("hdr-nlen286-ndist30-ncode19", s))

    # the fewest code-length code lengths a valid block can send: ncode 5 (16, 17, 18, 0, 8): with ncode 4 no length but 0 has a code
    lit = [8] * 255 + [0, 8]
    hdr = [8] + [(16, 6)] * 42 + [8, 8, 0, 8, 0]
    s = Stream().dynamic(text + [("lit", 254)], True, lit, [0], header=hdr, cl_lens={16: 1, 0: 2, 8: 2})
    assert expand_header(hdr)[:257] == lit and s.blocks[0][0] == "dynamic"
    out.append(_case("hdr-ncode5-literal-only", s))

    # a code-length code with 7-bit codes, used: literal lengths 1 .. 7, 7
    lit = {65: 1, 66: 2, 67: 3, 68: 4, 69: 5, 70: 6, 71: 7, 256: 7}
    hdr = [(18, 65), 1, 2, 3, 4, 5, 6, 7, (18, 138), (18, 46), 7, 0]
    cl = {18: 2, 0: 2, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 7}
    s = Stream().dynamic([("lit", b) for b in b"ABCDEFGGFEDCBA"], True, lit, [0], header=hdr, cl_lens=cl)
    out.append(_case("hdr-7bit-codelength-code", s))

    # an end-of-block-only block (a one-code literal set, no distance code) between two others
    s = Stream().fixed(text)
    s.dynamic([], False, {256: 1}, [0], header=[(18, 138), (18, 118), 1, 0])
    s.fixed([("match", 19, 19), ("lit", 33)], final=True)
    out.append(_case("hdr-eob-only-block", s))
    return out


# ---- 6. block structure --------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def blocks():
    rng = np.random.default_rng(606)
    out = []
    # a stored block whose header ends at each of the 8 bit positions: 8- and 9-bit fixed-code literals in front of it
    for k in range(8):
        s = Stream().fixed([("lit", 200 + j) for j in range(k)] + [("lit", 65)] * (7 - k))
        s.stored(rng.bytes(300), final=True)
        out.append(_case("blocks-stored-align%d" % ((s.blocks[1][1] + 3) % 8), s, {"bit": (s.blocks[1][1] + 3) % 8}))
    # a stored block of length 0: first, in the middle, last
    s = Stream().stored(b"").fixed([("lit", 1), ("lit", 2)]).stored(b"").fixed([("match", 3, 2), ("lit", 3)]).stored(b"", final=True)
    out.append(_case("blocks-stored-len0", s))
    # ISIZE 65536 from the largest stored block a BGZF member has room for, then a fixed block (a 65535-byte stored block does
    # not fit: BSIZE is 16 bits and counts header and trailer)
    s = Stream().stored(rng.bytes(65488)).fixed([("match", 47, 30000), ("lit", 9)], final=True)
    assert s.o == 65536
    out.append(_case("blocks-stored-max-isize65536", s))
    # stored -> fixed -> dynamic -> dynamic with other tables -> stored, every block opening with a match into the one before
    lit_a = complete_lens(286, {}, list(range(64, 96)) + [256, 257, 260, 270, 285])
    lit_b = complete_lens(286, {285: 1}, list(range(100, 110)) + [256, 258])
    dst_a = complete_lens(30, {}, [0, 5, 10, 26])
    dst_b = complete_lens(30, {}, [26, 3, 12])
    s = Stream().stored(rng.bytes(9000))
    s.fixed([("match", 100, 8500), ("lit", 70), ("lit", 71)])                                # far, into the stored block
    s.dynamic([("match", 6, 1), ("lit", 64), ("match", 258, 40), ("lit", 95), ("match", 3, 8200)], False, lit_a, dst_a)
    s.dynamic([("match", 258, 4), ("lit", 100), ("match", 4, 70), ("match", 258, 8193)], False, lit_b, dst_b)
    s.stored(rng.bytes(777), final=True)
    assert [b[0] for b in s.blocks] == ["stored", "fixed", "dynamic", "dynamic", "stored"]
    out.append(_case("blocks-every-type-in-turn", s))
    # 200 tiny blocks
    s = Stream()
    for i in range(200):
        fin = i == 199
        if i % 3 == 0:
            s.stored(bytes([i & 255]), final=fin)
        elif i % 3 == 1:
            s.fixed([("lit", i & 255)] + ([("match", 3, 2)] if i > 3 else []), final=fin)
        else:
            s.dynamic([("lit", 65), ("match", 3, 1)], fin, {65: 1, 257: 2, 256: 2}, [1])
    out.append(_case("blocks-200-tiny", s))
    return out


# ---- 7. staging of the compressed stream ---------------------------------------------------------------------------------------
def _staging_stream(lead, rng_seed=707, tail=0):
    """About 6 KiB of tokens of up to 48 bits (15-bit codes, 5 and 13 extra bits), `lead` one-bit literals in front: every
    variant moves every later token by one bit against the 2 KiB staging chunks and the 32-bit refill."""
    rng = np.random.default_rng(rng_seed)
    lit = complete_lens(286, {0x41: 1, 257: 15, 284: 15}, [y for y in range(256) if y != 0x41] + [256, 285])
    dst = complete_lens(30, {28: 15, 29: 15}, list(range(28)))
    assert lit[0x41] == 1
    toks = [("lit", 0x41)] * lead
    toks += [("lit", int(b)) for b in rng.bytes(293) if b != 0x41]
    per = len(toks) - lead
    toks += [("match", 258, per)] * 101                                       # a period that is no power of two, 26 KB of it
    o = lead + per + 101 * 258
    for i in range(1100):
        far = int(rng.integers(16385, min(o, 32768) + 1))
        toks.append(("match", 3, far) if i % 12 else ("match", 227 + int(rng.integers(0, 31)), far, 27))
        o += toks[-1][1]
        if i % 7 == 0:
            toks.append(("lit", 0x41))
            o += 1
    toks += [("lit", 0x41)] * tail
    return Stream().dynamic(toks, True, lit, dst)


@functools.lru_cache(None)
def staging():
    out = []
    for lead in range(32):
        s = _staging_stream(lead)
        out.append(_case("staging-shift%d" % lead, s, {"nbits": s.w.nbits}))
    for tail in range(8):                                                      # the stream ends on the last bit of its last byte
        s = _staging_stream(0, tail=tail)
        if s.w.nbits % 8 == 0:
            out.append(_case("staging-ends-on-byte", s, {"nbits": s.w.nbits}))
            break
    return out


# ---- 8. framing ----------------------------------------------------------------------------------------------------------------
SUB_A, SUB_B = subfield(ord("X"), ord("Y"), b"abc"), subfield(ord("B"), ord("D"), b"\x01\x02\x03\x04\x05")
EXTRAS = ((SUB_A, b""), (b"", SUB_B), (SUB_A, SUB_B), (subfield(ord("B"), ord("C"), b"\x07"), b""))    # (a BC of another length: not BSIZE)


def payload_member(payload, body, **kw):
    """a member that decodes to a given payload: stored blocks, fixed-code literals, or zlib's own stream re-wrapped"""
    s = Stream()
    if body == "stored":
        cut = list(range(0, len(payload), 21000)) or [0]
        for i, c in enumerate(cut):
            s.stored(payload[c:c + 21000], final=i == len(cut) - 1)
    elif body == "fixed":
        s.fixed([("lit", b) for b in payload], final=True)
    else:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        return member(co.compress(payload) + co.flush(), payload, **kw)
    d, p = s.finish()
    assert p == payload
    return member(d, p, **kw)


@functools.lru_cache(None)
def framing():
    rng = np.random.default_rng(808)
    out = []
    for i, (a, b) in enumerate(EXTRAS):
        s = Stream().fixed([("lit", 70 + i), ("match", 20, 1), ("lit", 3)], final=True)
        out.append(_case("framing-extra%d" % i, s, extra_before=a, extra_after=b))
    # ISIZE 1, 65536, 0, 65535, 7: every later payload starts at an odd offset, the CRC pass's unaligned head with n == 65536
    for n in (1, 65536, 0, 65535, 7):
        s = Stream()
        if n > 100:
            s.stored(rng.bytes(65000)).fixed([("match", 258, 31111), ("match", 258, 20000), ("match", n - 65516, 5)], final=True)
        else:
            s.stored(rng.bytes(n), final=True)
        assert s.o == n
        out.append(_case("framing-isize%d" % n, s))
    return out


def empty_run():
    return [_case("framing-empty%d" % i, Stream().stored(b"", final=True) if i % 2 else Stream().fixed([], final=True),
                  extra_before=EXTRAS[i % 3][0]) for i in range(5)]


FAMILIES = {"threshold": threshold, "short": short, "every_code": every_code, "table_widths": table_widths, "headers": headers,
            "blocks": blocks, "staging": staging, "framing": framing}


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def refusals():
    out = []
    text = [("lit", b) for b in b"refuse me"]

    def bad(name, s, **kw):
        d, p = s.finish()
        assert kw.get("isize", len(p)) > 0                 # (a member of ISIZE 0 is skipped by the host: its stream is never read)
        out.append(Bad(name, d, member(d, p, **kw), kw.get("isize")))

    s = Stream().fixed(text)
    s.w.bits(1, 1)
    s.w.bits(3, 2)
    bad("block-type-3", s)
    bad("stored-len-nlen-mismatch", Stream().stored(b"abcdef", final=True, nlen_field=0xFFF0))
    lit, dst = {97: 1, 256: 2, 257: 2}, [1]
    bad("hlit-nlen-287", Stream().dynamic([("lit", 97)], True, lit, dst, hlit=30))
    bad("hdist-ndist-31", Stream().dynamic([("lit", 97)], True, lit, dst, hdist=30))
    bad("16-first", Stream().fixed(text).dynamic([], True, {256: 1}, [0], header=[(16, 3), (18, 138), (18, 116), 1, 0], eob=False, check=False,
                                     cl_lens={16: 2, 18: 2, 1: 2, 0: 2}))
    bad("repeat-past-the-end", Stream().fixed(text).dynamic([], True, {256: 1}, [0], header=[(18, 138), (18, 118), 1, (17, 3)], check=False))
    bad("no-eob-code", Stream().dynamic([("lit", 0), ("lit", 1)], True, {0: 1, 1: 1}, [0], nlen=257, eob=False))
    # (ncode 4 sends lengths for 16, 17, 18 and 0 alone: every code length is 0, so no block of that kind is valid)
    bad("ncode-4", Stream().fixed(text).dynamic([], True, [0] * 257, [0], header=[(18, 138), (18, 120)], cl_lens={16: 2, 17: 2, 18: 2, 0: 2},
                                    ncode=4, eob=False))
    bad("lit-oversubscribed", Stream().fixed(text).dynamic([], True, {0: 1, 1: 1, 256: 1}, [0], eob=False))
    bad("dist-oversubscribed", Stream().dynamic([("lit", 0)], True, {0: 1, 256: 2, 257: 2}, {0: 1, 1: 1, 2: 1}))
    bad("codelength-code-incomplete", Stream().dynamic([("lit", 0)], True, {0: 1, 256: 2, 257: 2}, [1], cl_lens={0: 2, 1: 2, 2: 2}))
    bad("dist-o-plus-1", Stream().fixed(text + [("rawmatch", 5, len(text) + 1)], final=True), isize=len(text) + 5)
    for y in (286, 287):
        bad("fixed-length-symbol-%d" % y, Stream().fixed(text + [("sym", y), ("dsym", 0)], final=True), isize=len(text) + 3)
    for y in (30, 31):
        bad("fixed-distance-code-%d" % y, Stream().fixed(text + [("sym", 257), ("dsym", y)], final=True), isize=len(text) + 3)
    s = Stream().fixed(text + [("match", 100, 3)], final=True)                # ISIZE one short, the CRC that of the bytes it covers
    bad("decodes-to-isize-plus-1", s, isize=s.o - 1, crc=zlib.crc32(bytes(s.out[:-1])) & 0xFFFFFFFF)
    s = Stream().fixed(text + [("match", 100, 3)], final=True)
    bad("decodes-to-isize-minus-1", s, isize=s.o + 1)
    bad("no-final-block", Stream().fixed(text).stored(b"more").fixed(text, final=False))
    return out
