"""A plain RFC 1951 reader that keeps what a decoder throws away (test infrastructure; standard library only, no GPU).

zlib says whether a stream is valid and what it decodes to.  It does not say which tokens the encoder chose, which code lengths it
sent or how it spelled the header: what the device encoder's parse (bgz_deflate_k, bgzdef.hip) is judged by.  decode() returns, per
block, BTYPE, the counts HLIT / HDIST / HCLEN (the numbers of lengths sent: 257 + the 5-bit field, 1 + the 5-bit field, 4 + the 4-bit
field), the three code-length tables and the token list — a literal is an int, a match the pair (length, distance) —, and the payload.
It raises DeflateError on what zlib rejects: an over-subscribed or incomplete code (the one exception zlib makes: a literal/length or distance
code of a single symbol of length 1, or a distance code of none), a missing end-of-block code, a repeat without a previous length or past the end of the
lengths, a symbol without a meaning (286, 287, distance 30, 31), a distance before the start, a stream that ends early, anything but
padding behind the final block.  tests/test_deflate_tokens_cpu.py holds it against zlib's own streams and deflate_craft's."""
from collections import namedtuple

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

Block = namedtuple("Block", "btype final hlit hdist hclen lit_lens dist_lens cl_lens tokens start")
Decoded = namedtuple("Decoded", "blocks payload nbits")


class DeflateError(ValueError):
    pass


class _Bits:
    def __init__(self, data):
        self.d = data
        self.pos = 0                      # in bits

    def take(self, n):
        if self.pos + n > 8 * len(self.d):
            raise DeflateError("the stream ends inside a field")
        byte = self.pos >> 3                                              # (n <= 16: three bytes hold any field)
        v = (int.from_bytes(self.d[byte:byte + 3], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return v


def _table(lens, what, may_be_incomplete=False):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2); Kraft sum checked the way zlib's inflate_table does"""
    used = [l for l in lens if l]
    left = 1 << 15
    for l in used:
        left -= 1 << (15 - l)
    if left < 0:
        raise DeflateError("over-subscribed %s code" % what)
    if left > 0 and not (may_be_incomplete and (not used or used == [1])):
        raise DeflateError("incomplete %s code" % what)
    maxl = max(used, default=0)
    count = [0] * (maxl + 2)
    for l in used:
        count[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, l in enumerate(lens):
        if l:
            tab[(l, nxt[l])] = s
            nxt[l] += 1
    return tab


def _symbol(bits, tab, what):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)            # Huffman codes arrive most significant bit first
        s = tab.get((l, code))
        if s is not None:
            return s
    raise DeflateError("a bit string that is no %s code" % what)


def expand(tokens, out=None):
    """the plain LZ77 copy: tokens -> bytes (appended to out, whose tail is the window)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            if not 1 <= dist <= len(out):
                raise DeflateError("distance %d at output offset %d" % (dist, len(out)))
            for _ in range(length):
                out.append(out[-dist])
    return out


def positions(tokens, start=0):
    """[(payload offset of the token, token)]"""
    out, p = [], start
    for t in tokens:
        out.append((p, t))
        p += 1 if isinstance(t, int) else t[0]
    return out


def decode(data):
    """the deflate bytes of one member -> Decoded(blocks, payload, bits used)"""
    bits = _Bits(bytes(data))
    out = bytearray()
    blocks = []
    while True:
        final, btype = bits.take(1), bits.take(2)
        start = len(out)
        hlit = hdist = hclen = None
        lit_lens = dist_lens = cl_lens = None
        if btype == 3:
            raise DeflateError("block type 3")
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            ln, nln = bits.take(16), bits.take(16)
            if ln ^ nln != 0xFFFF:
                raise DeflateError("LEN and NLEN of a stored block disagree")
            at = bits.pos >> 3
            if at + ln > len(bits.d):
                raise DeflateError("the stream ends inside a stored block")
            tokens = list(bits.d[at:at + ln])
            bits.pos += 8 * ln
            out += bits.d[at:at + ln]
        else:
            if btype == 1:
                lit_lens, dist_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
                ltab, dtab = _table(lit_lens, "literal/length"), _table(dist_lens, "distance")
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise DeflateError("too many length or distance symbols")
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = bits.take(3)
                ctab = _table(cl_lens, "code-length")
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, ctab, "code-length")
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise DeflateError("a repeat with no length before it")
                        rep, v = 3 + bits.take(2), lens[-1]
                    elif s == 17:
                        rep, v = 3 + bits.take(3), 0
                    else:
                        rep, v = 11 + bits.take(7), 0
                    if len(lens) + rep > hlit + hdist:
                        raise DeflateError("a repeat runs past the last length")
                    lens += [v] * rep
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
                if lit_lens[256] == 0:
                    raise DeflateError("no end-of-block code")
                ltab = _table(lit_lens, "literal/length", may_be_incomplete=True)
                dtab = _table(dist_lens, "distance", may_be_incomplete=True)
            tokens = []
            while True:
                s = _symbol(bits, ltab, "literal/length")
                if s < 256:
                    tokens.append(s)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError("literal/length symbol %d" % s)
                length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                d = _symbol(bits, dtab, "distance")
                if d > 29:
                    raise DeflateError("distance symbol %d" % d)
                dist = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                tokens.append((length, dist))
                expand([(length, dist)], out)
        blocks.append(Block(btype, final, hlit, hdist, hclen, lit_lens, dist_lens, cl_lens, tokens, start))
        if final:
            break
    used = bits.pos
    end = (used + 7) >> 3
    if end != len(bits.d):
        raise DeflateError("%d bytes behind the final block" % (len(bits.d) - end))
    if used & 7 and bits.d[-1] >> (used & 7):
        raise DeflateError("bits behind the final block that are no padding")
    return Decoded(blocks, bytes(out), used)
