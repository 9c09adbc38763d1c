"""A deflate (RFC 1951) and BGZF writer that does what it is told (test infrastructure; standard library only).

zlib emits what its matcher and its tree builder choose.  The device decoder (bgz_inflate_wave_k, bamdev.hip) has edges zlib
rarely or never reaches: a given distance at a given output offset, a code of a given length, a header spelled a given way.
Here the caller gives the token list, the code lengths of both alphabets and the spelling of the header; the decoded payload is
computed alongside by the plain byte-by-byte definition.  test_deflate_craft_cpu.py pins every stream written here against zlib.
"""
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8      # 288 symbols: 286 and 287 have codes and no meaning
FIXED_DIST_LENS = [5] * 32                                        # likewise 30 and 31

# The decoder under test moves its output from an LDS ring to memory whenever this many bytes have gathered (IW_FLUSH).  The
# writer tracks where that happens so that a case can put a token right before a flush; the CPU suite checks the constant.
FLUSH = 2048


class BitWriter:
    """fields LSB first, Huffman codes MSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.done = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def nbits(self):
        return 8 * len(self.done) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n), (value, n)
        self.acc |= value << self.n
        self.n += n
        if self.n >= 8:
            k = self.n >> 3
            self.done += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, length):
        assert code is not None and 0 <= code < (1 << length), (code, length)
        self.bits(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.done += data

    def getvalue(self):
        return bytes(self.done) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lens):
    """RFC 1951 3.2.2: the code of every symbol from the code lengths (None for length 0)"""
    maxl = max(lens, default=0)
    count = [0] * (maxl + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt = [0] * (maxl + 2)
    code = 0
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """sum of 2^-l over the coded symbols, in units of 2^-15 (a complete code: 32768)"""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lens(n, placed, fill):
    """Code lengths of an n-symbol alphabet with the symbols of `placed` ({symbol: depth}) at their depths and the symbols of
    `fill` (in that order, the first the shortest) at whatever depths make the code complete: Kraft sum exactly 1."""
    lens = [0] * n
    for s, d in placed.items():
        assert 1 <= d <= 15 and s not in fill
        lens[s] = d
    rest = 32768 - kraft(lens)
    assert rest > 0 and fill
    terms = [1 << b for b in range(15, -1, -1) if rest >> b & 1]        # descending powers of two (units of 2^-15)
    assert len(terms) <= len(fill), "too few fill symbols"
    while len(terms) < len(fill):                                       # split the largest: codes stay as short as they can
        assert terms[0] > 1, "too many fill symbols"
        h = terms.pop(0) >> 1
        terms += [h, h]
        terms.sort(reverse=True)
    for s, t in zip(fill, terms):
        lens[s] = 15 - (t.bit_length() - 1)
        assert lens[s] >= 1
    assert kraft(lens) == 32768
    return lens


def length_symbol(length, code=None):
    """(symbol - 257, extra value, extra bits) of a match length; `code` forces a symbol that can spell it (284 + 31 is 258 too)"""
    if code is None:
        code = 28 if length == 258 else max(c for c in range(28) if LEN_BASE[c] <= length)
    ex = length - LEN_BASE[code]
    assert 0 <= ex < (1 << LEN_EXTRA[code]), (length, code)
    return code, ex, LEN_EXTRA[code]


def dist_symbol(dist):
    code = max(c for c in range(30) if DIST_BASE[c] <= dist)
    ex = dist - DIST_BASE[code]
    assert 0 <= ex < (1 << DIST_EXTRA[code]), dist
    return code, ex, DIST_EXTRA[code]


def expand_header(header):
    """the code lengths a header spelling stands for: ints are plain lengths, (16 | 17 | 18, count) the repeat codes"""
    out = []
    for h in header:
        if isinstance(h, int):
            out.append(h)
        elif h[0] == 16:
            out += [out[-1]] * h[1]
        else:
            out += [0] * h[1]
    return out


def _as_list(lens, n):
    if isinstance(lens, dict):
        out = [0] * n
        for s, l in lens.items():
            out[s] = l
        return out
    return list(lens) + [0] * (n - len(lens))


class Stream:
    """One raw deflate stream and, alongside, the payload it decodes to.

    Tokens: ("lit", byte); ("match", length, distance[, length code 0..28]); and for malformed streams, which leave the payload
    alone: ("rawmatch", length, distance), ("sym", literal/length symbol), ("dsym", distance symbol)."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.flushed = 0          # where the decoder under test last flushed (see FLUSH)
        self.blocks = []          # (type, bit offset of the block header) of every block written
        self.lit_used = set()     # (block index, symbol) of every literal/length and distance symbol written
        self.dist_used = set()

    @property
    def o(self):
        return len(self.out)

    def _token_done(self):
        if self.o - self.flushed >= FLUSH:
            self.flushed = self.o

    def stored(self, data, final=False, len_field=None, nlen_field=None):
        data = bytes(data)
        assert len(data) <= 0xFFFF
        self.blocks.append(("stored", self.w.nbits))
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        ln = len(data) if len_field is None else len_field
        self.w.bits(ln, 16)
        self.w.bits(ln ^ 0xFFFF if nlen_field is None else nlen_field, 16)
        self.w.raw(data)
        self.out += data
        self.flushed += (self.o - self.flushed) // FLUSH * FLUSH          # (a flush check per stored byte)
        return self

    def _tokens(self, tokens, lcodes, llens, dcodes, dlens):
        w, b = self.w, len(self.blocks) - 1

        def lsym(s):
            assert llens[s], "literal/length symbol %d has no code" % s
            w.code(lcodes[s], llens[s])
            self.lit_used.add((b, s))

        def dsym(s):
            assert dlens[s], "distance symbol %d has no code" % s
            w.code(dcodes[s], dlens[s])
            self.dist_used.add((b, s))

        for t in tokens:
            if t[0] == "lit":
                lsym(t[1])
                self.out.append(t[1])
            elif t[0] in ("match", "rawmatch"):
                length, dist = t[1], t[2]
                lc, lx, lxn = length_symbol(length, t[3] if len(t) > 3 else None)
                lsym(257 + lc)
                if lxn:
                    w.bits(lx, lxn)
                dc, dx, dxn = dist_symbol(dist)
                dsym(dc)
                if dxn:
                    w.bits(dx, dxn)
                if t[0] == "match":
                    assert 1 <= dist <= self.o, (dist, self.o)
                    for _ in range(length):
                        self.out.append(self.out[-dist])
            elif t[0] == "sym":
                lsym(t[1])
            elif t[0] == "dsym":
                dsym(t[1])
            else:
                raise ValueError(t)
            self._token_done()

    def fixed(self, tokens, final=False, eob=True):
        self.blocks.append(("fixed", self.w.nbits))
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        lc, dc = canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS)
        self._tokens(tokens, lc, FIXED_LIT_LENS, dc, FIXED_DIST_LENS)
        if eob:
            self.w.code(lc[256], FIXED_LIT_LENS[256])
        return self

    def dynamic(self, tokens, final, lit_lens, dist_lens, header=None, cl_lens=None, ncode=None, nlen=None, ndist=None,
                hlit=None, hdist=None, eob=True, check=True):
        """lit_lens / dist_lens: code lengths (list, or {symbol: length}).  header: how they are spelled (expand_header), default
        plain lengths.  cl_lens: the code-length code's own lengths ({symbol: length}), default a complete code over the symbols
        the header uses.  nlen / ndist / ncode: the counts, default the smallest that hold every coded symbol.  hlit / hdist: the
        raw 5-bit fields (malformed headers).  check=False lets a header through that does not spell the lengths."""
        lit_lens, dist_lens = _as_list(lit_lens, 288), _as_list(dist_lens, 32)
        if nlen is None:
            nlen = max([257] + [s + 1 for s, l in enumerate(lit_lens) if l])
        if ndist is None:
            ndist = max([1] + [s + 1 for s, l in enumerate(dist_lens) if l])
        want = lit_lens[:nlen] + dist_lens[:ndist]
        if header is None:
            header = list(want)
        if check:
            assert nlen <= 286 and ndist <= 30
            assert expand_header(header) == want, "the header does not spell the code lengths"
        used = sorted({h if isinstance(h, int) else h[0] for h in header})
        if cl_lens is None:
            if len(used) == 1:                                            # (a one-symbol code is incomplete: give it a partner)
                used.append(1 if used[0] != 1 else 2)
            cl = complete_lens(19, {}, used)
        else:
            cl = _as_list(cl_lens, 19)
        if ncode is None:
            ncode = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
        assert all(cl[s] == 0 for s in CL_ORDER[ncode:]) and max(cl) <= 7
        w = self.w
        self.blocks.append(("dynamic", w.nbits))
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(nlen - 257 if hlit is None else hlit, 5)
        w.bits(ndist - 1 if hdist is None else hdist, 5)
        w.bits(ncode - 4, 4)
        for s in CL_ORDER[:ncode]:
            w.bits(cl[s], 3)
        cc = canonical_codes(cl)
        self.cl_lens = cl
        for h in header:
            s = h if isinstance(h, int) else h[0]
            assert cl[s], "code-length symbol %d has no code" % s
            w.code(cc[s], cl[s])
            if s == 16:
                w.bits(h[1] - 3, 2)
            elif s == 17:
                w.bits(h[1] - 3, 3)
            elif s == 18:
                w.bits(h[1] - 11, 7)
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        self._tokens(tokens, lc, lit_lens, dc, dist_lens)
        if eob:
            w.code(lc[256], lit_lens[256])
        return self

    def finish(self):
        return self.w.getvalue(), bytes(self.out)


def subfield(si1, si2, data):
    """a well-formed gzip extra subfield (RFC 1952 2.3.1.1)"""
    return bytes([si1, si2]) + len(data).to_bytes(2, "little") + bytes(data)


def member(deflate_bytes, payload, extra_before=b"", extra_after=b"", isize=None, crc=None):
    """One BGZF member: the gzip header with the BC subfield (and whatever subfields the caller puts around it), the stream, CRC32
    and ISIZE of `payload` — or the ISIZE / CRC32 given (malformed members)."""
    xlen = len(extra_before) + 6 + len(extra_after)
    bsize = 12 + xlen + len(deflate_bytes) + 8 - 1
    assert bsize <= 0xFFFF, "a BGZF member holds 64 KiB at the most, header and trailer included"
    extra = extra_before + b"BC\x02\x00" + bsize.to_bytes(2, "little") + extra_after
    head = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + xlen.to_bytes(2, "little") + extra
    crc = zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc
    isize = len(payload) if isize is None else isize
    return head + bytes(deflate_bytes) + crc.to_bytes(4, "little") + isize.to_bytes(4, "little")
