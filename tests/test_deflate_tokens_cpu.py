"""tests/deflate_tokens.py, the RFC 1951 reader that reports tokens and headers, against zlib's own streams (levels 0, 1, 6, 9: stored,
fixed and dynamic blocks) and against streams deflate_craft writes to order: every decode gives exactly the payload, the tokens
re-expanded by the plain LZ77 copy give it too, and what zlib rejects is rejected."""
import functools
import zlib

import numpy as np
import pytest

import deflate_craft as dc
import deflate_tokens as dt


@functools.lru_cache(maxsize=None)
def _payloads():
    rng = np.random.default_rng(23)
    return {
        "empty": b"",
        "one": b"x",
        "short_text": b"hello, hello, hello world",                                   # small enough for a fixed block
        "text": b"".join(b"chr%d\t%d\tACGTTGCA\n" % (i % 5, 100 * i) for i in range(400)),
        "random": rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(),             # stored blocks at every level, several of them
        "zeros": bytes(5_000),
        "mixed": rng.integers(0, 256, 3_000, dtype=np.uint8).tobytes() + b"ab" * 1_000 + rng.integers(0, 4, 4_000, dtype=np.uint8).tobytes(),
    }


def lz77(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _decoded(name, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return dt.decode(c.compress(_payloads()[name]) + c.flush())


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("name", sorted(_payloads()))
def test_zlib_streams_decode_to_their_payload(name, level):
    payload = _payloads()[name]
    d = _decoded(name, level)
    assert d.payload == payload
    assert lz77([t for b in d.blocks for t in b.tokens]) == payload
    assert d.blocks[-1].final and not any(b.final for b in d.blocks[:-1])
    spans = [sum(1 if isinstance(t, int) else t[0] for t in b.tokens) for b in d.blocks]
    assert [b.start for b in d.blocks] == [sum(spans[:i]) for i in range(len(spans))]
    for b in d.blocks:
        if b.btype == 2:
            assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and 4 <= b.hclen <= 19 and len(b.cl_lens) == 19


def test_block_types_are_seen():
    types = set()
    for name in _payloads():
        for level in (0, 1, 6, 9):
            types |= {b.btype for b in _decoded(name, level).blocks}
    assert types == {0, 1, 2}


def _craft_products():
    lit = dc.complete_lens(288, {}, [65, 66, 256, 257 + 28, 257 + 2])
    dist = dc.complete_lens(32, {}, [0, 1, 3, 29])
    yield "dynamic", dc.Stream().dynamic([("lit", 65), ("lit", 66), ("match", 258, 1), ("match", 5, 2), ("match", 5, 4)] + [("match", 258, 1)] * 96 +
                                         [("match", 5, 24577)], True, lit, dist)
    yield "fixed", dc.Stream().fixed([("lit", 1), ("lit", 2), ("match", 3, 2), ("match", 258, 1, 28), ("match", 10, 7)], final=True)
    yield "stored_then_fixed", dc.Stream().stored(b"abcdef").stored(b"").fixed([("match", 6, 6), ("lit", 0)], final=True)
    yield "one_distance_code", dc.Stream().dynamic([("lit", 7), ("match", 4, 1)], True, {7: 1, 256: 2, 258: 2}, {0: 1})
    yield "zero_runs_in_the_header", dc.Stream().dynamic([("lit", 7), ("match", 4, 1)], True, {7: 1, 256: 2, 258: 2}, {0: 1},
                                                          header=[(17, 7), 1, (18, 138), (18, 110), 2, 0, 2, 1])
    yield "copied_lengths_in_the_header", dc.Stream().dynamic([("lit", 3), ("lit", 0)], True, {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 3, 256: 3}, {0: 1},
                                                               header=[3, (16, 6), (18, 138), (18, 111), 3, 1])


@pytest.mark.parametrize("name", [n for n, _ in _craft_products()])
def test_crafted_streams_decode_to_their_payload(name):
    z, payload = dict(_craft_products())[name].finish()
    d = zlib.decompressobj(-15)
    assert d.decompress(z) + d.flush() == payload and d.eof                     # (the stream is what it was meant to be)
    got = dt.decode(z)
    assert got.payload == payload
    assert lz77([t for b in got.blocks for t in b.tokens]) == payload


def test_what_zlib_rejects_is_rejected():
    lit = dc.complete_lens(288, {}, [65, 256, 258])
    bad = {
        "distance before the start": dc.Stream().fixed([("lit", 1), ("rawmatch", 3, 2)], final=True),
        "over-subscribed": dc.Stream().dynamic([("lit", 65)], True, {65: 1, 256: 1, 258: 1}, {0: 1}, check=False),
        "incomplete": dc.Stream().dynamic([("lit", 65)], True, {65: 2, 256: 2, 258: 2}, {0: 1}),
        "incomplete distances": dc.Stream().dynamic([("lit", 65)], True, lit, {0: 2, 1: 2}),
        "symbol 286": dc.Stream().fixed([("sym", 286)], final=True),
        "distance symbol 30": dc.Stream().fixed([("lit", 1), ("sym", 257), ("dsym", 30)], final=True),
        "no end": dc.Stream().fixed([("lit", 1)], final=True, eob=False),
        "LEN / NLEN": dc.Stream().stored(b"abc", final=True, nlen_field=0x1234),
    }
    for what, s in bad.items():
        z, _ = s.finish()
        with pytest.raises(zlib.error):
            d = zlib.decompressobj(-15)
            d.decompress(z)
            if not d.eof:
                raise zlib.error("incomplete")
        with pytest.raises(dt.DeflateError):
            dt.decode(z)
    good, _ = dc.Stream().fixed([("lit", 1)], final=True).finish()
    dt.decode(good)
    with pytest.raises(dt.DeflateError):
        dt.decode(good + b"\0")                                                  # a byte behind the final block
    with pytest.raises(dt.DeflateError):
        dt.decode(good[:-1] + bytes([good[-1] | 0x80]))                          # a bit behind it that is no padding
    with pytest.raises(dt.DeflateError):
        dt.decode(good[:1])                                                      # cut short
