"""tbk_zlib_deflate (bgzdef.hip: zl_size_k / zl_gather_k behind bgz_deflate_k): every piece of a byte run comes back as one zlib stream
that plain zlib.decompress — which checks the header and the Adler-32 — turns into exactly that piece.  The pieces sit on the edges of
the Adler sums (zlib's own NMAX is 5552; 0xff00 bytes of 0xFF is where a 32-bit weighted sum overflows), of the block types (stored
for random bytes, dynamic Huffman for text and runs) and of the cut table."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAXPAY = 0xff00


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _check(streams, payload, cuts):
    assert len(streams) == len(cuts) - 1
    for k, z in enumerate(streams):
        piece = payload[cuts[k]:cuts[k + 1]]
        assert z[0] & 0x0F == 8 and ((z[0] << 8) | z[1]) % 31 == 0, k            # a valid CMF / FLG pair
        d = zlib.decompressobj()
        got = d.decompress(z) + d.flush()
        assert d.eof and not d.unused_data, k                                    # one finished stream, nothing behind it
        assert got == piece, (k, len(piece))
        assert zlib.decompress(z) == piece
        assert z[-4:] == (zlib.adler32(piece) & 0xFFFFFFFF).to_bytes(4, "big"), k


def _pieces():
    rng = np.random.default_rng(11)
    text = (b"chr12\t98595000\t98595017\t3.250\n" * 4000)[:MAXPAY]
    return {
        "one_byte": b"\xa7",
        "adler_nmax_5552": bytes(rng.integers(0, 256, 5552, dtype=np.uint8)),
        "adler_nmax_5553": bytes(rng.integers(200, 256, 5553, dtype=np.uint8)),
        "full_of_ff": b"\xff" * MAXPAY,
        "full_of_zeros": b"\0" * MAXPAY,
        "random_stored": bytes(rng.integers(0, 256, MAXPAY, dtype=np.uint8)),
        "text": text,
    }


@pytest.mark.parametrize("name", list(_pieces()))
def test_single_piece(ctx, name):
    p = _pieces()[name]
    streams = ctx.zlib_deflate(p, cuts=[0, len(p)])
    _check(streams, p, [0, len(p)])
    if name == "random_stored":
        assert len(streams[0]) == 2 + 5 + len(p) + 4           # a stored block: no Huffman code beats random bytes
    if name in ("full_of_ff", "full_of_zeros", "text"):
        assert len(streams[0]) < len(p) // 20


def test_default_pieces_and_uneven_cuts(ctx):
    ps = _pieces()
    payload = ps["text"] + ps["random_stored"][:1000] + ps["full_of_ff"] + ps["one_byte"] + ps["adler_nmax_5553"]
    n = len(payload)
    # no cut table: pieces of 0xff00 bytes, the last one shorter
    cuts = list(range(0, n, MAXPAY)) + [n]
    _check(ctx.zlib_deflate(payload), payload, cuts)
    # uneven cuts, an empty piece among them (the stream of nothing), a one-byte piece, a full piece
    cuts = [0, 1, 1, 12313, 12313 + 32768, 12313 + 32768 + MAXPAY, n - 5553, n]
    assert all(b - a <= MAXPAY for a, b in zip(cuts, cuts[1:]))
    streams = ctx.zlib_deflate(payload, cuts=cuts)
    _check(streams, payload, cuts)
    assert zlib.decompress(streams[1]) == b""


def test_device_source_equals_host_source(ctx):
    import torch
    ps = _pieces()
    payload = ps["text"][:30001] + ps["adler_nmax_5552"] + ps["full_of_zeros"][:777]
    cuts = [0, 12312, 30001, 30001 + 5552, len(payload)]
    host = ctx.zlib_deflate(payload, cuts=cuts)
    dev = ctx.zlib_deflate(torch.frombuffer(bytearray(payload), dtype=torch.uint8).to("cuda:0"), cuts=cuts)
    _check(dev, payload, cuts)
    assert dev == host


def test_e2big_reports_the_sizes(ctx):
    from tiebrush_amd import _lib
    p = _pieces()["text"]
    cuts = [0, 20000, len(p)]
    want = ctx.zlib_deflate(p, cuts=cuts)
    with pytest.raises(_lib.TbkError) as e:
        ctx.zlib_deflate(p, cuts=cuts, out_cap=16)
    assert e.value.status == -4 and e.value.needed == sum(len(z) for z in want)
    assert list(e.value.sizes) == [len(z) for z in want]
    _check(ctx.zlib_deflate(p, cuts=cuts, out_cap=e.value.needed), p, cuts)     # exactly enough room is enough; the context goes on


def test_bgzf_members_unchanged_beside_zlib(ctx):
    """the BGZF framing of the same pieces carries the same deflate bytes: the zlib pass only reframes the slots"""
    p = _pieces()["text"][:40000] + _pieces()["random_stored"][:3000]
    cuts = [0, 25000, len(p)]
    z = ctx.zlib_deflate(p, cuts=cuts)
    run = ctx.bgzf_deflate(p, cuts=cuts)
    o = 0
    for k in range(2):
        bsize = int.from_bytes(run[o + 16:o + 18], "little") + 1
        assert run[o + 18:o + bsize - 8] == z[k][2:-4], k
        o += bsize
    assert o == len(run)
