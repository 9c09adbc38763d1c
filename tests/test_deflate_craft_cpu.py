"""The hand-built deflate streams of inflate_edge_cases.py (written by deflate_craft.py) against zlib, on the CPU: every valid case
inflates to exactly the payload the writer computed, every malformed one is refused, and the kernel's constants are the ones the
cases are laid out for — so that a failure of test_gpu_inflate_edges.py can only mean the kernel."""
import os
import re
import zlib

import pytest

import deflate_craft as dc
import inflate_edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_canonical_codes_rfc_example():
    # RFC 1951 3.2.2: A..H with lengths (3, 3, 3, 3, 3, 2, 4, 4)
    assert dc.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    assert dc.canonical_codes([0, 1, 0]) == [None, 0, None]


def test_bit_writer_orders():
    w = dc.BitWriter()
    w.bits(0b101, 3)            # a field: least significant bit first
    w.code(0b110, 3)            # a Huffman code: most significant bit first
    w.bits(1, 2)
    assert w.getvalue() == bytes([0b01011101]) and w.nbits == 8
    w.bits(1, 1)
    w.align()
    w.raw(b"\xab")
    assert w.getvalue() == bytes([0b01011101, 1, 0xab])


def test_writer_agrees_with_zlib_on_fixed_and_stored():
    data = b"abcabcabcabc" * 3
    s = dc.Stream().fixed([("lit", b) for b in b"abc"] + [("match", len(data) - 3, 3)]).stored(b"tail", final=True)
    d, p = s.finish()
    assert p == data + b"tail" and zlib.decompress(d, -15) == p


def test_complete_lens_is_complete():
    lens = dc.complete_lens(286, {1: 9, 285: 15}, list(range(40, 60)) + [256])
    assert dc.kraft(lens) == 32768 and lens[1] == 9 and lens[285] == 15 and all(lens[y] for y in range(40, 60))
    with pytest.raises(AssertionError):
        dc.complete_lens(30, {0: 15}, [1, 2])          # 1 - 2^-15 needs 15 terms


@pytest.mark.parametrize("family", sorted(E.FAMILIES))
def test_valid_cases_inflate_with_zlib(family):
    from tiebrush_amd import bamio
    cases = E.FAMILIES[family]()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert zlib.decompress(c.deflate, -15) == c.payload, c.name
        assert len(c.member) <= 65536 and len(c.payload) <= 65536, c.name
    assert bamio.bgzf_decompress(b"".join(c.member for c in cases)) == b"".join(c.payload for c in cases)


def test_empty_run_and_payload_members():
    from tiebrush_amd import bamio
    assert bamio.bgzf_decompress(b"".join(c.member for c in E.empty_run())) == b""
    assert all(zlib.decompress(c.deflate, -15) == b"" for c in E.empty_run())
    p = bytes(range(256)) * 90
    for body in ("stored", "fixed", "zlib"):
        assert bamio.bgzf_decompress(E.payload_member(p, body, extra_before=E.SUB_A)) == p
    assert bamio.bgzf_decompress(E.payload_member(b"", "stored")) == b""


def test_every_listed_value_is_present():
    """the families hold the values they are meant to, not a sample of them"""
    th = [(c.info["dist"], c.info["len"], c.info["o"]) for c in E.threshold() if c.info]      # (at 8064 and 8128 two places coincide)
    for d in (8064, 8127, 8128, 8129, 8130, 8191, 8192, 8193, 8256):
        for ln in (3, 63, 64, 65, 128, 129, 257, 258):
            at = sorted(o for (d_, l_, o) in th if d_ == d and l_ == ln)
            assert len(at) == 3 and d + 3 in at and min(at) >= d and any(o % 8192 == 8191 for o in at) and any(o % 2048 == 2047 for o in at)
    names = {c.name for c in E.threshold()}
    assert {"thresh-d16384-l258", "thresh-d32767-l258", "thresh-d32768-l258-isize65536"} <= names
    sh = E.short()
    for d in range(1, 67):
        want = sorted({l for l in (3, d - 1, d, d + 1, 64, 65, 127, 128, 129, 192, 193, 256, 257, 258) if 3 <= l <= 258})
        for pos in ("small", "flush"):
            c, = [c for c in sh if c.name == "short-d%d-%s" % (d, pos)]
            assert c.info["lens"] == want
        assert any(c.name.startswith("short-d%d-wrap" % d) for c in sh)
    assert sorted(c.info["bit"] for c in E.blocks() if "bit" in c.info) == list(range(8))
    st = E.staging()
    assert sorted(c.info["nbits"] % 32 for c in st[:32]) == list(range(32)) and len(st) == 33 and st[32].info["nbits"] % 8 == 0
    assert all(len(c.deflate) > 6144 + 64 for c in st)          # tokens on both sides of the stream offsets 2048, 4096 and 6144
    assert [len(c.payload) for c in E.framing()[-5:]] == [1, 65536, 0, 65535, 7]


def test_malformed_cases_are_refused_by_zlib():
    bad = E.refusals()
    assert len(bad) == 19
    for b in bad:
        assert int.from_bytes(b.member[-4:], "little") > 0, b.name      # (members of ISIZE 0 never reach the decoder)
        try:
            got = zlib.decompress(b.deflate, -15)
        except zlib.error:
            continue
        assert b.name.startswith("decodes-to-isize") and b.isize is not None and len(got) != b.isize, b.name


def test_cases_are_laid_out_for_the_kernels_constants():
    """If this fails the kernel was retuned: move the edges of inflate_edge_cases.py (WIN, FLUSH, CIN, LBITS, DBITS and the
    values derived from them: the 8128 threshold, the wrap and flush positions, the depths around the table widths) with it —
    the cases would otherwise pass without touching what they are for."""
    src = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "bamdev.hip")).read()
    win = re.search(r"#define\s+IW_WIN_BYTES\s+(\d+)", src)
    decl = re.search(r"constexpr int IW_WIN = IW_WIN_BYTES, IW_FLUSH = ([^,;]+), IW_CIN = (\d+), IW_LBITS = (\d+), IW_DBITS = (\d+);", src)
    assert win and decl, "the IW_* constants moved: update this guard"
    assert int(win.group(1)) == E.WIN == 8192
    assert decl.group(1).strip() == "IW_WIN / 4" and dc.FLUSH == E.WIN // 4
    assert (int(decl.group(2)), int(decl.group(3)), int(decl.group(4))) == (E.CIN, E.LBITS, E.DBITS) == (2048, 10, 9)
    assert "dist > (uint32_t)(IW_WIN - 64)" in src, "the near / far threshold moved: update family 1"
