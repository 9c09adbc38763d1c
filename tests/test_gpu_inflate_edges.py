"""The device inflate (bgz_inflate_wave_k and bgz_crc_k, bamdev.hip) on hand-built deflate streams at every edge the decoder
has: the near / far threshold of the LDS ring, short distances at the ring's wrap and across a flush, every length and
distance code, codes around the table widths, header spellings, block structure, the staging of the compressed stream, and the
framing.  The reference of every valid case is the payload its writer computed (test_deflate_craft_cpu.py shows it equal to
zlib's); the comparison is byte for byte.  Malformed members must be refused."""
import numpy as np
import pytest

import inflate_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _check(ctx, cases):
    """all members in one call, compared member by member: a mismatch names the case and the first differing offset"""
    from tiebrush_amd import api
    try:
        got = ctx.bgzf_inflate(b"".join(c.member for c in cases))
    except api.TbkError:
        refused = []
        for c in cases:                                   # (a refusal is an error code, not a fault: find the member)
            try:
                ctx.bgzf_inflate(c.member)
            except api.TbkError:
                refused.append(c.name)
        pytest.fail("valid members refused: %s" % (refused or "only in the joint call"))
    at, wrong = 0, []
    for c in cases:
        seg = got[at:at + len(c.payload)]
        at += len(c.payload)
        if seg != c.payload:
            a, b = np.frombuffer(seg, np.uint8), np.frombuffer(c.payload, np.uint8)
            n = min(len(a), len(b))
            d = np.flatnonzero(a[:n] != b[:n])
            wrong.append("%s: first difference at %d of %d" % (c.name, int(d[0]) if len(d) else n, len(b)))
    assert not wrong and len(got) == at, "%d of %d cases differ: %s" % (len(wrong), len(cases), "; ".join(wrong[:12]))


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_family(ctx, family):
    _check(ctx, E.FAMILIES[family]())


def test_isize_run_and_empty_run(ctx):
    """ISIZE 1, 65536, 0, 65535, 7 on their own: the payloads behind the first start at odd offsets (the CRC pass's unaligned
    head, with n == 65536); then a run of empty members"""
    run = E.framing()[-5:]
    assert [len(c.payload) for c in run] == [1, 65536, 0, 65535, 7]
    _check(ctx, run)
    assert ctx.bgzf_inflate(b"".join(c.member for c in E.empty_run())) == b""
    _check(ctx, E.empty_run() + run[:1] + E.empty_run())


SOA_FIELDS = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")


def test_bam_decode_on_crafted_framing(ctx):
    """tbk_bam_decode's own member walk: one BAM framed by bamio's writer and once more with hand-built members (odd cuts, empty
    members in the middle, subfields around BC, stored / fixed / zlib bodies) — the same tile and the same records"""
    from tiebrush_amd import bamio
    hdr = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:100000\n"
    body = b"".join(bamio.encode_record(0, 100 + i, 16 * (i & 1), 60, [(20 << 4), (5 << 4) | 3, (30 << 4)], b"read%05d" % i, b"NHC\x01")
                    for i in range(3200))
    raw = bamio.build_bam(hdr, ["c"], [100000], body)
    assert len(raw) > 140_000
    n_other = 77                                        # a second, small file beside it: the per-file base alignment is in play
    p, recs = 0, []
    for _ in range(n_other):
        bs = int.from_bytes(body[p:p + 4], "little")
        recs.append(body[p:p + 4 + bs])
        p += 4 + bs
    other = bamio.bgzf_compress(bamio.build_bam(hdr, ["c"], [100000], b"".join(recs)), 6)
    plain = bamio.bgzf_compress(raw, 6)
    sizes = [1, 65536, 0, 65535, 7, 0, 0, 20001, 9001, 333]
    kinds = ["stored", "zlib", "stored", "zlib", "fixed", "fixed", "zlib", "stored", "fixed", "zlib"]
    parts, at, i = [], 0, 0
    while at < len(raw):
        n, kind = sizes[i % len(sizes)], kinds[i % len(kinds)]
        a, b = E.EXTRAS[i % len(E.EXTRAS)] if i % 2 else (b"", b"")
        parts.append(E.payload_member(raw[at:at + n], kind, extra_before=a, extra_after=b))
        at += n
        i += 1
    crafted = b"".join(parts) + bamio._BGZF_EOF
    assert bamio.bgzf_decompress(crafted) == raw and i > len(sizes)

    def decode(files):
        s, fo = ctx.bam_decode(files)
        got = ctx.soa_to_numpy(s, fields=SOA_FIELDS)
        idx = np.concatenate([np.arange(0, s.n_records, 41, dtype=np.uint32), np.array([3199, 3200, s.n_records - 1], np.uint32)])
        blob, off = ctx.bam_records(idx)
        return fo.copy(), got, bytes(blob), off.copy(), int(s.n_records)

    try:
        fo_p, got_p, blob_p, off_p, n_p = decode([plain, other])
        fo_c, got_c, blob_c, off_c, n_c = decode([crafted, other])
    finally:
        ctx.bam_release()
    assert n_p == n_c == 3200 + n_other and np.array_equal(fo_p, fo_c) and fo_p.tolist() == [0, 3200, 3200 + n_other]
    for name in SOA_FIELDS:
        assert np.array_equal(got_p[name], got_c[name]), name
    assert np.array_equal(got_p["pos"][:3200], 100 + np.arange(3200))
    assert blob_p == blob_c and np.array_equal(off_p, off_c)
    assert blob_p[:int(off_p[1])] == body[:int(off_p[1])]


def test_malformed_members_are_refused(ctx):
    """one call per case, the verdict only; then the same context inflates a good run"""
    from tiebrush_amd import api
    good = E.headers()
    accepted = []
    for b in E.refusals():
        try:
            ctx.bgzf_inflate(b.member)
            accepted.append(b.name)
        except api.TbkError:
            pass
    bad = E.refusals()[0]
    try:
        ctx.bgzf_inflate(good[0].member + bad.member + good[1].member)
        accepted.append("good + %s + good" % bad.name)
    except api.TbkError:
        pass
    assert not accepted, "malformed members accepted: %s" % accepted
    _check(ctx, good)
