"""The encoder scenes (enc_scenes.py) before a GPU is asked: every scene is what its claims say, and the model (enc_model.py) writes the
record stream the host writer writes (tbh_tag_deflate_part: tagwrite.cpp, the code the command line's host writer tags with, pinned to
the reference's bytes by the golden end-to-end tests)."""
import struct

import pytest

import enc_model as em
import enc_scenes as es
from helpers import host_tagged_stream


@pytest.mark.parametrize("name", list(es.SCENES) + list(es.REFUSALS))
def test_claims_hold(name):
    assert es.check_claims(name) == []
    recs, yc, yx, yd, ref_len, claims = es.get(name)
    assert len(recs) == len(yc) == len(yx) == len(yd) <= 300 and sum(4 + len(r) for r in recs) < 210_000
    pos = [struct.unpack_from("<ii", r, 0) for r in recs]
    assert pos == sorted(pos) and all(t == 0 for t, _ in pos)          # coordinate order on reference 0: every scene can be indexed
    assert (name in es.REFUSALS) == em.refused(es.lengths(es.get(name)))


def test_the_copy_scene_covers_every_alignment():
    sc = es.get("alignments")
    assert len(es.copy_triples(sc)) == 64
    ln = sorted(len(r) for r in sc[0])
    assert ln == list(range(33, 163)) and min(ln) < 64 and set(range(64, 72)) <= set(ln)   # fewer dwords than lanes; 64 + k for k in 0 .. 7
    assert {struct.unpack_from("<I", r, 16)[0] % 2 for r in sc[0]} == {0, 1}


def test_the_cut_model_on_a_stream_by_hand():
    """L = 0xff00 - 300: B = 300.  Records begin at 0, 100, 299 | 300 | 65280 (range 217) | 65400 (range 218): of 219 ranges four are written"""
    ln = [100, 199, 1, 0xFF00 - 300, 120, 30]
    b, at, sizes = em.cuts(ln)
    assert (b, at, sizes) == (300, [0, 300, 65280, 65400, 65430], [300, 64980, 120, 30])
    assert em.empty_ranges(ln) == 219 - 4


@pytest.mark.parametrize("name", list(es.SCENES))
def test_model_stream_equals_the_host_writer(name, tmp_path):
    recs, yc, yx, yd, _, _ = es.get(name)
    want = em.stream(recs, yc, yx, yd)
    got = host_tagged_stream(recs, yc, yx, yd, tmp_path)
    if got != want:                                                    # say which record differs
        o = p = 0
        for i, r in enumerate(recs):
            t = em.tag(r, yc[i], yx[i], yd[i])
            bs = struct.unpack_from("<I", got, p)[0]
            assert got[p + 4:p + 4 + bs] == t, (i, yc[i], yx[i], yd[i], r[em.aux_start(r):], got[p + 4:p + 4 + bs][em.aux_start(r):], t[em.aux_start(r):])
            o, p = o + 4 + len(t), p + 4 + bs
    assert got == want
