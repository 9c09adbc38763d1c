"""The device deflate's parse (bgz_deflate_k, bgzdef.hip) as a checked contract: every scene of tests/deflate_scenes.py goes through
tbk_bgzf_deflate; the run is a well-formed BGZF run that zlib and the device inflate give back, the device's OWN tokens (read off
its bytes by tests/deflate_tokens.py) satisfy the scene's predicate, its deflate bytes equal the exact host model's
(tests/support/deflate_model.cpp, `tokens` mode) to the byte, and a second call writes the same bytes.  The size sweep puts members of
every length 0 .. 1100 and 0xff00 - 9 .. 0xff00 through tbk_bgzf_deflate and tbk_zlib_deflate: zlib and the model's bytes, per member.

All scenes travel in ONE call (a cut per member), twice; the model runs once."""
import zlib

import numpy as np
import pytest

import deflate_model_run as dm
import deflate_scenes as ds
import deflate_tokens as dt
from test_gpu_deflate import check_run, members

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes_run(ctx):
    """-> {scene: (payload parts, the device's member deflate bytes, the model's members)}, and the two runs"""
    payload, cuts, owner = b"", [0], []
    for name in ds.names():
        sc = ds.build(name)
        cuts += [len(payload) + c for c in sc.cuts[1:]]
        owner += [name] * (len(sc.cuts) - 1)
        payload += sc.payload
    run1 = ctx.bgzf_deflate(payload, cuts=cuts)
    run2 = ctx.bgzf_deflate(payload, cuts=cuts)
    ms = check_run(run1, payload)                                   # framing, CRC, ISIZE, zlib gives every member back
    assert [m[2] for m in ms] == [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    model = dm.run(payload, cuts)
    per = {}
    for name, m, mod, a, b in zip(owner, ms, model, cuts[:-1], cuts[1:]):
        per.setdefault(name, []).append((payload[a:b], m[0], mod))
    return per, payload, run1, run2


def test_the_run_inflates_on_the_device_and_is_the_same_twice(ctx, scenes_run):
    per, payload, run1, run2 = scenes_run
    assert run1 == run2
    assert ctx.bgzf_inflate(run1) == payload


@pytest.mark.parametrize("name", ds.names())
def test_scene_on_the_device(scenes_run, name):
    per = scenes_run[0]
    views = []
    for part, z, mod in per[name]:
        d = dt.decode(z)
        assert d.payload == part
        views.append(ds.view(d))
    ds.build(name).check(views)                                     # the predicate, on the device's own tokens
    for k, (part, z, mod) in enumerate(per[name]):
        if z != mod.deflate:
            v = views[k]
            first = next((i for i, (x, y) in enumerate(zip(v.tokens, mod.tokens)) if x != y), None) if v.btype == 2 == mod.btype else None
            assert False, "member %d: device %d bytes (BTYPE %d), model %d (BTYPE %d); first token that differs: %r" % (
                k, len(z), v.btype, len(mod.deflate), mod.btype, first and (first, v.tokens[first], mod.tokens[first]))


@pytest.mark.parametrize("kind", ds.SWEEP_CLASSES)
def test_size_sweep(ctx, kind):
    payload, cuts = ds.sweep(kind)
    model = dm.run(payload, cuts, want_tokens=False)
    run = ctx.bgzf_deflate(payload, cuts=cuts)
    ms = members(run)
    streams = ctx.zlib_deflate(payload, cuts=cuts)
    sized = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(ms) == sum(b > a for a, b in sized) and len(streams) == len(sized)
    k = 0
    for (a, b), mod, zs in zip(sized, model, streams):
        part = payload[a:b]
        assert zlib.decompress(zs) == part, (a, b)                                   # (header, deflate bytes, Adler-32)
        if b == a:
            assert zs == b"\x78\x9c\x03\x00\x00\x00\x00\x01"                         # an empty piece: no BGZF member, an empty stream
            continue
        z, crc, isize = ms[k]
        k += 1
        assert isize == b - a and crc == zlib.crc32(part) and zlib.decompress(z, -15) == part, (a, b)
        assert z == mod.deflate, "member of %d bytes at %d: the device's bytes are not the model's" % (b - a, a)
        assert zs[2:-4] == z, (a, b)
