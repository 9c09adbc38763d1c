"""Every scene of tests/deflate_scenes.py proven on the exact host model of the device deflate's parse (tests/support/deflate_model.cpp,
`tokens` mode): the model's member inflates with zlib to the payload, its bytes decode (deflate_tokens) to the very tokens the model
says it chose, and the scene's predicate holds on them.  The same predicates are put to the device's own tokens in
tests/test_gpu_deflate_edges.py, whose bytes must equal the model's.

Run as a script it repeats the seed searches the scenes file records: `python tests/test_deflate_scenes_cpu.py [--switch] [--cl-limit]`."""
import sys
import zlib

import numpy as np
import pytest

import deflate_model_run as dm
import deflate_scenes as ds
import deflate_tokens as dt


def prove(name, seed=None):
    """the model's members of a scene, as Views, after every check but the predicate; -> (scene, model members, views)"""
    sc = ds.build(name, seed)
    mm = dm.run(sc.payload, sc.cuts, want_candidates=True)
    for pos, want in sc.relies.items():                       # the candidates the scene says its tokens come from
        got = dict(zip(("k4", "k8", "l4", "l8"), (int(v) for v in mm[0].cand[pos])))
        assert all(got[k] == v for k, v in want.items()), (pos, want, got)
    views = []
    for m, a, b in zip(mm, sc.cuts[:-1], sc.cuts[1:]):
        part = sc.payload[a:b]
        z = zlib.decompressobj(-15)
        assert z.decompress(m.deflate) + z.flush() == part and z.eof and not z.unused_data
        d = dt.decode(m.deflate)
        assert d.payload == part and m.n == len(part)
        v = ds.view(d)
        assert v.btype == m.btype
        if m.btype == 2:
            assert v.tokens == m.tokens                       # the reader and the model's writer agree on what was written
        else:
            assert m.deflate == b"\x01" + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
        assert bytes(dt.expand(m.tokens)) == part
        views.append(v)
    return sc, mm, views


@pytest.mark.parametrize("name", ds.names())
def test_scene_predicate_holds_on_the_model(name):
    sc, mm, views = prove(name)
    sc.check(views)


def test_scene_list_is_what_the_suite_expects():
    names = ds.names()
    assert len(names) == len(set(names)) and len(names) >= 100
    assert set(ds.SEEDS) <= set(names)
    assert sum(bool(ds.build(n).relies) for n in names) >= 8
    assert "stored_dynamic_switch" in names                  # (defined only once its search has recorded a result)


def test_switch_members_are_within_64_bits_of_the_rule():
    alpha, n, s_dyn, s_sto = ds.SWITCH
    sc, mm, views = prove("stored_dynamic_switch")
    limit = 8 * n + 32
    assert mm[0].btype == 2 and limit - 64 <= mm[0].bits < limit, (mm[0].bits, limit)
    assert mm[1].btype == 0 and limit <= mm[1].bits <= limit + 64, (mm[1].bits, limit)
    assert (mm[0].bits, mm[1].bits) == (limit - 1, limit)                              # as recorded: one bit either side of `>=`
    assert set(sc.payload[:n]) == set(sc.payload[n:]) == set(range(alpha))            # the same alphabet on both sides


def test_model_exact_mode_on_the_sweep_sizes():
    """the exact mode over members of every small length (the GPU test compares the device's bytes with these)"""
    payload, cuts = ds.sweep("text")
    few = cuts[:300]
    mm = dm.run(payload[:int(few[-1])], few, want_tokens=False)
    assert mm[0].n == 0 and mm[0].deflate == b""
    for m, a, b in zip(mm, few[:-1], few[1:]):
        if m.n:
            assert zlib.decompress(m.deflate, -15) == payload[int(a):int(b)]


# ---- the searches (not tests: their results are recorded in deflate_scenes.py) --------------------------------------------------------

def search_seeds(limit=64):
    seeds = {}
    for name in ds.names():
        if name in ("stored_dynamic_switch", "cl_limit"):
            continue
        for seed in range(limit):
            try:
                sc, mm, views = prove(name, seed)
                sc.check(views)
            except AssertionError as e:
                last = e
                continue
            if seed:
                seeds[name] = seed
            break
        else:
            print("no seed below %d for %s: %r" % (limit, name, last))
    print("SEEDS = %r" % seeds)


def search_switch(n=2000, nseeds=120):
    """the alphabet and the two seeds whose dynamic blocks lie nearest to 8 n + 32 bits from below and from above"""
    limit, best = 8 * n + 32, None
    for alpha in range(256, 128, -1):
        seeds = list(range(nseeds))
        payload = b"".join(ds.switch_member(alpha, n, s).tobytes() for s in seeds)
        mm = dm.run(payload, [n * i for i in range(len(seeds) + 1)], want_tokens=False)
        near = [s for s in seeds if abs(mm[s].bits - limit) <= 64]
        full = [s for s in near if len(set(ds.switch_member(alpha, n, s).tolist())) == alpha]
        below = sorted((limit - mm[s].bits, s) for s in full if mm[s].bits < limit)
        above = sorted((mm[s].bits - limit, s) for s in full if mm[s].bits >= limit)
        if below and above and (best is None or below[0][0] + above[0][0] < best[0]):
            best = (below[0][0] + above[0][0], alpha, below[0][1], above[0][1], limit - below[0][0], limit + above[0][0])
    if best:
        print("SWITCH = (%d, %d, %d, %d)   # bits %d and %d around %d" % (best[1], n, best[2], best[3], best[4], best[5], limit))
    else:
        print("no switch found")


def search_cl_limit(count=4000):
    """members of several families: is the code-length code ever held by its 7-bit limit?"""
    found, tried = None, 0
    for fam in ("skewed_lengths", "random_alpha", "runs"):
        parts = [ds.cl_family(fam, i).tobytes() for i in range(count // 3)]
        cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        mm = dm.run(b"".join(parts), cuts, want_tokens=False)
        for i, m in enumerate(mm):
            tried += 1
            if m.btype != 2 or found is not None:
                continue
            b = dt.decode(m.deflate).blocks[0]
            if max(b.cl_lens) == 7 and ds.unlimited_depth(ds.cl_freqs(b.lit_lens, b.dist_lens)) > 7:
                found = (fam, i)
    print("CL_LIMIT_SEARCH = (%d, %r)" % (tried, found))


if __name__ == "__main__":
    if "--switch" in sys.argv:
        search_switch()
    elif "--cl-limit" in sys.argv:
        search_cl_limit()
    else:
        search_seeds()
