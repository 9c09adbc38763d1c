"""tbk_cov_stream_push on the device: every scene of stream_scenes.py, push by push, against the model (stream_model.py) —
info, every column of the view, and through the following views the carried records — and the contract the streaming rests on: the
coverage, junction and sample rows of the views, one after the other, are bit-equal to one call over the uncut records."""
import ctypes

import numpy as np
import pytest

import cov_scenes as cs
import stream_model as sm
import stream_scenes as ss

pytestmark = pytest.mark.gpu

SCENES = ss.scenes()
COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
SAMP_KEYS = ("s_tid", "s_start", "s_end", "s_count", "s_heat")
VIEW_COLS = (("tid", np.int32), ("pos", np.int32), ("flag", np.uint16), ("cig_off", np.uint32), ("cig", np.uint32), ("yc", np.float64), ("strand", np.uint8),
             ("yx", np.int64))
YC = {"integral": lambda y: y, "fractional": lambda y: y * 1.25 + 0.1}      # the lean interval chain / the ordered one


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _tile(cin):
    """a tile of one TieBrush-written file from a CovInput: the columns the push reads, the others filled in"""
    from tiebrush_amd import soa
    n = cin.n_records
    return soa.SoATile(n_files=1, file_off=np.array([0, n], np.uint32), tbmerged=np.ones(1, np.uint8), tid=cin.tid, pos=cin.pos, flag=cin.flag,
                       mapq=np.full(n, 60, np.uint8), strand=cin.strand, nh=np.full(n, soa.NH_ABSENT, np.int32), cig_off=cin.cig_off, cig=cin.cig,
                       yc_in=cin.yc, yx_in=cin.yx if cin.yx is not None else np.ones(n, np.int64), yd_in=np.zeros(n, np.int64))


def _soa_struct(ctx, tile):
    """the SoaIn struct of a SoATile (numpy: a HOST tile; to_device(): a DEVICE tile), and what keeps its arrays alive"""
    keep = []
    s, _dev, _n = ctx._soa_struct(tile, keep)
    return s, keep


def _view_to_numpy(view):
    """the columns of a DeviceCovView on the host"""
    s, n, nc = view.struct, view.n_records, view.n_cigar_ops
    hip = ctypes.CDLL("libamdhip64.so")
    out = {}
    for name, dt in VIEW_COLS:
        cnt = {"cig_off": n + 1 if n else 0, "cig": nc}.get(name, n)
        a = np.empty(cnt, dtype=dt)
        if cnt and getattr(s, name):
            assert hip.hipMemcpy(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(getattr(s, name)), ctypes.c_size_t(a.nbytes), 2) == 0
        out[name] = a
    return out


def _push(ctx, cin, final, seen):
    import torch
    from tiebrush_amd import api
    s, keep = _soa_struct(ctx, api.to_device(_tile(cin)))
    sn = torch.from_numpy(np.ascontiguousarray(seen)).to("cuda:0") if seen is not None else None
    return ctx.cov_stream_push(s, sn.data_ptr() if sn is not None else None, final)


def _assert_view(ctx, view, want, what):
    got = _view_to_numpy(view)
    w = sm.to_cin(want)
    assert view.n_records == len(want) and view.n_cigar_ops == len(w.cig), what
    if not want:
        return
    for k, dt in VIEW_COLS:
        a = np.ascontiguousarray(getattr(w, k), dtype=dt)
        assert got[k].tobytes() == a.tobytes(), (what, k)


def _assert_rows(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(w), (what, k, len(g), len(w))
        assert g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes(), (what, k)


def _with_yc(pushes, f):
    return [(cs.with_yc(cin, f), final, seen) for cin, final, seen in pushes]


def _whole(ctx, pushes, ns):
    """one coverage() / sample() over the uncut records, on the device"""
    from tiebrush_amd import api
    u = sm.uncut(pushes)
    if u.n_records == 0:
        return None, None
    d = api.to_device(u)
    return api.to_numpy(ctx.coverage(d)), api.to_numpy(ctx.sample(d, ns, cap_intervals=2 * len(u.cig) + 2 * u.n_records + 16))


@pytest.mark.parametrize("yc", sorted(YC))
@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_scene(ctx, scene, yc):
    from tiebrush_amd import api
    pushes = _with_yc(scene.pushes, YC[yc])
    want, _left = sm.run(pushes)
    ctx.cov_stream_reset()
    cov, samp, model = [], [], sm.Stream()
    for k, ((cin, final, seen), (wview, winfo)) in enumerate(zip(pushes, want)):
        view, info = _push(ctx, cin, final, seen)
        assert info == winfo, (k, info, winfo)
        _assert_view(ctx, view, wview, k)
        model.push(cin, final, seen)                                # (the model's carry: its first record is what the call reports)
        assert ctx.cov_stream_first == ((model.carry[0][0][0], model.carry[0][0][1]) if model.carry else None), k
        if view.n_records:
            cov.append(api.to_numpy(ctx.coverage(view)))
            samp.append(api.to_numpy(ctx.sample(view, scene.num_samples)))
            _assert_view(ctx, view, wview, (k, "after the coverage and sample calls"))
    wcov, wsamp = _whole(ctx, pushes, scene.num_samples)
    if wcov is None:
        assert not cov
        return
    if pushes[-1][1]:                                               # (a stream that was flushed: the views hold every record)
        _assert_rows({k: np.concatenate([c[k] for c in cov]) for k in COV_KEYS}, wcov, COV_KEYS, "coverage")
        _assert_rows({k: np.concatenate([c[k] for c in samp]) for k in SAMP_KEYS}, wsamp, SAMP_KEYS, "sample")
        assert sum(c["n_bases"] for c in cov) == wcov["n_bases"] and sum(c["span_bases"] for c in cov) == wcov["span_bases"]
    ctx.cov_stream_reset()


def test_reset_forgets_the_carry(ctx):
    sc = ss.by_name()["head0_only"]
    ctx.cov_stream_reset()
    _, info = _push(ctx, sc.pushes[0][0], False, None)
    assert info == ss.info(0, 9, 0, 0)
    ctx.cov_stream_reset()
    view, info = _push(ctx, sc.pushes[0][0], True, None)
    assert info == ss.info(9, 0, 9, 9)                              # (not 18: the first nine are gone)
    _assert_view(ctx, view, sm.tile_records(sc.pushes[0][0]), "after reset")


def test_stream_cap_refuses_and_leaves_the_carry(ctx):
    """carry + tile beyond the debug cap: TBK_E2BIG, the carry intact, and the same push under a larger cap gives the model's view"""
    from tiebrush_amd import api
    sc = ss.by_name()["carry_grows"]
    want, _ = sm.run(sc.pushes)
    ctx.cov_stream_reset()
    try:
        ctx.set_debug("stream_cap=10")
        _, info = _push(ctx, sc.pushes[0][0], False, None)
        assert info == want[0][1] and info["n_carry"] == 9
        with pytest.raises(api.TbkError) as e:
            _push(ctx, sc.pushes[1][0], False, None)               # 9 + 7 records
        assert e.value.status == -4
        first = sm.tile_records(sc.pushes[0][0])[0][0]
        assert ctx.cov_stream_first == (first[0], first[1])         # the refusal names the bundle that did not fit: the carry's first record
        ctx.set_debug("stream_cap=100")
        for k in range(1, len(sc.pushes)):
            view, info = _push(ctx, sc.pushes[k][0], sc.pushes[k][1], None)
            assert info == want[k][1], k
            _assert_view(ctx, view, want[k][0], k)
    finally:
        ctx.set_debug("")
        ctx.cov_stream_reset()


def test_host_tile_is_refused(ctx):
    from tiebrush_amd import api
    sc = ss.by_name()["touch_then_gap"]
    ctx.cov_stream_reset()
    _, info = _push(ctx, sc.pushes[0][0], False, None)
    s, keep = _soa_struct(ctx, _tile(sc.pushes[0][0]))             # numpy arrays: TBK_MEM_HOST
    with pytest.raises(api.TbkError) as e:
        ctx.cov_stream_push(s, None, True)
    assert e.value.status == -1
    view, info2 = _push(ctx, cs.mk([]), True, None)                 # the context takes the next call and the carry is still there
    assert info2 == ss.info(info["n_carry"], 0, 0, 0)
    ctx.cov_stream_reset()
