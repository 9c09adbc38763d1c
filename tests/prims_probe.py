"""Loader of tiebrush_amd/_build/libtbk_probe.so (tests/support/prims_probe.hip): the library's device-wide primitives, each on its
own.  Arguments are torch device tensors; every call waits for torch's work first, because a context runs on a stream of its own,
and returns when the primitive has finished."""
import ctypes as C
import os

import numpy as np
import torch

from tiebrush_amd import _lib

PROBE_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libtbk_probe.so")
DERR_INTERNAL, DERR_BIGBUCKET = 1 << 7, 1 << 8     # tbk_internal.h
_P = C.c_void_p
_probe = None


def load():
    global _probe
    if _probe is None:
        _lib.load()      # first: the probe's NEEDED libtbk.so (and through it the HIP runtime torch brought) is then the loaded one
        if not os.path.exists(PROBE_PATH):
            raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % PROBE_PATH)
        L = C.CDLL(PROBE_PATH)
        L.probe_exscan.argtypes = [_P, _P, _P, C.c_uint32, C.c_int, _P]
        L.probe_radix128.argtypes = [_P, _P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int]
        L.probe_radix_w64.argtypes = [_P, _P, C.c_uint32, C.c_uint64, C.c_int, _P, _P]
        L.probe_sort_runs.argtypes = [_P, _P, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P]
        L.probe_scan.argtypes = [_P, _P, _P, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P, _P, _P, _P]
        L.probe_scan_two.argtypes = [_P, _P, _P, C.c_uint32, C.c_int, _P, _P, _P, _P, _P]
        for f in (L.probe_exscan, L.probe_radix128, L.probe_radix_w64, L.probe_sort_runs, L.probe_scan, L.probe_scan_two):
            f.restype = C.c_int
        _probe = L
    return _probe


def _p(t):
    return _P(t.data_ptr()) if t is not None and t.numel() else None


def dev(a):
    """numpy array (unsigned types go as their bit patterns) -> device tensor"""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to("cuda:0")


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _ok(ctx, rc, what):
    assert rc == 0, "%s: status %d (%s)" % (what, rc, ctx.last_message())


def exscan(ctx, d_in, n, u64, with_total):
    """-> (out tensor, total or None)"""
    out = torch.full((max(n, 1),), -1, dtype=torch.int64 if u64 else torch.int32, device="cuda:0")
    tot = torch.full((1,), -1, dtype=torch.int64, device="cuda:0") if with_total else None
    torch.cuda.synchronize()
    _ok(ctx, load().probe_exscan(ctx.h, _p(d_in), _p(out), n, int(u64), _p(tot)), "probe_exscan")
    return out[:n], (int(host(tot, np.uint64)[0]) if with_total else None)


def radix128(ctx, hi, lo, val, n, only_hi=2**64 - 1, only_lo=2**64 - 1, exact=False):
    torch.cuda.synchronize()
    _ok(ctx, load().probe_radix128(ctx.h, _p(hi), _p(lo), _p(val), n, only_hi, only_lo, int(exact)), "probe_radix128")


def radix_w64(ctx, w, n, mask, exact=False, emit=False):
    """-> None, or (calls [n + 1], words [n]) of the emit functor"""
    calls = words = None
    if emit:
        calls = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
        words = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    _ok(ctx, load().probe_radix_w64(ctx.h, _p(w), n, mask, int(exact), _p(calls), _p(words)), "probe_radix_w64")
    return (calls, words[:n]) if emit else None


def sort_runs(ctx, side_a, side_b, n_hi, run_off, nruns):
    """side_a = (hi, lo, val) holds the runs, side_b the other side -> (device error bits, result side, other side)"""
    err = (C.c_uint32 * 2)(0, 0)
    torch.cuda.synchronize()
    _ok(ctx, load().probe_sort_runs(ctx.h, _p(side_a[0]), _p(side_a[1]), _p(side_a[2]), n_hi, _p(run_off), nruns, err, _p(side_b[0]), _p(side_b[1]),
                                    _p(side_b[2])), "probe_sort_runs")
    res, other = (side_b, side_a) if err[1] else (side_a, side_b)
    return int(err[0]), res, other


def scan(ctx, flag, value, n, words, form, delay_index=0, delay_ticks=0):
    """-> (element, inclusive, exclusive) as [words, n] tensors, device error bits"""
    outs = [torch.full((words, n), -1, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    err = C.c_uint32(0xFFFFFFFF)
    torch.cuda.synchronize()
    _ok(ctx, load().probe_scan(ctx.h, _p(flag), _p(value), n, words, form, delay_index, delay_ticks, _p(outs[0]), _p(outs[1]), _p(outs[2]), C.byref(err)),
        "probe_scan")
    return outs, err.value


def scan_two(ctx, flag, value, n, E):
    """-> inclusive [3, n], exclusive [3, n], term [n], terms before [n], device error bits"""
    inc, exc = (torch.full((3, n), -1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    term, before = (torch.full((n,), -1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    err = C.c_uint32(0xFFFFFFFF)
    torch.cuda.synchronize()
    _ok(ctx, load().probe_scan_two(ctx.h, _p(flag), _p(value), n, E, _p(inc), _p(exc), _p(term), _p(before), C.byref(err)), "probe_scan_two")
    return inc, exc, term, before, err.value
