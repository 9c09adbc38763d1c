"""Loader of tiebrush_amd/_build/libtbk_offsets_probe.so (tests/support/offsets_probe.hip): the raw form's offsets pass of the window
path on its own.  Which kernel runs is the context's debug state (`kernel`: "wave", the default, or "block"; `og`: wg_og)."""
import ctypes as C
import os

import numpy as np
import torch

from prims_probe import _p, dev, host
from tiebrush_amd import _lib

PROBE_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libtbk_offsets_probe.so")
DERR_RAWORDER = 1 << 9       # tbk_internal.h
_probe = None


def load():
    global _probe
    if _probe is None:
        _lib.load()
        if not os.path.exists(PROBE_PATH):
            raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % PROBE_PATH)
        L = C.CDLL(PROBE_PATH)
        L.probe_offsets_raw.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.probe_offsets_raw.restype = C.c_int
        _probe = L
    return _probe


def offsets(ctx, tid, pos, run_off, W, kernel="wave", og=0):
    """numpy inputs -> (off [nW + 2, k], wbase [nW + 2], device error bits).  The outputs are filled with 0xFFFFFFFF first."""
    L = load()
    n, k, nW = len(pos), len(run_off) - 1, len(W)
    spec = ["path=window"] + (["wg_offsets=block"] if kernel == "block" else []) + (["wg_og=%d" % og] if og else [])
    ctx.set_debug(",".join(spec))
    try:
        d_tid, d_pos = dev(np.asarray(tid, np.int32)), dev(np.asarray(pos, np.int32))
        d_run, d_W = dev(np.asarray(run_off, np.uint32)), dev(np.asarray(W, np.uint64))
        off = torch.full(((nW + 2) * k,), -1, dtype=torch.int32, device="cuda:0")
        wbase = torch.full((nW + 2,), -1, dtype=torch.int32, device="cuda:0")
        err = C.c_uint32(0xFFFFFFFF)
        torch.cuda.synchronize()
        rc = L.probe_offsets_raw(ctx.h, _p(d_tid), _p(d_pos), _p(d_run), k, n, _p(d_W), nW, _p(off), _p(wbase), C.byref(err))
        assert rc == 0, "probe_offsets_raw: status %d (%s)" % (rc, ctx.last_message())
        return host(off, np.uint32).reshape(nW + 2, k), host(wbase, np.uint32), err.value
    finally:
        ctx.set_debug("")
