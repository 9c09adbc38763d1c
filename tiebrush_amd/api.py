"""Host-side Python mirror of the hot-path boundary (`include/tbk.h`).

`Context.collapse` stands where the reference's tiebrush main loop stands
(/root/reference/src/tiebrush.cpp:570-592: TInputFiles::next + passes_options + addPData +
flushPData), `Context.coverage` where tiecov's loop stands (tiecov.cpp:435-513).  Arrays may be
numpy (TBK_MEM_HOST: staged by the library) or torch CUDA tensors (TBK_MEM_DEVICE: used in
place, resident in HBM).  torch is plumbing only: device memory + streams.
"""
from __future__ import annotations

import contextlib
import os
import ctypes as C
from dataclasses import replace

import numpy as np

from . import _lib
from ._lib import TbkError
from .soa import CovInput, SoATile


def _torch():
    import torch
    return torch


def _is_torch(a):
    return a is not None and type(a).__module__.startswith("torch")


def _addr(a, dtype, keep, n=None):
    """Pointer of a numpy array / torch tensor after a dtype + contiguity check."""
    if a is None:
        return None
    if _is_torch(a):
        torch = _torch()
        want = {np.int32: torch.int32, np.uint32: torch.int32, np.uint16: torch.int16, np.uint8: torch.uint8,
                np.float64: torch.float64, np.int64: torch.int64, np.uint64: torch.int64, np.float32: torch.float32}[dtype]
        # unsigned types travel as their signed twins of the same width (torch has no uint32 storage maths we need)
        if a.dtype != want and a.element_size() != np.dtype(dtype).itemsize:
            raise TypeError("tensor dtype %s does not match %s" % (a.dtype, dtype))
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        if n is not None and a.numel() < n:
            raise ValueError("tensor too small: %d < %d" % (a.numel(), n))
        keep.append(a)
        return a.data_ptr()
    b = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and b.size < n:
        raise ValueError("array too small: %d < %d" % (b.size, n))
    keep.append(b)
    return b.ctypes.data


def to_device(obj, device="cuda:0"):
    """Copy the per-record arrays of a SoATile / CovInput into HBM (torch tensors)."""
    torch = _torch()

    def mv(a, dt):
        if a is None:
            return None
        b = np.ascontiguousarray(a, dtype=dt)
        sd = {np.uint32: np.int32, np.uint16: np.int16, np.uint64: np.int64}.get(dt, dt)
        return torch.from_numpy(b.view(sd)).to(device)

    if isinstance(obj, SoATile):
        r = replace(obj, tid=mv(obj.tid, np.int32), pos=mv(obj.pos, np.int32), flag=mv(obj.flag, np.uint16),
                       mapq=mv(obj.mapq, np.uint8), strand=mv(obj.strand, np.uint8), nh=mv(obj.nh, np.int32),
                       cig_off=mv(obj.cig_off, np.uint32), cig=mv(obj.cig, np.uint32), yc_in=mv(obj.yc_in, np.float64),
                       yx_in=mv(obj.yx_in, np.int64), yd_in=mv(obj.yd_in, np.int64), md_off=mv(obj.md_off, np.uint32),
                       md=mv(obj.md, np.uint8), md_has=mv(obj.md_has, np.uint8),
                       qname_hash=mv(obj.qname_hash, np.uint64), qn_off=mv(obj.qn_off, np.uint32), qn=mv(obj.qn, np.uint8),
                       prio_hi=mv(obj.prio_hi, np.uint64), prio_lo=mv(obj.prio_lo, np.uint64))
        torch.cuda.synchronize()
        return r
    if isinstance(obj, CovInput):
        r = replace(obj, tid=mv(obj.tid, np.int32), pos=mv(obj.pos, np.int32), flag=mv(obj.flag, np.uint16),
                       cig_off=mv(obj.cig_off, np.uint32), cig=mv(obj.cig, np.uint32), yc=mv(obj.yc, np.float64),
                       strand=mv(obj.strand, np.uint8), yx=mv(obj.yx, np.int64))
        torch.cuda.synchronize()
        return r
    raise TypeError(type(obj))


def _numel(a):
    return int(a.numel()) if _is_torch(a) else int(np.asarray(a).size)


class DeviceTile:
    """a tile living in context-owned device memory (tbk_unpack_tile): goes to collapse() like a SoATile"""

    def __init__(self, struct, n_files, keep):
        self.struct, self.n_files, self._keep = struct, n_files, keep
        self.n_records = int(struct.n_records)


class DeviceCovView:
    """tbk_cov_in view living in context-owned device memory (valid until the next call)."""

    def __init__(self, struct, n_records, n_cigar_ops):
        self.struct = struct
        self.n_records = n_records
        self.n_cigar_ops = n_cigar_ops


class _FollowDebug:
    """The library reads TBK_DEBUG once, when a context is created (tbk_create).  This binding is what the tests drive, and a test changes
    the variable between two calls on one context: before a call goes out, the context is told (tbk_set_debug) when the variable has
    changed since the last one."""

    def __init__(self, lib, ctx):
        self._lib, self._ctx = lib, ctx

    def __getattr__(self, name):
        self._ctx._follow_debug()
        return getattr(self._lib, name)


class Context:
    def __init__(self, device: int = 0):
        lib = _lib.load()
        h = C.c_void_p()
        self._debug_spec = os.environ.get("TBK_DEBUG", "")
        rc = lib.tbk_create(int(device), C.byref(h))
        if rc != 0:
            raise TbkError(rc, "tbk_create(device=%d)" % device)
        self._lib = lib
        self.L = _FollowDebug(lib, self)
        self.h = h
        self.device = device
        self._on_torch_stream = False

    def _follow_debug(self):
        spec = os.environ.get("TBK_DEBUG", "")
        if spec != self._debug_spec and getattr(self, "h", None):
            self._debug_spec = spec
            self._lib.tbk_set_debug(self.h, spec.encode())

    def set_debug(self, spec: str):
        """tbk_set_debug: test hooks / forced paths of this context ("key=value,..."; "" = the defaults)"""
        self._debug_spec = os.environ.get("TBK_DEBUG", "")      # (an explicit setting stays until the variable changes again)
        self._check(self._lib.tbk_set_debug(self.h, spec.encode()), "tbk_set_debug")

    def close(self):
        if getattr(self, "h", None):
            self._lib.tbk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ---------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise TbkError(rc, "%s: %s" % (what, (self.L.tbk_last_error(self.h) or b"").decode()))

    def use_torch_stream(self):
        """Launch on torch's current stream so that torch ops and our kernels order correctly."""
        s = _torch().cuda.current_stream(self.device).cuda_stream
        self._check(self.L.tbk_set_stream(self.h, C.c_void_p(s if s else 1)), "tbk_set_stream")   # (0 = the default stream: TBK_STREAM_DEFAULT)
        self._on_torch_stream = True

    def _order_after_torch(self, dev):
        """Device inputs were produced on torch's stream; the context launches on its own stream unless
        use_torch_stream() was called: make the producer visible first."""
        if dev and not self._on_torch_stream:
            _torch().cuda.current_stream(self.device).synchronize()   # (of THIS context's device: the current device is per thread)

    def last_message(self) -> str:
        return (self.L.tbk_last_error(self.h) or b"").decode()

    def collapse_route(self) -> dict:
        """tbk_last_route: the route the last collapse on this context took — form ("raw" / "compacted" window path, "sort", "none": no
        result), reseeds, raw_handed_back, big_bucket; with the debug key wg_stats=1 also nw, nw_live, ovf1, ovf2 of the window path"""
        r = _lib.CollapseRoute()
        self._check(self._lib.tbk_last_route(self.h, C.byref(r)), "tbk_last_route")
        d = dict(form=_lib.ROUTE_FORMS[int(r.form)], reseeds=int(r.reseeds), raw_handed_back=bool(r.raw_handed_back),
                 big_bucket=bool(r.big_bucket))
        if r.wg_stats:
            d.update(nw=int(r.nw), nw_live=int(r.nw_live), ovf1=int(r.ovf1), ovf2=int(r.ovf2))
        return d

    def stream_ptr(self):
        return self.L.tbk_get_stream(self.h)

    def set_profiling(self, on: bool):
        self._check(self.L.tbk_set_profiling(self.h, 1 if on else 0), "tbk_set_profiling")

    def kernel_times(self):
        arr = (_lib.KernelTime * 128)()
        n = self.L.tbk_kernel_times(self.h, arr, 128)
        return {arr[i].name.decode(): (float(arr[i].ms), int(arr[i].launches)) for i in range(min(n, 128))}

    def _alloc(self, device_mode, n, dtype):
        n = max(int(n), 1)
        if device_mode:
            torch = _torch()
            td = {np.int32: torch.int32, np.uint32: torch.int32, np.uint8: torch.uint8, np.float64: torch.float64,
                  np.int64: torch.int64, np.uint64: torch.int64, np.float32: torch.float32}[dtype]
            return torch.empty(n, dtype=td, device="cuda:%d" % self.device)
        return np.empty(n, dtype=dtype)

    @staticmethod
    def _trim(a, n, dtype):
        if _is_torch(a):
            return a[:n]
        return a[:n].view(dtype) if a.dtype != dtype else a[:n]

    # ---- collapse -----------------------------------------------------------------------------
    def make_opts(self, strategy="cigar", max_nh=2**31 - 1, min_qual=-1, keep_supplementary=False,
                  keep_secondary=False, keep_unmapped=False, collapse_same=False, store_frac=False, flags_mask=0,
                  defer_yd=False, keep_results=False):
        o = _lib.CollapseOpts()
        self.L.tbk_collapse_opts_default(C.byref(o))
        o.strategy = _lib.STRAT[strategy] if isinstance(strategy, str) else int(strategy)
        o.max_nh, o.min_qual, o.flags_mask = int(max_nh), int(min_qual), int(flags_mask)
        o.keep_supplementary, o.keep_secondary = int(keep_supplementary), int(keep_secondary)
        o.keep_unmapped, o.collapse_same, o.store_frac = int(keep_unmapped), int(collapse_same), int(store_frac)
        o.defer_yd = int(defer_yd)
        o.keep_results = int(keep_results)
        return o

    def finish_yd(self):
        """Wait for a deferred YD stage (collapse(..., defer_yd=True)); the `yd` array is complete afterwards."""
        self._check(self.L.tbk_collapse_finish_yd(self.h), "tbk_collapse_finish_yd")

    def unpack_tile(self, pt) -> DeviceTile:
        """tbk_unpack_tile: a soa.PackedTile (numpy, or torch tensors in pinned host memory) -> the tile on the device"""
        keep = []

        def addr(a, dt):
            if _is_torch(a):
                keep.append(a)
                return a.data_ptr() if a.numel() else None
            b = np.ascontiguousarray(a, dtype=dt)
            keep.append(b)
            return b.ctypes.data if b.size else None

        fo = np.ascontiguousarray(pt.file_off, dtype=np.uint32)
        re_, rt = np.ascontiguousarray(pt.tid_run_end, np.uint32), np.ascontiguousarray(pt.tid_run_tid, np.int32)
        keep += [fo, re_, rt]
        p = _lib.PackedIn(pt.n_files, _numel(pt.pos), _numel(pt.cig), len(re_), fo.ctypes.data, re_.ctypes.data, rt.ctypes.data, addr(pt.pos, np.int32),
                          addr(pt.meta, np.uint32), addr(pt.ncig, np.uint8), addr(pt.cig, np.uint32), _numel(pt.nh_esc_idx), _numel(pt.ncig_esc_idx),
                          addr(pt.nh_esc_idx, np.uint32), addr(pt.nh_esc_val, np.int32), addr(pt.ncig_esc_idx, np.uint32),
                          addr(pt.ncig_esc_val, np.uint32))
        s = _lib.SoaIn()
        self._check(self.L.tbk_unpack_tile(self.h, C.byref(p), C.byref(s)), "tbk_unpack_tile")
        return DeviceTile(s, pt.n_files, keep)

    def _soa_struct(self, tile: SoATile, keep):
        if isinstance(tile, DeviceTile):
            keep.append(tile)
            return tile.struct, True, tile.n_records
        dev = _is_torch(tile.tid)
        n = _numel(tile.tid)
        nc = _numel(tile.cig)
        fo = np.ascontiguousarray(tile.file_off, dtype=np.uint32)
        tb = np.ascontiguousarray(tile.tbmerged, dtype=np.uint8)
        keep += [fo, tb]
        s = _lib.SoaIn(
            _lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, tile.n_files, n, nc, fo.ctypes.data, tb.ctypes.data,
            _addr(tile.tid, np.int32, keep, n), _addr(tile.pos, np.int32, keep, n), _addr(tile.flag, np.uint16, keep, n),
            _addr(tile.mapq, np.uint8, keep, n), _addr(tile.strand, np.uint8, keep, n), _addr(tile.nh, np.int32, keep, n),
            _addr(tile.cig_off, np.uint32, keep, n + 1), _addr(tile.cig, np.uint32, keep, nc),
            _addr(tile.yc_in, np.float64, keep, n), _addr(tile.yx_in, np.int64, keep, n),
            _addr(tile.yd_in, np.int64, keep, n), _addr(tile.md_off, np.uint32, keep, n + 1),
            _addr(tile.md, np.uint8, keep), _addr(tile.md_has, np.uint8, keep, n),
            _addr(tile.qname_hash, np.uint64, keep, n), _addr(tile.prio_hi, np.uint64, keep, n),
            _addr(tile.prio_lo, np.uint64, keep, n), _addr(tile.qn_off, np.uint32, keep, n + 1), _addr(tile.qn, np.uint8, keep))
        return s, dev, n

    def collapse(self, tile: SoATile, opts=None, want_coords=True, want_rec_group=False, want_effend=False, out=None,
                 raw=False, want_key=None, cap_groups=None, **kw):
        """Collapse one tile.  Returns a dict (rep, yc, yx, yd[, g_start, g_end, rec_group, g_key], n_groups,
        n_passed) in the reference's output order.  `out` may carry preallocated buffers to reuse.
        want_key (default: device tiles): tbk_groups_out.g_key — groups_to_cov_in then builds the tiecov input of the
        representatives from the keys instead of fetching every representative."""
        o = opts if opts is not None else self.make_opts(**kw)
        keep = []
        s, dev, n = self._soa_struct(tile, keep)
        self._order_after_torch(dev)
        # capacity of the group arrays: one group per record can never overflow (the default); a caller that knows its data
        # collapses (cap_groups, e.g. a quarter of the records) saves the memory, and a call that needs more says how many
        # (TBK_E2BIG with n_groups = the need) and is repeated once with that
        cap = max(n if cap_groups is None else min(int(cap_groups), n), 1)
        bufs = out if out is not None else {}
        if bufs.get("_cap_groups", 0) > cap:
            cap = bufs["_cap_groups"]
        res = self._collapse_once(o, s, dev, n, cap, bufs, keep, want_coords, want_rec_group, want_effend, want_key, raw)
        if isinstance(res, int):                    # TBK_E2BIG: res groups are needed
            bufs["_cap_groups"] = cap = min(n, res + res // 16 + 1)
            res = self._collapse_once(o, s, dev, n, cap, bufs, keep, want_coords, want_rec_group, want_effend, want_key, raw)
            assert not isinstance(res, int)
        return res

    def _collapse_once(self, o, s, dev, n, cap, bufs, keep, want_coords, want_rec_group, want_effend, want_key, raw):

        def buf(name, count, dt, wanted=True):
            if not wanted:
                return None
            if name not in bufs or _numel(bufs[name]) < count:
                bufs[name] = self._alloc(dev, count, dt)
            return bufs[name]

        rep, yc = buf("rep", cap, np.uint32), buf("yc", cap, np.float64)
        yx, yd = buf("yx", cap, np.int64), buf("yd", cap, np.int32)
        gs, ge = buf("g_start", cap, np.int32, want_coords), buf("g_end", cap, np.int32, want_coords)
        rg = buf("rec_group", max(n, 1), np.int32, want_rec_group)
        re_ = buf("rep_effend", cap, np.int32, want_effend)
        want_key = bool(dev) if want_key is None else want_key
        gk = buf("g_key", 2 * cap, np.uint64, want_key)
        g = _lib.GroupsOut(s.mem, cap, _addr(rep, np.uint32, keep), _addr(yc, np.float64, keep),
                           _addr(yx, np.int64, keep), _addr(yd, np.int32, keep), _addr(gs, np.int32, keep),
                           _addr(ge, np.int32, keep), _addr(rg, np.int32, keep), _addr(re_, np.int32, keep),
                           _addr(gk, np.uint64, keep), 0, 0)
        rc = self.L.tbk_collapse_tile(self.h, C.byref(o), C.byref(s), C.byref(g))
        if rc == -4 and int(g.n_groups) > cap:      # TBK_E2BIG on the group arrays: the call reported the need
            return int(g.n_groups)
        self._check(rc, "tbk_collapse_tile")
        m = int(g.n_groups)
        res = dict(n_groups=m, n_passed=int(g.n_passed), _bufs=bufs, _struct=g, _soa=s, _keep=keep)
        if raw:
            return res
        res.update(rep=self._trim(rep, m, np.uint32), yc=yc[:m], yx=yx[:m], yd=yd[:m])
        if want_coords:
            res.update(g_start=gs[:m], g_end=ge[:m])
        if want_rec_group:
            res["rec_group"] = rg[:n]
        if want_effend:
            res["rep_effend"] = re_[:m]
        if want_key:
            res["g_key"] = gk[:2 * m]
        return res

    def groups_to_cov_in(self, collapse_result) -> DeviceCovView:
        """Device-side chain tiebrush -> tiecov (tbk_groups_to_cov_in)."""
        v = _lib.CovIn()
        self._order_after_torch(True)
        self._check(self.L.tbk_groups_to_cov_in(self.h, C.byref(collapse_result["_soa"]),
                                                C.byref(collapse_result["_struct"]), C.byref(v)),
                    "tbk_groups_to_cov_in")
        return DeviceCovView(v, int(v.n_records), int(v.n_cigar_ops))

    # ---- BGZF on the device -------------------------------------------------------------------------
    def bgzf_inflate(self, comp: bytes) -> bytes:
        """tbk_bgzf_inflate: whole BGZF members -> their payload (host bytes in, host bytes out)"""
        src = np.frombuffer(comp, dtype=np.uint8)
        need = C.c_uint64(0)
        out = np.empty(max(1, 4 * len(src) + 65536), dtype=np.uint8)
        rc = self.L.tbk_bgzf_inflate(self.h, src.ctypes.data, len(src), out.ctypes.data, out.size, C.byref(need), _lib.TBK_MEM_HOST)
        if rc == -4:    # TBK_E2BIG: the call reported the size
            out = np.empty(int(need.value), dtype=np.uint8)
            rc = self.L.tbk_bgzf_inflate(self.h, src.ctypes.data, len(src), out.ctypes.data, out.size, C.byref(need), _lib.TBK_MEM_HOST)
        self._check(rc, "tbk_bgzf_inflate")
        return out[:int(need.value)].tobytes()

    def bgzf_deflate(self, payload: bytes, cuts=None) -> bytes:
        """tbk_bgzf_deflate: a byte run -> whole BGZF members (host bytes in, host bytes out); cuts = payload offsets of the member
        boundaries ([0, ..., len(payload)]), default one member per 0xff00 bytes"""
        src = np.frombuffer(payload, dtype=np.uint8)
        need = C.c_uint64(0)
        out = np.empty(len(src) + (len(src) // 0xff00 + 2 + (len(cuts) if cuts is not None else 0)) * 64 + 4096, dtype=np.uint8)
        cp, nm = None, 0
        if cuts is not None:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            cp, nm = cuts.ctypes.data, len(cuts) - 1
        rc = self.L.tbk_bgzf_deflate(self.h, src.ctypes.data if len(src) else None, len(src), _lib.TBK_MEM_HOST, cp, nm, out.ctypes.data, out.size,
                                     C.byref(need))
        if rc == -4:
            out = np.empty(int(need.value), dtype=np.uint8)
            rc = self.L.tbk_bgzf_deflate(self.h, src.ctypes.data, len(src), _lib.TBK_MEM_HOST, cp, nm, out.ctypes.data, out.size, C.byref(need))
        self._check(rc, "tbk_bgzf_deflate")
        return out[:int(need.value)].tobytes()

    def kept_results(self, first, n, tags_only=False):
        """tbk_kept_results: groups [first, first + n) of the results the last collapse(..., keep_results=True) left on the context"""
        rep, yc, yx, yd = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n, np.int32)
        self._check(self.L.tbk_kept_results(self.h, first, n, None if tags_only else rep.ctypes.data, yc.ctypes.data, yx.ctypes.data, yd.ctypes.data),
                    "tbk_kept_results")
        return (None if tags_only else rep), yc, yx, yd

    def bam_encode(self, rep, yc, yx, yd, n_dev=0, host_records=None, kept_first=None, from_ctx=None):
        """tbk_bam_encode: the output records of a collapse -> (run of BGZF members, payload bytes).  rep < n_dev: records of the tile
        bam_decode left on this context; the others come from host_records = {group index: raw record bytes WITHOUT block_size}.
        kept_first: the len(rep) groups from that index on of the results the context kept (keep_results): rep / yc / yx / yd are not handed over;
        from_ctx: the Context that holds them (and the decoded tile), when it is not this one"""
        return self._bam_encode(rep, yc, yx, yd, n_dev, host_records, kept_first, from_ctx, None)

    def bam_encode_indexed(self, rep, yc, yx, yd, ref_len, n_dev=0, host_records=None, kept_first=None, from_ctx=None, csi_depth=None):
        """tbk_bam_encode_indexed: bam_encode's (run, payload bytes) and the run's index part (BAI) as a dict of numpy arrays:
        chunks (structured: tid, bin, beg, end), lin (uint64, UINT64_MAX = no record) with lin_first, refs (structured: tid, n_records, first,
        last), rec_vbeg (uint64 [n + 1]).  Virtual offsets are relative to the run's first byte.  ref_len: the header's reference lengths.
        csi_depth: None for the BAI's bins (references up to 2^29); an integer d for a CSI's bins of that depth (tbk_ix_opts.reserved = d + 1:
        references up to 2^(14 + 3 d), d <= 6)"""
        if csi_depth is not None and not 0 <= int(csi_depth) < 2 ** 32 - 1:
            raise ValueError("csi_depth must be None or a non-negative integer")
        return self._bam_encode(rep, yc, yx, yd, n_dev, host_records, kept_first, from_ctx, np.ascontiguousarray(ref_len, dtype=np.uint32),
                                0 if csi_depth is None else int(csi_depth) + 1)

    def _bam_encode(self, rep, yc, yx, yd, n_dev, host_records, kept_first, from_ctx, ref_len, ix_format=0):
        rep = np.ascontiguousarray(rep, dtype=np.uint32)
        n = len(rep)
        e = _lib.EncIn()
        if kept_first is None:
            yc = np.ascontiguousarray(yc, dtype=np.float64)
            yx = np.ascontiguousarray(yx, dtype=np.int64)
            yd = np.ascontiguousarray(yd, dtype=np.int32)
            e.mem, e.n, e.rep, e.yc, e.yx, e.yd, e.n_dev = _lib.TBK_MEM_HOST, n, rep.ctypes.data, yc.ctypes.data, yx.ctypes.data, yd.ctypes.data, n_dev
        else:
            e.mem, e.n, e.n_dev, e.first = _lib.TBK_MEM_KEPT, n, n_dev, int(kept_first)
        if from_ctx is not None:                  # another Context whose kept results / decoded tile this call reads (tbk_enc_in.from)
            e.from_ctx = from_ctx.h
        keep = []
        if host_records:
            slot = np.zeros(n, dtype=np.uint32)
            blobs, off = [], [0]
            for k, g in enumerate(sorted(host_records)):
                r = host_records[g]
                slot[g] = k
                blobs.append(len(r).to_bytes(4, "little") + r)
                off.append(off[-1] + 4 + len(r))
            blob = np.frombuffer(b"".join(blobs), dtype=np.uint8)
            offa = np.asarray(off, dtype=np.uint64)
            keep = [slot, blob, offa]
            e.n_host, e.host_blob, e.host_off, e.host_slot = len(blobs), blob.ctypes.data, offa.ctypes.data, slot.ctypes.data
        need, pay = C.c_uint64(0), C.c_uint64(0)
        out = np.empty(max(1 << 16, 64 * n), dtype=np.uint8)
        if ref_len is None:
            call = lambda: self.L.tbk_bam_encode(self.h, C.byref(e), out.ctypes.data, out.size, C.byref(need), C.byref(pay))
        else:
            vb = np.zeros(n + 1, dtype=np.uint64)
            io, part = _lib.IxOpts(), _lib.IxPart()
            io.n_ref, io.reserved, io.ref_len, io.rec_vbeg = len(ref_len), ix_format, ref_len.ctypes.data, vb.ctypes.data
            call = lambda: self.L.tbk_bam_encode_indexed(self.h, C.byref(e), out.ctypes.data, out.size, C.byref(need), C.byref(pay), C.byref(io), C.byref(part))
        rc = call()
        if rc == -4:
            out = np.empty(int(need.value), dtype=np.uint8)
            rc = call()
        self._check(rc, "tbk_bam_encode" if ref_len is None else "tbk_bam_encode_indexed")
        del keep
        run = out[:int(need.value)].tobytes()
        if ref_len is None:
            return run, int(pay.value)

        def arr(ptr, count, dt):  # (the part's arrays are the context's: copied out before its next call)
            if not count:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dt).itemsize), dtype=dt).copy()
        chunk_dt = np.dtype([("tid", "<i4"), ("bin", "<u4"), ("beg", "<u8"), ("end", "<u8")])
        ref_dt = np.dtype([("tid", "<i4"), ("reserved", "<u4"), ("n_records", "<u8"), ("first", "<u8"), ("last", "<u8")])
        return run, int(pay.value), {"chunks": arr(part.chunks, part.n_chunks, chunk_dt), "lin": arr(part.lin, part.n_lin, np.dtype("<u8")),
                                     "lin_first": int(part.lin_first), "refs": arr(part.refs, part.n_refs, ref_dt), "rec_vbeg": vb}

    def bam_decode(self, files, tbmerged=None, want_md=False, want_names=False):
        """tbk_bam_decode: list of whole BAM files (bytes) -> (SoaIn struct describing the device-resident tile, file_off).
        The struct can go straight to collapse_struct(); its arrays live in the context until bam_release()."""
        k = len(files)
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        ptrs = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
        sizes = np.array([len(b) for b in bufs], dtype=np.uint64)
        tb = np.ascontiguousarray(tbmerged if tbmerged is not None else np.zeros(k, np.uint8), dtype=np.uint8)
        fo = np.zeros(k + 1, dtype=np.uint32)
        s = _lib.SoaIn()
        self._check(self.L.tbk_bam_decode(self.h, k, ptrs, sizes.ctypes.data, tb.ctypes.data, int(want_md), int(want_names), C.byref(s),
                                          fo.ctypes.data), "tbk_bam_decode")
        self._bam_keep = (bufs, tb, fo)
        return s, fo

    def bam_decode_spans(self, spans, n_ref):
        """tbk_bam_decode_spans: spans = [(bytes of whole BGZF members, first_uoff, last_uoff)] -> (SoaIn struct of the device-resident
        tile, span_off [n_spans + 1], tag_seen: device pointer of the per-record YC / YX presence bits, or None).  The arrays live in the
        context until bam_release() or the next decode."""
        k = len(spans)
        bufs = [np.frombuffer(z, dtype=np.uint8) for z, _, _ in spans]
        ptrs = (C.c_void_p * max(k, 1))(*[b.ctypes.data if len(b) else None for b in bufs])
        sizes = np.array([len(b) for b in bufs], dtype=np.uint64)
        fu = np.array([s[1] for s in spans], dtype=np.uint32)
        lu = np.array([s[2] for s in spans], dtype=np.uint32)
        so = np.zeros(k + 1, dtype=np.uint32)
        s, seen = _lib.SoaIn(), C.c_void_p()
        self._check(self.L.tbk_bam_decode_spans(self.h, k, ptrs, sizes.ctypes.data, fu.ctypes.data, lu.ctypes.data, int(n_ref), C.byref(s), so.ctypes.data,
                                                C.byref(seen)), "tbk_bam_decode_spans")
        self._bam_keep = (bufs, so)
        return s, so, seen.value

    # ---- the region entries: one region (tid, beg, end) or a table [(tid, beg, end)] (tbk_regions).  Each pair of
    # methods shares one body, given the C entry and the arguments that name the selection. ----
    def _region_view(self, name, tile_struct, tag_seen, sel) -> DeviceCovView:
        v, nk = _lib.CovIn(), C.c_uint32(0)
        self._check(getattr(self.L, name)(self.h, C.byref(tile_struct), tag_seen, *sel, C.byref(v), C.byref(nk)), name)
        assert int(nk.value) == int(v.n_records)
        return DeviceCovView(v, int(v.n_records), int(v.n_cigar_ops))

    def region_view(self, tile_struct, tag_seen, tid, beg, end) -> DeviceCovView:
        """tbk_region_view: the records of a device tile (bam_decode_spans / bam_decode) overlapping [beg, end) on tid, as tiecov's input"""
        return self._region_view("tbk_region_view", tile_struct, tag_seen, (int(tid), int(beg), int(end)))

    def regions_view(self, tile_struct, tag_seen, table) -> DeviceCovView:
        """tbk_regions_view: the records of a device tile overlapping any interval of the table, as tiecov's input"""
        u, _keep = _regions(table)
        return self._region_view("tbk_regions_view", tile_struct, tag_seen, (C.byref(u),))

    # ---- a record stream in tiles ----
    def bam_decode_open(self, comp, first_uoff, n_ref):
        """tbk_bam_decode_open: bytes of whole BGZF members whose record stream starts at first_uoff of the first member's payload and
        may end inside a record -> (SoaIn struct of the device-resident tile of the whole records, tag_seen: device pointer or None,
        tail_off: the inflated offset of the first byte no whole record consumed).  The arrays live in the context until bam_release()
        or the next decode."""
        buf = np.frombuffer(comp, dtype=np.uint8)
        s, seen, tail = _lib.SoaIn(), C.c_void_p(), C.c_uint64(0)
        self._check(self.L.tbk_bam_decode_open(self.h, buf.ctypes.data if len(buf) else None, len(buf), int(first_uoff), int(n_ref), C.byref(s), C.byref(seen),
                                               C.byref(tail)), "tbk_bam_decode_open")
        self._bam_keep = (buf,)
        return s, seen.value, int(tail.value)

    def cov_stream_push(self, tile_struct, tag_seen, final):
        """tbk_cov_stream_push: the next tile of a record stream (a SoaIn struct of a device tile: bam_decode_open / bam_decode_spans) -> (DeviceCovView of the carried records and the tile's mapped records before its last bundle head, info
        dict n_view / n_carry / n_taken / cut).  The records from that head on wait in the context for the next push; final: nothing
        waits.  The view is valid until the next push or cov_stream_reset()."""
        v, info = _lib.CovIn(), _lib.CovStreamInfo()
        self._order_after_torch(True)
        rc = self.L.tbk_cov_stream_push(self.h, C.byref(tile_struct), tag_seen, int(bool(final)), C.byref(v), C.byref(info))
        # (tid, pos) of the first record of the bundle that is open after the call — after TBK_E2BIG: of the one that did not fit —, or None
        self.cov_stream_first = (int(info.first_tid), int(info.first_pos)) if rc in (0, -4) and info.first_tid != -2 else None
        self._check(rc, "tbk_cov_stream_push")
        return DeviceCovView(v, int(v.n_records), int(v.n_cigar_ops)), {k: int(getattr(info, k)) for k in ("n_view", "n_carry", "n_taken", "cut")}

    def cov_stream_reset(self):
        """tbk_cov_stream_reset: forget the carried records (a new stream begins)"""
        self._check(self.L.tbk_cov_stream_reset(self.h), "tbk_cov_stream_reset")

    def bam_decode_file_spans(self, file_spans, n_ref, tbmerged=None, want_md=False, want_names=False):
        """tbk_bam_decode_file_spans: file_spans = per input file the list of its spans [(bytes of whole BGZF members, first_uoff,
        last_uoff)] (a file may have none) -> (SoaIn struct of the device-resident tile, file_off [n_files + 1]).  The arrays live in the
        context until bam_release() or the next decode."""
        k = len(file_spans)
        spans = [s for f in file_spans for s in f]
        m = len(spans)
        first = np.zeros(k + 1, dtype=np.uint32)
        first[1:] = np.cumsum([len(f) for f in file_spans])
        bufs = [np.frombuffer(z, dtype=np.uint8) for z, _, _ in spans]
        ptrs = (C.c_void_p * max(m, 1))(*[b.ctypes.data if len(b) else None for b in bufs])
        sizes = np.array([len(b) for b in bufs], dtype=np.uint64)
        fu = np.array([s[1] for s in spans], dtype=np.uint32)
        lu = np.array([s[2] for s in spans], dtype=np.uint32)
        tb = np.ascontiguousarray(tbmerged if tbmerged is not None else np.zeros(k, np.uint8), dtype=np.uint8)
        fo = np.zeros(k + 1, dtype=np.uint32)
        s = _lib.SoaIn()
        self._check(self.L.tbk_bam_decode_file_spans(self.h, k, first.ctypes.data, ptrs, sizes.ctypes.data, fu.ctypes.data, lu.ctypes.data, int(n_ref),
                                                     tb.ctypes.data, int(want_md), int(want_names), C.byref(s), fo.ctypes.data), "tbk_bam_decode_file_spans")
        self._bam_keep = (bufs, tb, fo)
        return s, fo

    def _tile_region(self, name, tile_struct, sel):
        k = int(tile_struct.n_files)
        fo = np.zeros(k + 1, dtype=np.uint32)
        out, nk = _lib.SoaIn(), C.c_uint32(0)
        self._check(getattr(self.L, name)(self.h, C.byref(tile_struct), *sel, C.byref(out), fo.ctypes.data, C.byref(nk)), name)
        assert int(nk.value) == int(out.n_records)
        self._region_keep = (fo, getattr(self, "_bam_keep", None))
        return out, fo

    def tile_region(self, tile_struct, tid, beg, end):
        """tbk_tile_region: the records of the context's decoded tile overlapping [beg, end) on tid as a collapse tile -> (SoaIn struct,
        file_off [n_files + 1]); the input tile is consumed, tile indices are the compacted ones from here on"""
        return self._tile_region("tbk_tile_region", tile_struct, (int(tid), int(beg), int(end)))

    def tile_regions(self, tile_struct, table):
        """tbk_tile_regions: the records of the context's decoded tile overlapping any interval of the table as a collapse tile -> (SoaIn
        struct, file_off [n_files + 1]); the input tile is consumed"""
        u, _keep = _regions(table)
        return self._tile_region("tbk_tile_regions", tile_struct, (C.byref(u),))

    def _cov_clip(self, name, res, sel, cap):
        """the clips of coverage() rows: own copies of the rows (the interval columns in arrays of cap elements: None for the rows' own
        count, which one region never exceeds), the call, the rows that came out"""
        keep = []
        dev = any(_is_torch(res.get(k)) for k in ("iv_tid", "j_tid"))
        a, b = (len(res["iv_tid"]) if "iv_tid" in res else 0), (len(res["j_tid"]) if "j_tid" in res else 0)
        cap = a if cap is None else cap
        own = {k: _grown(v, cap if k[:3] == "iv_" else len(v)) for k, v in res.items() if k[:3] == "iv_" or k[:2] == "j_"}

        def ptr(name, dt):
            return _addr(own[name], dt, keep) if name in own and _numel(own[name]) else None
        o = _lib.CovOut(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, cap if "iv_tid" in own else 0, ptr("iv_tid", np.int32), ptr("iv_start", np.int32),
                        ptr("iv_end", np.int32), ptr("iv_val", np.float64), b, ptr("j_tid", np.int32), ptr("j_start", np.int32), ptr("j_end", np.int32),
                        ptr("j_strand", np.uint8), ptr("j_val", np.float64), a, b, 0, 0)
        self._order_after_torch(dev)
        self._check_grow(getattr(self.L, name)(self.h, C.byref(o), *sel), name, o, own)
        out = dict(n_intervals=int(o.n_intervals), n_junctions=int(o.n_junctions))
        for k, v in own.items():
            out[k] = v[:out["n_intervals"] if k[:3] == "iv_" else out["n_junctions"]]
        return out

    def cov_clip(self, res, tid, beg, end):
        """tbk_cov_clip: the result dict of coverage() cut to [beg, end) on tid (numpy rows or device tensors), as a new dict"""
        return self._cov_clip("tbk_cov_clip", res, (int(tid), int(beg), int(end)), None)

    def cov_clip_regions(self, res, table, cap_intervals=None):
        """tbk_cov_clip_regions: the result dict of coverage() cut to the table, as a new dict.  The interval rows can grow by
        len(table) - 1: the arrays are sized cap_intervals (default: the rows + len(table)).  On TBK_E2BIG the TbkError carries
        .needed (the count the call asks for) and .rows (the arrays as the call left them)."""
        u, _keep = _regions(table)
        a = len(res["iv_tid"]) if "iv_tid" in res else 0
        return self._cov_clip("tbk_cov_clip_regions", res, (C.byref(u),), a + len(table) if cap_intervals is None else int(cap_intervals))

    def _sample_clip(self, name, res, sel, cap):
        """the clips of sample() rows (as _cov_clip)"""
        keep = []
        dev = _is_torch(res["s_tid"])
        a = len(res["s_tid"])
        cap = a if cap is None else cap
        own = {k: _grown(v, cap) for k, v in res.items() if k[:2] == "s_"}

        def ptr(name, dt):
            return _addr(own[name], dt, keep) if cap else None
        o = _lib.SampleOut(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, cap, ptr("s_tid", np.int32), ptr("s_start", np.int32), ptr("s_end", np.int32),
                           ptr("s_count", np.int64), ptr("s_heat", np.float32), a)
        self._order_after_torch(dev)
        self._check_grow(getattr(self.L, name)(self.h, C.byref(o), *sel), name, o, own)
        m = int(o.n_intervals)
        out = {k: v[:m] for k, v in own.items()}
        out["n_sample"] = m
        return out

    def sample_clip(self, res, tid, beg, end):
        """tbk_sample_clip: the result dict of sample() cut to [beg, end) on tid, as a new dict"""
        return self._sample_clip("tbk_sample_clip", res, (int(tid), int(beg), int(end)), None)

    def sample_clip_regions(self, res, table, cap_intervals=None):
        """tbk_sample_clip_regions: the result dict of sample() cut to the table, as a new dict (capacity and TBK_E2BIG as cov_clip_regions)"""
        u, _keep = _regions(table)
        return self._sample_clip("tbk_sample_clip_regions", res, (C.byref(u),), len(res["s_tid"]) + len(table) if cap_intervals is None else int(cap_intervals))

    def _check_grow(self, rc, what, o, own):
        if rc == -4:
            e = TbkError(rc, "%s: %d interval rows needed" % (what, int(o.n_intervals)))
            e.needed, e.rows = int(o.n_intervals), own
            raise e
        self._check(rc, what)

    def bam_records(self, idx):
        """tbk_bam_records: (bytes of the packed records, offsets [n+1])"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        n = len(idx)
        off = np.zeros(n + 1, dtype=np.uint64)
        out = np.empty(max(1, 512 * n), dtype=np.uint8)
        rc = self.L.tbk_bam_records(self.h, idx.ctypes.data, n, _lib.TBK_MEM_HOST, out.ctypes.data, out.size, off.ctypes.data)
        if rc == -4:
            out = np.empty(int(off[n]), dtype=np.uint8)
            rc = self.L.tbk_bam_records(self.h, idx.ctypes.data, n, _lib.TBK_MEM_HOST, out.ctypes.data, out.size, off.ctypes.data)
        self._check(rc, "tbk_bam_records")
        return out[:int(off[n])].tobytes(), off

    def bam_release(self):
        self.L.tbk_bam_release(self.h)

    def tile_join(self, dev_struct, host_tile: SoATile):
        """tbk_tile_join: the device tile of bam_decode + a host tile (plain inputs) -> (SoaIn struct of the joined device tile, file_off);
        its arrays live in the context until bam_release()"""
        keep = []
        hs, dev, _ = self._soa_struct(host_tile, keep)
        assert not dev
        k = int(dev_struct.n_files) + int(host_tile.n_files)
        fo = np.zeros(k + 1, dtype=np.uint32)
        tb = np.zeros(k, dtype=np.uint8)
        out = _lib.SoaIn()
        self._check(self.L.tbk_tile_join(self.h, C.byref(dev_struct), C.byref(hs), C.byref(out), fo.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         tb.ctypes.data_as(C.POINTER(C.c_uint8))), "tbk_tile_join")
        self._join_keep = (fo, tb)
        return out, fo

    def reserve_tile(self, n_records, n_cigar_ops):
        self._check(self.L.tbk_reserve_tile(self.h, int(n_records), int(n_cigar_ops)), "tbk_reserve_tile")

    def soa_to_numpy(self, s, fields=("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")):
        """copy arrays of a device-resident SoaIn (bam_decode) to numpy (tests)"""
        import ctypes
        torch = _torch()
        n, nc = int(s.n_records), int(s.n_cigar_ops)
        spec = {"tid": (np.int32, n), "pos": (np.int32, n), "flag": (np.uint16, n), "mapq": (np.uint8, n), "strand": (np.uint8, n),
                "nh": (np.int32, n), "cig_off": (np.uint32, n + 1), "cig": (np.uint32, nc), "yc_in": (np.float64, n), "yx_in": (np.int64, n),
                "yd_in": (np.int64, n), "md_off": (np.uint32, n + 1), "md_has": (np.uint8, n), "qname_hash": (np.uint64, n),
                "qname_off": (np.uint32, n + 1)}
        out = {}
        hip = ctypes.CDLL("libamdhip64.so")
        for name in fields:
            dt, cnt = spec[name]
            a = np.empty(cnt, dtype=dt)
            ptr = getattr(s, name)
            if cnt and ptr:
                assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), 2) == 0
            out[name] = a
        for name, offname in (("md", "md_off"), ("qname", "qname_off")):
            if offname in out and getattr(s, name):
                cnt = int(out[offname][-1])
                a = np.empty(cnt, dtype=np.uint8)
                if cnt:
                    assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(getattr(s, name)), C.c_size_t(cnt), 2) == 0
                out[name] = a
        return out

    def collapse_struct(self, s, n_files, **kw):
        """collapse a tile given as a raw SoaIn struct on the device (bam_decode); returns the usual dict (torch tensors)"""
        torch = _torch()
        o = self.make_opts(**kw)
        n = int(s.n_records)
        cap = max(n, 1)
        dev = "cuda:%d" % self.device
        rep = torch.empty(cap, dtype=torch.int32, device=dev)
        yc = torch.empty(cap, dtype=torch.float64, device=dev)
        yx = torch.empty(cap, dtype=torch.int64, device=dev)
        yd = torch.empty(cap, dtype=torch.int32, device=dev)
        gs = torch.empty(cap, dtype=torch.int32, device=dev)
        ge = torch.empty(cap, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g = _lib.GroupsOut(_lib.TBK_MEM_DEVICE, cap, rep.data_ptr(), yc.data_ptr(), yx.data_ptr(), yd.data_ptr(), gs.data_ptr(), ge.data_ptr(),
                           None, None, None, 0, 0)
        self._check(self.L.tbk_collapse_tile(self.h, C.byref(o), C.byref(s), C.byref(g)), "tbk_collapse_tile")
        m = int(g.n_groups)
        return dict(n_groups=m, n_passed=int(g.n_passed), rep=rep[:m], yc=yc[:m], yx=yx[:m], yd=yd[:m], g_start=gs[:m], g_end=ge[:m])

    # ---- multi-GPU: shuffle, then collapse (device side of tiebrush_amd.dist) -------------------
    def _dev(self):
        return "cuda:%d" % self.device

    def shard_prepare(self, tile: SoATile, out=None, **filters):
        """tbk_shard_prepare: (key, emax, effend, pass) for the device-resident tile."""
        torch = _torch()
        keep = []
        s, dev, n = self._soa_struct(tile, keep)
        assert dev, "shard_prepare needs a device-resident tile"
        bufs = out if out is not None else {}
        for name, dt in (("key", torch.int64), ("emax", torch.int64), ("effend", torch.int32), ("pass", torch.uint8)):
            if name not in bufs or bufs[name].numel() < max(n, 1):
                bufs[name] = torch.empty(max(n, 1), dtype=dt, device=self._dev())
        o = self.make_opts(**filters)
        self._order_after_torch(True)
        self._check(self.L.tbk_shard_prepare(self.h, C.byref(o), C.byref(s), C.c_void_p(bufs["key"].data_ptr()),
                                             C.c_void_p(bufs["emax"].data_ptr()), C.c_void_p(bufs["effend"].data_ptr()),
                                             C.c_void_p(bufs["pass"].data_ptr())), "tbk_shard_prepare")
        return bufs["key"][:n], bufs["emax"][:n], bufs["effend"][:n], bufs["pass"][:n]

    def shard_probe_max(self, file_off, key, emax, cuts, m_out):
        fo = np.ascontiguousarray(file_off, dtype=np.uint32)
        self._order_after_torch(True)
        self._check(self.L.tbk_shard_probe_max(self.h, fo.ctypes.data, len(fo) - 1, C.c_void_p(key.data_ptr()), C.c_void_p(emax.data_ptr()),
                                               C.c_void_p(cuts.data_ptr()), int(cuts.numel()), C.c_void_p(m_out.data_ptr())),
                    "tbk_shard_probe_max")
        return m_out

    def shard_probe_next(self, file_off, key, m, nxt_out):
        fo = np.ascontiguousarray(file_off, dtype=np.uint32)
        self._order_after_torch(True)
        self._check(self.L.tbk_shard_probe_next(self.h, fo.ctypes.data, len(fo) - 1, C.c_void_p(key.data_ptr()), C.c_void_p(m.data_ptr()),
                                                int(m.numel()), C.c_void_p(nxt_out.data_ptr())), "tbk_shard_probe_next")
        return nxt_out

    def shard_pack(self, tile: SoATile, key, passm, effend, cuts, world, out=None):
        """tbk_shard_pack: (rows [n, 6] int32 — the first sum(tab[..., 1]) are filled —, cig words, src_idx [n] int64,
        tab [world, n_files, 5] int64)."""
        torch = _torch()
        keep = []
        s, dev, n = self._soa_struct(tile, keep)
        bufs = out if out is not None else {}
        nc = _numel(tile.cig)
        n_pass = n                                   # upper bound; the table tells how many rows were written
        if "rows" not in bufs or bufs["rows"].shape[0] < max(n_pass, 1):
            bufs["rows"] = torch.empty((max(n_pass, 1), 6), dtype=torch.int32, device=self._dev())
        if "cig" not in bufs or bufs["cig"].numel() < max(nc, 1):
            bufs["cig"] = torch.empty(max(nc, 1), dtype=torch.int32, device=self._dev())
        if "src" not in bufs or bufs["src"].numel() < max(n_pass, 1):
            bufs["src"] = torch.empty(max(n_pass, 1), dtype=torch.int64, device=self._dev())
        tab = torch.empty((world, tile.n_files, 5), dtype=torch.int64, device=self._dev())
        self._order_after_torch(True)
        self._check(self.L.tbk_shard_pack(self.h, C.byref(s), C.c_void_p(key.data_ptr()), C.c_void_p(passm.data_ptr()),
                                          C.c_void_p(effend.data_ptr()), C.c_void_p(cuts.data_ptr()) if world > 1 else None, int(world),
                                          C.c_void_p(bufs["rows"].data_ptr()), C.c_void_p(bufs["cig"].data_ptr()),
                                          C.c_void_p(bufs["src"].data_ptr()), C.c_void_p(tab.data_ptr())), "tbk_shard_pack")
        return bufs["rows"][:n_pass], bufs["cig"], bufs["src"][:n_pass], tab

    def shard_unpack(self, rows, file_off2, out=None):
        """tbk_shard_unpack: the SoA arrays (torch tensors) of the received rows; file_off2 = run boundaries (host)."""
        torch = _torch()
        n2 = int(rows.shape[0])
        fo = np.ascontiguousarray(file_off2, dtype=np.uint32)
        bufs = out if out is not None else {}
        spec = (("tid", torch.int32, n2), ("pos", torch.int32, n2), ("flag", torch.int16, n2), ("mapq", torch.uint8, n2),
                ("strand", torch.uint8, n2), ("nh", torch.int32, n2), ("cig_off", torch.int32, n2 + 1), ("prio_hi", torch.int64, n2),
                ("prio_lo", torch.int64, n2))
        for name, dt, cnt in spec:
            if name not in bufs or bufs[name].numel() < max(cnt, 1):
                bufs[name] = torch.empty(max(cnt, 1), dtype=dt, device=self._dev())
        self._order_after_torch(True)
        rows = rows.contiguous()
        self._check(self.L.tbk_shard_unpack(self.h, C.c_void_p(rows.data_ptr()) if n2 else None, n2, fo.ctypes.data, len(fo) - 1,
                                            *[C.c_void_p(bufs[name].data_ptr()) for name, _, _ in spec]), "tbk_shard_unpack")
        return {name: bufs[name][:cnt] for name, _, cnt in spec}

    # ---- multi-GPU: collapse locally, exchange group partials (device side of tiebrush_amd.dist.partials_collapse) ------
    def partial_keys(self, tile: SoATile, fin, out=None):
        """tbk_partial_keys: (key [ng], emax [ng], not_packable) of the local groups in `fin` (a collapse() result with
        want_coords=True)."""
        torch = _torch()
        ng = int(fin["n_groups"])
        bufs = out if out is not None else {}
        for name in ("pkey", "pemax"):
            if name not in bufs or bufs[name].numel() < max(ng, 1):
                bufs[name] = torch.empty(max(ng, 1), dtype=torch.int64, device=self._dev())
        bad = C.c_uint32(0)
        self._order_after_torch(True)
        self._check(self.L.tbk_partial_keys(self.h, C.byref(fin["_soa"]), C.byref(fin["_struct"]), C.c_void_p(bufs["pkey"].data_ptr()),
                                            C.c_void_p(bufs["pemax"].data_ptr()), C.byref(bad)), "tbk_partial_keys")
        return bufs["pkey"][:ng], bufs["pemax"][:ng], int(bad.value)

    def partial_pack(self, tile: SoATile, fin, key, cuts, world, first_fidx, out=None, opts=None, **kw):
        """tbk_partial_pack: (rows [ng, 12] int32, cig words, tab [world, 3] int64) of the local groups (fin needs want_effend=True
        and a final yd; opts / kw = the options the groups were collapsed with)."""
        torch = _torch()
        o = opts if opts is not None else self.make_opts(**kw)
        ng = int(fin["n_groups"])
        nc = _numel(tile.cig)
        bufs = out if out is not None else {}
        if "prows" not in bufs or bufs["prows"].shape[0] < max(ng, 1):
            bufs["prows"] = torch.empty((max(ng, 1), 12), dtype=torch.int32, device=self._dev())
        if "pcig" not in bufs or bufs["pcig"].numel() < max(nc, 1):
            bufs["pcig"] = torch.empty(max(nc, 1), dtype=torch.int32, device=self._dev())
        tab = torch.empty((world, 3), dtype=torch.int64, device=self._dev())
        self._order_after_torch(True)
        self._check(self.L.tbk_partial_pack(self.h, C.byref(o), C.byref(fin["_soa"]), C.byref(fin["_struct"]), C.c_void_p(key.data_ptr()) if ng else None,
                                            C.c_void_p(cuts.data_ptr()) if world > 1 else None, int(world), int(first_fidx),
                                            C.c_void_p(bufs["prows"].data_ptr()), C.c_void_p(bufs["pcig"].data_ptr()),
                                            C.c_void_p(tab.data_ptr())), "tbk_partial_pack")
        return bufs["prows"][:ng], bufs["pcig"], tab

    # ---- the sender's side without a wait (tbk_partial_stage_*): every call only queues kernels, on torch's current stream, so that
    # the collectives between the stages are ordered with them by the stream alone
    @contextlib.contextmanager
    def _queued_on_torch_stream(self):
        torch = _torch()
        was = self._on_torch_stream
        if not was:
            sp = torch.cuda.current_stream(self.device).cuda_stream
            self.L.tbk_set_stream(self.h, C.c_void_p(sp if sp else 1))      # (0 = the default stream: TBK_STREAM_DEFAULT)
            self._on_torch_stream = True
        try:
            yield
        finally:
            if not was:
                self.L.tbk_set_stream(self.h, None)
                self._on_torch_stream = False

    def partial_stage_keys(self, tile: SoATile, fin, first_fidx, carry=0, out=None):
        """tbk_partial_stage_keys: (key, emax, meta [PARTIAL_META] int64) — device tensors, nothing read back"""
        torch = _torch()
        ng = int(fin["n_groups"])
        bufs = out if out is not None else {}
        for name in ("pkey", "pemax"):
            if name not in bufs or bufs[name].numel() < max(ng, 1):
                bufs[name] = torch.empty(max(ng, 1), dtype=torch.int64, device=self._dev())
        meta = torch.empty(_lib.PARTIAL_META, dtype=torch.int64, device=self._dev())
        with self._queued_on_torch_stream():
            self._check(self.L.tbk_partial_stage_keys(self.h, C.byref(fin["_soa"]), C.byref(fin["_struct"]), C.c_void_p(bufs["pkey"].data_ptr()),
                                                      C.c_void_p(bufs["pemax"].data_ptr()), int(first_fidx), int(carry), C.c_void_p(meta.data_ptr())),
                        "tbk_partial_stage_keys")
        return bufs["pkey"][:ng], bufs["pemax"][:ng], meta

    def partial_stage_cands(self, key, emax, allmeta, world):
        """tbk_partial_stage_cands: (targets [world - 1], cands [world - 1, PARTIAL_CAND]) from the gathered meta rows"""
        torch = _torch()
        nc = max(world - 1, 1)
        targets = torch.empty(nc, dtype=torch.int64, device=self._dev())
        cands = torch.empty((nc, _lib.PARTIAL_CAND), dtype=torch.int64, device=self._dev())
        ng = int(key.numel())
        allmeta = allmeta.contiguous()
        with self._queued_on_torch_stream():
            self._check(self.L.tbk_partial_stage_cands(self.h, C.c_void_p(key.data_ptr()) if ng else None, C.c_void_p(emax.data_ptr()) if ng else None, ng,
                                                       C.c_void_p(allmeta.data_ptr()), int(world), C.c_void_p(targets.data_ptr()), C.c_void_p(cands.data_ptr())),
                        "tbk_partial_stage_cands")
        return targets, cands

    def partial_stage_pack(self, tile: SoATile, fin, key, meta, allcands, targets, world, first_fidx, out=None, opts=None, **kw):
        """tbk_partial_stage_pack: (rows [ng, 12] int32, cig words, tabx [world * 3 + 4] int64, cuts [world - 1]) — all on the device"""
        torch = _torch()
        o = opts if opts is not None else self.make_opts(**kw)
        ng = int(fin["n_groups"])
        nc = _numel(tile.cig)
        bufs = out if out is not None else {}
        if "prows" not in bufs or bufs["prows"].shape[0] < max(ng, 1):
            bufs["prows"] = torch.empty((max(ng, 1), 12), dtype=torch.int32, device=self._dev())
        if "pcig" not in bufs or bufs["pcig"].numel() < max(nc, 1):
            bufs["pcig"] = torch.empty(max(nc, 1), dtype=torch.int32, device=self._dev())
        tabx = torch.empty(world * 3 + 4, dtype=torch.int64, device=self._dev())
        cuts = torch.empty(max(world - 1, 1), dtype=torch.int64, device=self._dev())
        allcands = allcands.contiguous() if allcands is not None else None
        with self._queued_on_torch_stream():
            self._check(self.L.tbk_partial_stage_pack(self.h, C.byref(o), C.byref(fin["_soa"]), C.byref(fin["_struct"]), C.c_void_p(key.data_ptr()) if ng else None,
                                                      C.c_void_p(meta.data_ptr()), C.c_void_p(allcands.data_ptr()) if world > 1 else None,
                                                      C.c_void_p(targets.data_ptr()) if world > 1 else None, int(world), int(first_fidx),
                                                      C.c_void_p(cuts.data_ptr()), C.c_void_p(bufs["prows"].data_ptr()), C.c_void_p(bufs["pcig"].data_ptr()),
                                                      C.c_void_p(tabx.data_ptr())), "tbk_partial_stage_pack")
        return bufs["prows"][:ng], bufs["pcig"], tabx, cuts[:max(world - 1, 0)]

    def partial_unpack(self, rows, out=None):
        """tbk_partial_unpack: the SoA arrays (torch tensors) of the received partial rows."""
        torch = _torch()
        n2 = int(rows.shape[0])
        bufs = out if out is not None else {}
        spec = (("tid", torch.int32, n2), ("pos", torch.int32, n2), ("flag", torch.int16, n2), ("mapq", torch.uint8, n2),
                ("strand", torch.uint8, n2), ("nh", torch.int32, n2), ("cig_off", torch.int32, n2 + 1), ("yc_in", torch.float64, n2),
                ("yx_in", torch.int64, n2), ("yd_in", torch.int64, n2), ("prio_hi", torch.int64, n2), ("prio_lo", torch.int64, n2))
        for name, dt, cnt in spec:
            if name not in bufs or bufs[name].numel() < max(cnt, 1):
                bufs[name] = torch.empty(max(cnt, 1), dtype=dt, device=self._dev())
        self._order_after_torch(True)
        rows = rows.contiguous()
        self._check(self.L.tbk_partial_unpack(self.h, C.c_void_p(rows.data_ptr()) if n2 else None, n2,
                                              *[C.c_void_p(bufs[name].data_ptr()) for name, _, _ in spec]), "tbk_partial_unpack")
        return {name: bufs[name][:cnt] for name, _, cnt in spec}

    def partial_pack_md(self, tile: SoATile, fin, tab, world, rows):
        """tbk_partial_pack_md (-L): (MD bytes of the local groups' representatives in group order [uint8], bytes per destination [world]
        int64) — device tensors; the rows' word 11 is written.  tab: the [world, 3] table of the pack (tabx starts with it)."""
        torch = _torch()
        ng = int(fin["n_groups"])
        nmd = _numel(tile.md)
        md_out = torch.empty(max(nmd, 1), dtype=torch.uint8, device=self._dev())
        md_tab = torch.empty(world, dtype=torch.int64, device=self._dev())
        with self._queued_on_torch_stream():
            self._check(self.L.tbk_partial_pack_md(self.h, C.byref(fin["_soa"]), C.byref(fin["_struct"]), C.c_void_p(tab.data_ptr()), int(world),
                                                   C.c_void_p(rows.data_ptr()) if ng else None, C.c_void_p(md_out.data_ptr()), C.c_void_p(md_tab.data_ptr())),
                        "tbk_partial_pack_md")
        return md_out, md_tab

    def partial_unpack_md(self, rows):
        """tbk_partial_unpack_md: (md_off [n2 + 1] uint32 as int32 tensor, md_has [n2] uint8) of received rows"""
        torch = _torch()
        n2 = int(rows.shape[0])
        md_off = torch.empty(n2 + 1, dtype=torch.int32, device=self._dev())
        md_has = torch.empty(max(n2, 1), dtype=torch.uint8, device=self._dev())
        self._order_after_torch(True)
        rows = rows.contiguous()
        self._check(self.L.tbk_partial_unpack_md(self.h, C.c_void_p(rows.data_ptr()) if n2 else None, n2, C.c_void_p(md_off.data_ptr()),
                                                 C.c_void_p(md_has.data_ptr())), "tbk_partial_unpack_md")
        return md_off, md_has[:n2]

    def partial_reduce(self, rows, run_off, cig, out=None, want_view=True, opts=None, md=None, **kw):
        """tbk_partial_reduce: the owner's merge-reduce of the received partial rows (torch int32 [n2, 12]; run_off = host run
        boundaries [R + 1]; cig = the CIGAR words as received).  Returns the usual collapse dict (rep = ROW index of the
        representative) plus "view" (DeviceCovView of the reduced groups, valid until the next call)."""
        torch = _torch()
        o = opts if opts is not None else self.make_opts(**kw)
        n2 = int(rows.shape[0])
        ro = np.ascontiguousarray(run_off, dtype=np.uint32)
        bufs = out if out is not None else {}
        cap = max(n2, 1)
        spec = (("rep", torch.int32), ("yc", torch.float64), ("yx", torch.int64), ("yd", torch.int32), ("g_start", torch.int32),
                ("g_end", torch.int32))
        for name, dt in spec:
            if name not in bufs or bufs[name].numel() < cap:
                bufs[name] = torch.empty(cap, dtype=dt, device=self._dev())
        rows = rows.contiguous()
        g = _lib.GroupsOut(_lib.TBK_MEM_DEVICE, cap, *[bufs[name].data_ptr() for name, _ in spec], None, None, None, 0, 0)
        v = _lib.CovIn()
        self._order_after_torch(True)
        self._check(self.L.tbk_partial_reduce_md(self.h, C.byref(o), C.c_void_p(rows.data_ptr()) if n2 else None, n2, ro.ctypes.data, len(ro) - 1,
                                                 C.c_void_p(cig.data_ptr()) if cig is not None and cig.numel() else None,
                                                 C.c_void_p(md.data_ptr()) if md is not None and md.numel() else None, C.byref(g),
                                                 C.byref(v) if want_view else None), "tbk_partial_reduce")
        m = int(g.n_groups)
        res = dict(n_groups=m, n_passed=n2, _bufs=bufs, _struct=g, _keep=[rows, cig, ro, md])
        res.update({name: bufs[name][:m] for name, _ in spec})
        if want_view:
            res["view"] = DeviceCovView(v, int(v.n_records), int(v.n_cigar_ops))
        return res

    # ---- coverage -----------------------------------------------------------------------------
    def coverage(self, cin, want_cov=True, want_junc=True, cap_intervals=None, cap_junctions=None, out=None, raw=False):
        keep = []
        if isinstance(cin, DeviceCovView):
            s = cin.struct
            dev, n, nc = True, cin.n_records, cin.n_cigar_ops
        else:
            dev = _is_torch(cin.tid)
            n = _numel(cin.tid)
            nc = _numel(cin.cig)
            s = _lib.CovIn(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, n, nc, _addr(cin.tid, np.int32, keep, n),
                           _addr(cin.pos, np.int32, keep, n), _addr(cin.flag, np.uint16, keep, n),
                           _addr(cin.cig_off, np.uint32, keep, n + 1), _addr(cin.cig, np.uint32, keep, nc),
                           _addr(cin.yc, np.float64, keep, n), _addr(cin.strand, np.uint8, keep, n), None)
        self._order_after_torch(dev)
        ci = (cap_intervals if cap_intervals is not None else 2 * nc + 2 * n + 16) if want_cov else 0
        cj = (cap_junctions if cap_junctions is not None else nc + 16) if want_junc else 0
        bufs = out if out is not None else {}

        def buf(name, count, dt):
            if count == 0:
                return None
            if name not in bufs or _numel(bufs[name]) < count:
                bufs[name] = self._alloc(dev, count, dt)
            return bufs[name]

        iv = [buf("iv_tid", ci, np.int32), buf("iv_start", ci, np.int32), buf("iv_end", ci, np.int32),
              buf("iv_val", ci, np.float64)]
        jv = [buf("j_tid", cj, np.int32), buf("j_start", cj, np.int32), buf("j_end", cj, np.int32),
              buf("j_strand", cj, np.uint8), buf("j_val", cj, np.float64)]
        o = _lib.CovOut(s.mem, ci, _addr(iv[0], np.int32, keep), _addr(iv[1], np.int32, keep),
                        _addr(iv[2], np.int32, keep), _addr(iv[3], np.float64, keep), cj, _addr(jv[0], np.int32, keep),
                        _addr(jv[1], np.int32, keep), _addr(jv[2], np.int32, keep), _addr(jv[3], np.uint8, keep),
                        _addr(jv[4], np.float64, keep), 0, 0, 0, 0)
        self._check(self.L.tbk_coverage_tile(self.h, C.byref(s), C.byref(o)), "tbk_coverage_tile")
        a, b = int(o.n_intervals), int(o.n_junctions)
        res = dict(n_intervals=a, n_junctions=b, n_bases=int(o.n_bases), span_bases=int(o.span_bases), _bufs=bufs)
        if raw:
            return res
        if want_cov:
            res.update(iv_tid=iv[0][:a], iv_start=iv[1][:a], iv_end=iv[2][:a], iv_val=iv[3][:a])
        if want_junc:
            res.update(j_tid=jv[0][:b], j_start=jv[1][:b], j_end=jv[2][:b], j_strand=jv[3][:b], j_val=jv[4][:b])
        return res

    def cov_split_strand(self, cin):
        """tbk_cov_split_strand: a CovInput (numpy arrays: uploaded by the call; or device tensors) or a DeviceCovView divided by splice
        strand -> [view of '+', view of '-', view of every other strand byte], each a DeviceCovView in the input's order without the
        unmapped records (flag 0x4), in memory of the context's own: valid until the next cov_split_strand, through coverage(), sample(),
        the clips and the track writers."""
        keep = []
        if isinstance(cin, DeviceCovView):
            s, dev = cin.struct, True
        else:
            dev = _is_torch(cin.tid)
            n = _numel(cin.tid)
            nc = _numel(cin.cig)
            s = _lib.CovIn(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, n, nc, _addr(cin.tid, np.int32, keep, n),
                           _addr(cin.pos, np.int32, keep, n), _addr(cin.flag, np.uint16, keep, n),
                           _addr(cin.cig_off, np.uint32, keep, n + 1), _addr(cin.cig, np.uint32, keep, nc),
                           _addr(cin.yc, np.float64, keep, n), _addr(cin.strand, np.uint8, keep, n), _addr(cin.yx, np.int64, keep, n))
        self._order_after_torch(dev)
        v = (_lib.CovIn * 3)()
        self._check(self.L.tbk_cov_split_strand(self.h, C.byref(s), v), "tbk_cov_split_strand")
        return [DeviceCovView(v[k], int(v[k].n_records), int(v[k].n_cigar_ops)) for k in range(3)]

    def cov_summary(self, rows, features):
        """tbk_cov_summary: the result dict of coverage() (numpy rows or device tensors; a dict without iv_* / j_* rows leaves those
        columns out) read against features: [(tid, beg, end)] or [(tid, beg, end, strand)] with strand one of '+', '-', '.', or a dict
        of arrays tid / beg / end (/ strand).  Returns numpy arrays, one element per feature: covered (uint64), sum, max, junc."""
        keep = []
        if isinstance(features, dict):
            ft, fb, fe = (np.ascontiguousarray(features[k], dtype=d) for k, d in (("tid", np.int32), ("beg", np.int64), ("end", np.int64)))
            fs = np.ascontiguousarray(features["strand"], dtype=np.uint8) if features.get("strand") is not None else None
        else:
            fl = [tuple(f) for f in features]
            ft = np.array([f[0] for f in fl], dtype=np.int32)
            fb = np.array([f[1] for f in fl], dtype=np.int64)
            fe = np.array([f[2] for f in fl], dtype=np.int64)
            fs = None
            if any(len(f) > 3 for f in fl):
                fs = np.array([(f[3] if isinstance(f[3], int) else ord(f[3])) if len(f) > 3 else ord(".") for f in fl], dtype=np.uint8)
        n = len(ft)
        want_cov, want_junc = "iv_tid" in rows, "j_tid" in rows
        dev = any(_is_torch(rows.get(k)) for k in ("iv_tid", "j_tid"))
        a, b = (len(rows["iv_tid"]) if want_cov else 0), (len(rows["j_tid"]) if want_junc else 0)

        def ptr(name, dt, cnt):
            return _addr(rows[name], dt, keep, cnt) if cnt else None
        # (a capacity of zero says "not computed": rows of a wanted but empty track keep a capacity of one)
        o = _lib.CovOut(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, max(a, 1) if want_cov else 0, ptr("iv_tid", np.int32, a), ptr("iv_start", np.int32, a),
                        ptr("iv_end", np.int32, a), ptr("iv_val", np.float64, a), max(b, 1) if want_junc else 0, ptr("j_tid", np.int32, b),
                        ptr("j_start", np.int32, b), ptr("j_end", np.int32, b), ptr("j_strand", np.uint8, b), ptr("j_val", np.float64, b), a, b, 0, 0)
        f = _lib.Features(n, ft.ctypes.data, fb.ctypes.data, fe.ctypes.data, fs.ctypes.data if fs is not None else None)
        res = dict(covered=np.zeros(n, dtype=np.uint64), sum=np.zeros(n), max=np.zeros(n), junc=np.zeros(n))
        fo = _lib.FeatOut(_lib.TBK_MEM_HOST, *(res[k].ctypes.data if n else None for k in ("covered", "sum", "max", "junc")))
        self._order_after_torch(dev)
        self._check(self.L.tbk_cov_summary(self.h, C.byref(o), C.byref(f), C.byref(fo)), "tbk_cov_summary")
        if not want_cov:
            del res["covered"], res["sum"], res["max"]
        if not want_junc:
            del res["junc"]
        return res

    def cov_thresholds(self, rows, features, thr, out=None):
        """tbk_cov_thresholds: the interval rows of coverage()'s result dict (numpy rows or device tensors) read against features (as
        cov_summary takes them; strands are ignored) and 1 to 16 strictly ascending thresholds > 0.  Returns covered [n] and ge
        [n, len(thr)] — the bases of the feature under a row, and under a row with value >= thr[k] — as uint64 numpy arrays for numpy
        rows, as int64 tensors on the rows' device for device rows (the library writes them there); out="host" / "device" says where
        they go whatever the rows are."""
        keep = []
        if isinstance(features, dict):
            ft, fb, fe = (np.ascontiguousarray(features[k], dtype=d) for k, d in (("tid", np.int32), ("beg", np.int64), ("end", np.int64)))
        else:
            fl = [tuple(f) for f in features]
            ft = np.array([f[0] for f in fl], dtype=np.int32)
            fb = np.array([f[1] for f in fl], dtype=np.int64)
            fe = np.array([f[2] for f in fl], dtype=np.int64)
        n = len(ft)
        t = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
        nt = len(t)
        dev = _is_torch(rows.get("iv_tid"))
        a = len(rows["iv_tid"]) if "iv_tid" in rows else 0

        def ptr(name, dt):
            return _addr(rows[name], dt, keep, a) if a else None
        o = _lib.CovOut(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, max(a, 1), ptr("iv_tid", np.int32), ptr("iv_start", np.int32), ptr("iv_end", np.int32),
                        ptr("iv_val", np.float64), 0, None, None, None, None, None, a, 0, 0, 0)
        f = _lib.Features(n, ft.ctypes.data, fb.ctypes.data, fe.ctypes.data, None)
        dev_out = dev if out is None else out == "device"
        if dev_out:
            import torch
            device = rows["iv_tid"].device if dev else "cuda:%d" % self.device
            res = dict(covered=torch.zeros(max(n, 1), dtype=torch.int64, device=device)[:n], ge=torch.zeros((max(n, 1), max(nt, 1)), dtype=torch.int64, device=device))
            fo = _lib.ThrOut(_lib.TBK_MEM_DEVICE, res["covered"].data_ptr(), res["ge"].data_ptr())
        else:
            res = dict(covered=np.zeros(n, dtype=np.uint64), ge=np.zeros((n, nt), dtype=np.uint64))
            fo = _lib.ThrOut(_lib.TBK_MEM_HOST, res["covered"].ctypes.data if n else None, res["ge"].ctypes.data if n and nt else None)
        self._order_after_torch(dev or dev_out)
        self._check(self.L.tbk_cov_thresholds(self.h, C.byref(o), C.byref(f), t.ctypes.data if nt else None, nt, C.byref(fo)), "tbk_cov_thresholds")
        if dev_out:
            res["ge"] = res["ge"][:n, :nt]
        return res

    def tx_summary(self, rows, tx, parts=False):
        """tbk_tx_summary: the result dict of coverage() (numpy rows or device tensors; a dict without iv_* / j_* rows leaves those
        columns out) read against transcripts: a dict of arrays tx_off [n_tx + 1] (CSR into the exons), tid [n_tx], ex_beg / ex_end
        [n_exon] and optionally strand [n_tx] ('+', '-', '.'), as transcripts_from_gtf returns it.  Returns numpy arrays, one element
        per transcript: covered (uint64), sum, max, exons_hit (uint32), introns_hit (uint32), junc_min, junc_sum.  parts=True adds the
        per-exon ex_covered, ex_sum, ex_max and in_junc (the intron behind the exon; 0 for a transcript's last); a tuple of those
        names asks for just them."""
        keep = []
        off = np.ascontiguousarray(tx["tx_off"], dtype=np.uint32)
        tt = np.ascontiguousarray(tx["tid"], dtype=np.int32)
        eb, ee = np.ascontiguousarray(tx["ex_beg"], dtype=np.int64), np.ascontiguousarray(tx["ex_end"], dtype=np.int64)
        ts = np.ascontiguousarray(tx["strand"], dtype=np.uint8) if tx.get("strand") is not None else None
        n_tx, n_ex = len(tt), len(eb)
        want_cov, want_junc = "iv_tid" in rows, "j_tid" in rows
        dev = any(_is_torch(rows.get(k)) for k in ("iv_tid", "j_tid"))
        a, b = (len(rows["iv_tid"]) if want_cov else 0), (len(rows["j_tid"]) if want_junc else 0)

        def ptr(name, dt, cnt):
            return _addr(rows[name], dt, keep, cnt) if cnt else None
        # (a capacity of zero says "not computed": rows of a wanted but empty track keep a capacity of one)
        o = _lib.CovOut(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, max(a, 1) if want_cov else 0, ptr("iv_tid", np.int32, a), ptr("iv_start", np.int32, a),
                        ptr("iv_end", np.int32, a), ptr("iv_val", np.float64, a), max(b, 1) if want_junc else 0, ptr("j_tid", np.int32, b),
                        ptr("j_start", np.int32, b), ptr("j_end", np.int32, b), ptr("j_strand", np.uint8, b), ptr("j_val", np.float64, b), a, b, 0, 0)
        x = _lib.Transcripts(n_tx, n_ex, off.ctypes.data if len(off) else None, tt.ctypes.data if n_tx else None, ts.ctypes.data if ts is not None else None,
                             eb.ctypes.data if n_ex else None, ee.ctypes.data if n_ex else None)
        cov_cols, junc_cols = ("covered", "sum", "max", "exons_hit"), ("introns_hit", "junc_min", "junc_sum")
        ex_cols = ("ex_covered", "ex_sum", "ex_max", "in_junc")
        asked = ex_cols if parts is True else tuple(parts or ())
        dts = dict(covered=np.uint64, exons_hit=np.uint32, introns_hit=np.uint32, ex_covered=np.uint64)
        res = {k: np.zeros(n_tx, dtype=dts.get(k, np.float64)) for k in cov_cols + junc_cols}
        res.update({k: np.zeros(n_ex, dtype=dts.get(k, np.float64)) for k in asked})
        xo = _lib.TxOut(_lib.TBK_MEM_HOST, *((res[k].ctypes.data if k in res and len(res[k]) else None) for k in cov_cols + junc_cols + ex_cols))
        self._order_after_torch(dev)
        self._check(self.L.tbk_tx_summary(self.h, C.byref(o), C.byref(x), C.byref(xo)), "tbk_tx_summary")
        for k in (() if want_cov else cov_cols + ex_cols[:3]) + (() if want_junc else junc_cols + ex_cols[3:]):
            res.pop(k, None)
        return res

    def sample(self, cin: CovInput, num_samples: int, cap_intervals=None):
        keep = []
        if isinstance(cin, DeviceCovView):                      # (region_view / groups_to_cov_in: the view carries yx)
            s, dev = cin.struct, True
            if cap_intervals is None:
                cap_intervals = 2 * cin.n_cigar_ops + 2 * cin.n_records + 16
        else:
            dev = _is_torch(cin.tid)
            n = _numel(cin.tid)
            nc = _numel(cin.cig)
            s = _lib.CovIn(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, n, nc, _addr(cin.tid, np.int32, keep, n),
                           _addr(cin.pos, np.int32, keep, n), _addr(cin.flag, np.uint16, keep, n),
                           _addr(cin.cig_off, np.uint32, keep, n + 1), _addr(cin.cig, np.uint32, keep, nc), None, None,
                           _addr(cin.yx, np.int64, keep, n))
        if cap_intervals is None:
            if dev:
                raise ValueError("cap_intervals is required for device inputs")
            c = np.asarray(cin.cig)
            cap_intervals = int((c >> 4)[(c & 0xF) == 0].sum()) + 16
        ci = cap_intervals
        iv = [self._alloc(dev, ci, np.int32) for _ in range(3)] + [self._alloc(dev, ci, np.int64),
                                                                    self._alloc(dev, ci, np.float32)]
        o = _lib.SampleOut(s.mem, ci, _addr(iv[0], np.int32, keep), _addr(iv[1], np.int32, keep),
                           _addr(iv[2], np.int32, keep), _addr(iv[3], np.int64, keep), _addr(iv[4], np.float32, keep), 0)
        self._check(self.L.tbk_sample_tile(self.h, C.byref(s), int(num_samples), C.byref(o)), "tbk_sample_tile")
        a = int(o.n_intervals)
        return dict(n_sample=a, s_tid=iv[0][:a], s_start=iv[1][:a], s_end=iv[2][:a], s_count=iv[3][:a], s_heat=iv[4][:a])

    # ---- track text -----------------------------------------------------------------------------
    def track_names(self, names):
        """The reference names (str or bytes, any length) that tid indexes in format_track's rows."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        off = np.zeros(len(raw) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in raw], dtype=np.uint64)
        blob = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
        self._check(self.L.tbk_track_names(self.h, len(raw), off.ctypes.data, blob.ctypes.data), "tbk_track_names")

    def format_track(self, kind, tid, start, end, val=None, strand=None, count=None, heat=None, first_junc=1):
        """The bytes of one track as tiecov prints it (kind: "cov", "junc" or "sample"), formatted on the device from numpy rows or
        device tensors; names from track_names().  Raises TbkError(TBK_EUNSUPPORTED) for a value outside the exact range."""
        keep = []
        dev = _is_torch(tid)
        n = _numel(tid)
        s = _lib.TrackRows(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, _lib.TRACK[kind], n, 0, _addr(tid, np.int32, keep, n),
                           _addr(start, np.int32, keep, n), _addr(end, np.int32, keep, n), _addr(val, np.float64, keep, n),
                           _addr(strand, np.uint8, keep, n), _addr(count, np.int64, keep, n), _addr(heat, np.float32, keep, n), int(first_junc))
        self._order_after_torch(dev)
        parts = []

        def sink(_user, p, nb):
            parts.append(C.string_at(p, nb))
            return 0

        cb = _lib.TRACK_SINK(sink)
        total = C.c_uint64(0)
        self._check(self.L.tbk_format_track(self.h, C.byref(s), cb, None, C.byref(total)), "tbk_format_track")
        text = b"".join(parts)
        assert len(text) == total.value
        return text

    def track_bgzf(self, kind, tid, start, end, val=None, strand=None, count=None, heat=None, first_junc=1, head=b"", ref_len=None, csi_depth=None, on_run=None):
        """tbk_track_bgzf: format_track's rows as a list of (run of whole BGZF members, index part) — the text is formatted, deflated and
        indexed on the device, slice by slice; `head` goes before row 0.  The part is a dict as bam_encode_indexed
        returns it (chunks, lin, lin_first, refs; virtual offsets relative to the run's first byte), or None when ref_len is None
        (the rows are only compressed).  csi_depth as there.  on_run(run, part): called from the sink; a true return stops the call
        (TBK_EINVAL).  A TbkError carries .n_runs, the runs the sink had taken.  The last call's text and run sizes are left in
        self.last_track_bytes."""
        if csi_depth is not None and not 0 <= int(csi_depth) < 2 ** 32 - 1:
            raise ValueError("csi_depth must be None or a non-negative integer")
        keep = []
        dev = _is_torch(tid)
        n = _numel(tid)
        s = _lib.TrackRows(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, _lib.TRACK[kind], n, 0, _addr(tid, np.int32, keep, n),
                           _addr(start, np.int32, keep, n), _addr(end, np.int32, keep, n), _addr(val, np.float64, keep, n),
                           _addr(strand, np.uint8, keep, n), _addr(count, np.int64, keep, n), _addr(heat, np.float32, keep, n), int(first_junc))
        self._order_after_torch(dev)
        io = None
        if ref_len is not None:
            ref_len = np.ascontiguousarray(ref_len, dtype=np.uint32)
            io = _lib.IxOpts()
            io.n_ref, io.reserved, io.ref_len, io.rec_vbeg = len(ref_len), 0 if csi_depth is None else int(csi_depth) + 1, ref_len.ctypes.data, None
        chunk_dt = np.dtype([("tid", "<i4"), ("bin", "<u4"), ("beg", "<u8"), ("end", "<u8")])
        ref_dt = np.dtype([("tid", "<i4"), ("reserved", "<u4"), ("n_records", "<u8"), ("first", "<u8"), ("last", "<u8")])
        runs = []

        def arr(ptr, count, dt):  # (the run and its part are valid only during the sink call: copied out here)
            if not count:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dt).itemsize), dtype=dt).copy()

        def sink(_user, p, nb, part):
            d = None
            if part:
                q = part.contents
                d = {"chunks": arr(q.chunks, q.n_chunks, chunk_dt), "lin": arr(q.lin, q.n_lin, np.dtype("<u8")), "lin_first": int(q.lin_first),
                     "refs": arr(q.refs, q.n_refs, ref_dt)}
            runs.append((C.string_at(p, nb), d))
            return 1 if on_run is not None and on_run(*runs[-1]) else 0

        cb = _lib.TBX_SINK(sink)
        head = bytes(head)
        text, out = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.tbk_track_bgzf(self.h, C.byref(s), head if head else None, len(head), C.byref(io) if io is not None else None, cb, None,
                                   C.byref(text), C.byref(out))
        try:
            self._check(rc, "tbk_track_bgzf")
        except TbkError as e:
            e.n_runs = len(runs)
            raise
        del keep
        assert sum(len(r) for r, _ in runs) == out.value
        self.last_track_bytes = (int(text.value), int(out.value))
        return runs

    def zlib_deflate(self, payload, cuts=None, out_cap=None):
        """tbk_zlib_deflate: a byte run (bytes, or a uint8 device tensor) -> the list of its pieces' zlib streams; cuts = payload
        offsets of the piece boundaries ([0, ..., len(payload)]), default one piece per 0xff00 bytes.  out_cap: the room offered for
        the streams (default: enough); when they do not fit, TbkError(TBK_E2BIG) with .needed (bytes) and .sizes (per stream)."""
        keep = []
        dev = _is_torch(payload)
        n = _numel(payload) if dev else len(payload)
        src = _addr(payload, np.uint8, keep, n) if dev else np.frombuffer(payload, dtype=np.uint8)
        cp, nm = None, 0
        if cuts is not None:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            cp, nm = cuts.ctypes.data, len(cuts) - 1
        pieces = nm if cuts is not None else (n + 0xff00 - 1) // 0xff00
        sizes = np.zeros(max(pieces, 1), dtype=np.uint32)
        cap = int(out_cap) if out_cap is not None else n + pieces * 64 + 4096
        out = np.empty(max(cap, 1), dtype=np.uint8)
        need = C.c_uint64(0)
        self._order_after_torch(dev)
        sp = src if dev else (src.ctypes.data if n else None)
        rc = self.L.tbk_zlib_deflate(self.h, sp, n, _lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, cp, nm, out.ctypes.data, cap, C.byref(need),
                                     sizes.ctypes.data)
        if rc == -4:
            e = TbkError(rc, "tbk_zlib_deflate: %d bytes needed" % int(need.value))
            e.needed, e.sizes = int(need.value), sizes[:pieces].copy()
            raise e
        self._check(rc, "tbk_zlib_deflate")
        if n == 0:
            return []
        assert int(sizes[:pieces].sum()) == int(need.value)
        ends = np.cumsum(sizes[:pieces].astype(np.uint64))
        return [out[int(e) - int(s):int(e)].tobytes() for s, e in zip(sizes[:pieces], ends)]

    def bigwig_build(self, tid, start, end, val, ref_len):
        """tbk_bigwig_build: the compressed sections of a bigWig file from coverage rows (numpy arrays or device tensors; the value is
        taken as float32) and the chromosome lengths.  Returns the levels, data first: dicts of reduction (0: the data), n_items,
        max_payload, bytes (the level's zlib streams back to back) and sections [(chrom, start, end, offset, size)]."""
        keep = []
        dev = _is_torch(tid)
        n = _numel(tid)
        rows = _lib.TrackRows(_lib.TBK_MEM_DEVICE if dev else _lib.TBK_MEM_HOST, _lib.TRACK["cov"], n, 0, _addr(tid, np.int32, keep, n),
                              _addr(start, np.int32, keep, n), _addr(end, np.int32, keep, n), _addr(val, np.float64, keep, n), None, None, None, 0)
        lens = np.ascontiguousarray(ref_len, dtype=np.uint32)
        self._order_after_torch(dev)
        out = _lib.BwOut()
        parts = {}
        tables = {}

        def sink(_user, level, p, nb):
            if level not in tables:   # (the level's table is complete before its first byte)
                lv = out.level[level]
                tables[level] = [(int(s.chrom), int(s.start), int(s.end), int(s.offset), int(s.size))
                                 for s in lv.sections[:int(lv.n_sections)]]
            parts.setdefault(level, []).append(C.string_at(p, nb))
            return 0

        cb = _lib.BW_SINK(sink)
        self._check(self.L.tbk_bigwig_build(self.h, C.byref(rows), len(lens), lens.ctypes.data if len(lens) else None, cb, None, C.byref(out)),
                    "tbk_bigwig_build")
        levels = []
        for k in range(int(out.n_levels)):
            lv = out.level[k]
            data = b"".join(parts.get(k, []))
            assert len(data) == int(lv.bytes) and len(tables.get(k, [])) == int(lv.n_sections)
            levels.append(dict(reduction=int(lv.reduction), n_items=int(lv.n_items), max_payload=int(lv.max_payload), bytes=data,
                               sections=tables.get(k, [])))
        return levels


def index_query(bam_path, tid, beg, end, index_path=None):
    """tbh_index_query: the chunks [(vbeg, vend)] a reader of [beg, end) on reference tid has to read, through the file's index
    (index_path None: PATH.csi, PATH.bai, then the .bai beside the stem).  Host only."""
    H = _lib.load_host()
    ip = None if index_path is None else os.fsencode(index_path)
    cap = 64
    while True:
        cb, ce = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        n = H.tbh_index_query(os.fsencode(bam_path), ip, int(tid), int(beg), int(end), cb.ctypes.data, ce.ctypes.data, cap)
        if n < 0:
            raise RuntimeError((H.tbh_last_error() or b"").decode())
        if n <= cap:
            return [(int(cb[i]), int(ce[i])) for i in range(n)]
        cap = int(n)


def _table_arrays(table):
    t = [(int(a), int(b), int(c)) for a, b, c in table]
    return (np.array([x[0] for x in t], dtype=np.int32), np.array([x[1] for x in t], dtype=np.int64), np.array([x[2] for x in t], dtype=np.int64))


def _regions(table):
    """[(tid, beg, end)] -> (tbk_regions struct over host arrays, the arrays to keep alive)"""
    tid, beg, end = _table_arrays(table)
    return _lib.Regions(len(tid), tid.ctypes.data, beg.ctypes.data, end.ctypes.data), (tid, beg, end)


def _grown(v, cap):
    """a copy of the rows v in an array of cap elements (the rest zero)"""
    if _is_torch(v):
        g = _torch().zeros(cap, dtype=v.dtype, device=v.device)
    else:
        v = np.asarray(v)
        g = np.zeros(cap, dtype=v.dtype)
    g[:min(cap, len(v))] = v[:cap]
    return g


def regions_from_bed(bam_path, bed_path):
    """tbh_regions_from_bed: the BED file's intervals against the header of bam_path as the normalised table [(tid, beg, end)]: sorted,
    merged where they overlap or abut, ends cut to the reference, empty ones dropped.  RuntimeError (with the line number) for a
    malformed line, an unknown chrom, a file without a region.  Host only."""
    H = _lib.load_host()
    cap = 64
    while True:
        t, b, e = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
        n = H.tbh_regions_from_bed(os.fsencode(bam_path), os.fsencode(bed_path), t.ctypes.data, b.ctypes.data, e.ctypes.data, cap)
        if n < 0:
            raise RuntimeError((H.tbh_last_error() or b"").decode())
        if n <= cap:
            return [(int(t[i]), int(b[i]), int(e[i])) for i in range(n)]
        cap = int(n)


def features_from_bed(bam_path, bed_path):
    """tbh_features_from_bed: the BED file's lines against the header of bam_path as features, one per line in the file's order (nothing
    merged, sorted or dropped): a dict of numpy arrays tid (int32), beg, end (int64, the end cut to the reference), strand (uint8: '+',
    '-', '.') and line (uint64, the line in the file from 1) and the list name.  RuntimeError (with the line number) for a malformed
    line, an unknown chrom, a strand other than + - ., a feature that is empty after the cut.  Host only."""
    H = _lib.load_host()
    cap, ncap = 64, 1024
    while True:
        t, b, e = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
        s, ln = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint64)
        names, nb = C.create_string_buffer(ncap), C.c_uint64(0)
        n = H.tbh_features_from_bed(os.fsencode(bam_path), os.fsencode(bed_path), t.ctypes.data, b.ctypes.data, e.ctypes.data, s.ctypes.data, ln.ctypes.data,
                                    cap, C.cast(names, C.c_void_p), ncap, C.byref(nb))
        if n < 0:
            raise RuntimeError((H.tbh_last_error() or b"").decode())
        if n <= cap and nb.value <= ncap:
            return dict(tid=t[:n].copy(), beg=b[:n].copy(), end=e[:n].copy(), strand=s[:n].copy(), line=ln[:n].copy(),
                        name=[x.decode() for x in names.raw[:nb.value].split(b"\0")[:n]])
        cap, ncap = max(cap, int(n)), max(ncap, int(nb.value))


def cov_summary_host(rows, features):
    """tbh_cov_summary_host: Context.cov_summary's columns by the host summariser (plain loops, a feature's rows added in row order)
    from numpy rows and a dict of feature arrays tid / beg / end (/ strand).  Host only."""
    H = _lib.load_host()
    keep = []
    ft, fb, fe = (np.ascontiguousarray(features[k], dtype=d) for k, d in (("tid", np.int32), ("beg", np.int64), ("end", np.int64)))
    fs = np.ascontiguousarray(features["strand"], dtype=np.uint8) if features.get("strand") is not None else None
    n = len(ft)
    want_cov, want_junc = "iv_tid" in rows, "j_tid" in rows
    a, b = (len(rows["iv_tid"]) if want_cov else 0), (len(rows["j_tid"]) if want_junc else 0)

    def ptr(name, dt, cnt):
        return _addr(rows[name], dt, keep, cnt) if cnt else None
    res = dict(covered=np.zeros(n, dtype=np.uint64), sum=np.zeros(n), max=np.zeros(n), junc=np.zeros(n))
    rc = H.tbh_cov_summary_host(n, ft.ctypes.data, fb.ctypes.data, fe.ctypes.data, fs.ctypes.data if fs is not None else None, int(want_cov), a,
                                ptr("iv_tid", np.int32, a), ptr("iv_start", np.int32, a), ptr("iv_end", np.int32, a), ptr("iv_val", np.float64, a), int(want_junc), b,
                                ptr("j_tid", np.int32, b), ptr("j_start", np.int32, b), ptr("j_end", np.int32, b), ptr("j_strand", np.uint8, b), ptr("j_val", np.float64, b),
                                *(res[k].ctypes.data for k in ("covered", "sum", "max", "junc")))
    if rc != 0:
        raise RuntimeError((H.tbh_last_error() or b"").decode())
    return res


def cov_thresholds_host(rows, features, thr):
    """tbh_cov_thresholds_host: Context.cov_thresholds' columns by the host loop, from numpy rows and a dict of feature arrays
    tid / beg / end.  RuntimeError for what the device entry refuses of the thresholds and the features' count.  Host only."""
    H = _lib.load_host()
    keep = []
    ft, fb, fe = (np.ascontiguousarray(features[k], dtype=d) for k, d in (("tid", np.int32), ("beg", np.int64), ("end", np.int64)))
    n = len(ft)
    t = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
    a = len(rows["iv_tid"]) if "iv_tid" in rows else 0

    def ptr(name, dt):
        return _addr(rows[name], dt, keep, a) if a else None
    res = dict(covered=np.zeros(n, dtype=np.uint64), ge=np.zeros((n, len(t)), dtype=np.uint64))
    rc = H.tbh_cov_thresholds_host(n, ft.ctypes.data, fb.ctypes.data, fe.ctypes.data, a, ptr("iv_tid", np.int32), ptr("iv_start", np.int32), ptr("iv_end", np.int32),
                                   ptr("iv_val", np.float64), t.ctypes.data if len(t) else None, len(t), res["covered"].ctypes.data if n else None,
                                   res["ge"].ctypes.data if n and len(t) else None)
    if rc != 0:
        raise RuntimeError((H.tbh_last_error() or b"").decode())
    return res


def parse_thresholds(text):
    """tbh_parse_thresholds: a --thresholds list as the command lines parse it -> the thresholds (float64 array); RuntimeError names the
    offending item.  Host only."""
    H = _lib.load_host()
    t = np.zeros(_lib.MAX_THRESHOLDS, dtype=np.float64)
    n = H.tbh_parse_thresholds(os.fsencode(text), t.ctypes.data, len(t))
    if n < 0:
        raise RuntimeError((H.tbh_last_error() or b"").decode())
    return t[:n].copy()


def transcripts_from_gtf(bam_path, gtf_path):
    """tbh_transcripts_from_gtf: the exon lines of the GTF file against the header of bam_path as a transcript table: a dict of numpy
    arrays tx_off (uint32, [n_tx + 1], CSR into the exons), tid (int32), strand (uint8), line (uint64: the line of the transcript's
    first exon line, from 1), ex_beg / ex_end (int64, 0-based half-open, ascending within a transcript) and the lists id and gene.
    Transcripts come in the order of their first appearance.  RuntimeError (with the line number) for what the parser refuses.  Host
    only."""
    H = _lib.load_host()
    tcap, ecap, ncap = 64, 256, 4096
    while True:
        off, t = np.zeros(tcap + 1, dtype=np.uint32), np.zeros(tcap, dtype=np.int32)
        s, ln = np.zeros(tcap, dtype=np.uint8), np.zeros(tcap, dtype=np.uint64)
        eb, ee = np.zeros(ecap, dtype=np.int64), np.zeros(ecap, dtype=np.int64)
        names, nb, ne = C.create_string_buffer(ncap), C.c_uint64(0), C.c_uint64(0)
        n = H.tbh_transcripts_from_gtf(os.fsencode(bam_path), os.fsencode(gtf_path), off.ctypes.data, t.ctypes.data, s.ctypes.data, ln.ctypes.data, tcap,
                                       eb.ctypes.data, ee.ctypes.data, ecap, C.byref(ne), C.cast(names, C.c_void_p), ncap, C.byref(nb))
        if n < 0:
            raise RuntimeError((H.tbh_last_error() or b"").decode())
        if n <= tcap and ne.value <= ecap and nb.value <= ncap:
            both = [x.decode() for x in names.raw[:nb.value].split(b"\0")[:2 * n]]
            m = int(ne.value)
            return dict(tx_off=off[:n + 1].copy(), tid=t[:n].copy(), strand=s[:n].copy(), line=ln[:n].copy(), ex_beg=eb[:m].copy(), ex_end=ee[:m].copy(),
                        id=both[0::2], gene=both[1::2])
        tcap, ecap, ncap = max(tcap, int(n)), max(ecap, int(ne.value)), max(ncap, int(nb.value))


def tx_summary_host(rows, tx):
    """tbh_tx_summary_host: Context.tx_summary's columns (the per-exon ones included) by the host summariser (plain loops, a
    transcript's parts added in exon order) from numpy rows and a transcript table as Context.tx_summary takes it.  Host only."""
    H = _lib.load_host()
    keep = []
    off = np.ascontiguousarray(tx["tx_off"], dtype=np.uint32)
    tt = np.ascontiguousarray(tx["tid"], dtype=np.int32)
    eb, ee = np.ascontiguousarray(tx["ex_beg"], dtype=np.int64), np.ascontiguousarray(tx["ex_end"], dtype=np.int64)
    ts = np.ascontiguousarray(tx["strand"], dtype=np.uint8) if tx.get("strand") is not None else None
    n_tx, n_ex = len(tt), len(eb)
    want_cov, want_junc = "iv_tid" in rows, "j_tid" in rows
    a, b = (len(rows["iv_tid"]) if want_cov else 0), (len(rows["j_tid"]) if want_junc else 0)

    def ptr(name, dt, cnt):
        return _addr(rows[name], dt, keep, cnt) if cnt else None
    cols = ("covered", "sum", "max", "exons_hit", "introns_hit", "junc_min", "junc_sum", "ex_covered", "ex_sum", "ex_max", "in_junc")
    dts = dict(covered=np.uint64, exons_hit=np.uint32, introns_hit=np.uint32, ex_covered=np.uint64)
    res = {k: np.zeros(n_ex if k in cols[7:] else n_tx, dtype=dts.get(k, np.float64)) for k in cols}
    rc = H.tbh_tx_summary_host(n_tx, n_ex, off.ctypes.data if len(off) else None, tt.ctypes.data if n_tx else None, ts.ctypes.data if ts is not None else None,
                               eb.ctypes.data if n_ex else None, ee.ctypes.data if n_ex else None, int(want_cov), a, ptr("iv_tid", np.int32, a),
                               ptr("iv_start", np.int32, a), ptr("iv_end", np.int32, a), ptr("iv_val", np.float64, a), int(want_junc), b, ptr("j_tid", np.int32, b),
                               ptr("j_start", np.int32, b), ptr("j_end", np.int32, b), ptr("j_strand", np.uint8, b), ptr("j_val", np.float64, b),
                               *(res[k].ctypes.data if len(res[k]) else None for k in cols))
    if rc != 0:
        raise RuntimeError((H.tbh_last_error() or b"").decode())
    for k in (() if want_cov else cols[:4] + cols[7:10]) + (() if want_junc else cols[4:7] + cols[10:]):
        del res[k]
    return res


def index_query_regions(bam_path, table, index_path=None):
    """tbh_index_query_regions: index_query for a normalised table [(tid, beg, end)]: the chunks of all intervals, merged over the whole
    set so that no file byte is in two of them.  Host only."""
    H = _lib.load_host()
    ip = None if index_path is None else os.fsencode(index_path)
    tid, beg, end = _table_arrays(table)
    cap = 64
    while True:
        cb, ce = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        n = H.tbh_index_query_regions(os.fsencode(bam_path), ip, len(tid), tid.ctypes.data, beg.ctypes.data, end.ctypes.data, cb.ctypes.data, ce.ctypes.data, cap)
        if n < 0:
            raise RuntimeError((H.tbh_last_error() or b"").decode())
        if n <= cap:
            return [(int(cb[i]), int(ce[i])) for i in range(n)]
        cap = int(n)


STRAND_CLASSES = ("plus", "minus", "none")   # the views of cov_split_strand, in order


def cov_view_to_numpy(view) -> CovInput:
    """The arrays of a DeviceCovView copied back to the host as a CovInput (tests and tools): a column the view lacks is None (flag, and
    yc / yx where the input had none); an empty view gives empty arrays and cig_off == [0]."""
    s, n, nc = view.struct, int(view.n_records), int(view.n_cigar_ops)
    hip = C.CDLL("libamdhip64.so")

    def col(name, dt, cnt):
        ptr = getattr(s, name)
        if not ptr and name in ("flag", "yc", "yx"):
            return None
        a = np.zeros(cnt, dtype=dt)
        if cnt and ptr and n:
            rc = hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), 2)
            if rc != 0:
                raise RuntimeError("hipMemcpy failed (%d)" % rc)
        return a

    return CovInput(tid=col("tid", np.int32, n), pos=col("pos", np.int32, n), flag=col("flag", np.uint16, n),
                    cig_off=col("cig_off", np.uint32, n + 1), cig=col("cig", np.uint32, nc), yc=col("yc", np.float64, n),
                    strand=col("strand", np.uint8, n), yx=col("yx", np.int64, n))


def split_strand_host(cin: CovInput):
    """The rule of tbk_cov_split_strand in numpy: [the records with strand '+', with '-', with any other byte], each a CovInput in the
    input's order without the unmapped records (flag bit 0x4; flag None: every record is mapped), CIGAR CSR rebuilt from 0, flag None,
    every other column copied bit for bit."""
    if cin.strand is None:
        raise ValueError("split_strand_host: the input carries no strand column")
    n = int(np.asarray(cin.tid).shape[0])
    strand = np.asarray(cin.strand, dtype=np.uint8)
    mapped = np.ones(n, dtype=bool) if cin.flag is None else (np.asarray(cin.flag, dtype=np.uint16) & 0x4) == 0
    cls = np.where(strand == ord("+"), 0, np.where(strand == ord("-"), 1, 2))
    off = np.asarray(cin.cig_off, dtype=np.uint32).astype(np.int64)
    cig = np.asarray(cin.cig, dtype=np.uint32)
    out = []
    for k in range(3):
        idx = np.flatnonzero(mapped & (cls == k))
        cnt = off[idx + 1] - off[idx]
        noff = np.zeros(len(idx) + 1, dtype=np.int64)
        np.cumsum(cnt, out=noff[1:])
        # word j of the part comes from off[record] + (j - the record's new offset)
        src = np.repeat(off[idx] - noff[:-1], cnt) + np.arange(int(noff[-1]), dtype=np.int64)
        out.append(CovInput(tid=np.asarray(cin.tid, dtype=np.int32)[idx], pos=np.asarray(cin.pos, dtype=np.int32)[idx], flag=None,
                            cig_off=noff.astype(np.uint32), cig=cig[src], yc=None if cin.yc is None else np.asarray(cin.yc, dtype=np.float64)[idx],
                            strand=strand[idx], yx=None if cin.yx is None else np.asarray(cin.yx, dtype=np.int64)[idx]))
    return out


def _split_strand_libtbh(cin: CovInput):
    """tbh_split_strand_host: the same rule by the command lines' host loop (libtbh.so; TBK_SPLIT_HOST=1), as three CovInput"""
    H = _lib.load_host()
    n, nc = int(np.asarray(cin.tid).shape[0]), int(np.asarray(cin.cig).shape[0])
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        b = np.ascontiguousarray(a, dtype=dt)
        keep.append(b)
        return b.ctypes.data
    n_rec, n_cig = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    o_tid, o_pos, o_strand = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    o_off, o_cig = np.zeros(n + 3, np.uint32), np.zeros(nc, np.uint32)
    o_yc = np.zeros(n, np.float64) if cin.yc is not None else None
    o_yx = np.zeros(n, np.int64) if cin.yx is not None else None
    rc = H.tbh_split_strand_host(n, nc, ptr(cin.tid, np.int32), ptr(cin.pos, np.int32), ptr(cin.flag, np.uint16), ptr(cin.cig_off, np.uint32), ptr(cin.cig, np.uint32),
                                 ptr(cin.yc, np.float64), ptr(cin.strand, np.uint8), ptr(cin.yx, np.int64), n_rec.ctypes.data, n_cig.ctypes.data, o_tid.ctypes.data,
                                 o_pos.ctypes.data, o_off.ctypes.data, o_cig.ctypes.data, None if o_yc is None else o_yc.ctypes.data, o_strand.ctypes.data,
                                 None if o_yx is None else o_yx.ctypes.data)
    if rc != 0:
        raise RuntimeError((H.tbh_last_error() or b"").decode())
    out, r, w = [], 0, 0
    for s in range(3):
        m, c = int(n_rec[s]), int(n_cig[s])
        out.append(CovInput(tid=o_tid[r:r + m].copy(), pos=o_pos[r:r + m].copy(), flag=None, cig_off=o_off[r + s:r + s + m + 1].copy(), cig=o_cig[w:w + c].copy(),
                            yc=None if o_yc is None else o_yc[r:r + m].copy(), strand=o_strand[r:r + m].copy(), yx=None if o_yx is None else o_yx[r:r + m].copy()))
        r, w = r + m, w + c
    return out


def to_numpy(d):
    """Bring every tensor value of a result dict back to numpy (tests / writers)."""
    out = {}
    for k, v in d.items():
        if k.startswith("_"):
            continue
        out[k] = v.cpu().numpy() if _is_torch(v) else v
    if "rep" in out and out["rep"].dtype == np.int32:
        out["rep"] = out["rep"].view(np.uint32)
    return out
