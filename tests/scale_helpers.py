"""Array-for-array comparison of the HIP path with the CPU oracle on tiles of hundreds of millions of records
(`tests/test_gpu_scale.py`; the comparator, the coverage split and the memory formula are tested without a GPU in
`tests/test_scale_compare_cpu.py`).

  * `exact_at_scale`: collapse + tiecov on the GPU (production path, no TBK_DEBUG form), results to numpy, the tile to the
    host and off the device, the oracle on the host tile, every output array compared bit for bit;
  * `compare_results`: a mismatch names the array, the number of differing entries, the first differing index, the group
    there and the window of the tile that reproduces it on a small tile;
  * `oracle_coverage`: the oracle's tiecov, one call or one call per reference sequence (its capacity field is 32 bits wide);
  * `memory_need` / `host_memory_budget`: what a comparison holds on the host, known before it allocates;
  * `chain_stats`: the YD chains of a collapsed tile, from the oracle's result.
"""
import numpy as np

GROUP_KEYS = ("rep", "yc", "yx", "yd", "g_start", "g_end", "rec_group")
COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")
STRATEGY = {"cigar": 0, "full": 1, "clip": 2, "exon": 3}
WINDOW_MARGIN = 1000        # bases kept beyond the failing group's start: every record of its (tid, start) bucket and the next ones


# ---------------------------------------------------------------------------------------------------------------------
# host memory

def host_memory_budget():
    """bytes this process may use: min(cgroup limit, MemAvailable) — the rule of bench.host_memory_budget (read only)"""
    lim = None
    for p in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
        try:
            v = open(p).read().strip()
            if v.isdigit():
                lim = int(v)
                break
        except OSError:
            pass
    avail = None
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                avail = int(line.split()[1]) * 1024
    except OSError:
        pass
    c = [x for x in (lim, avail) if x]
    return min(c) if c else 16 << 30


def tile_bytes(n, ncig, n_files):
    """numpy SoATile of a plain tile: tid pos nh 4, flag 2, mapq strand 1, cig_off 4 (n + 1), cig 4, file_off 4, tbmerged 1"""
    return 16 * n + 4 * (n + 1) + 4 * ncig + 4 * (n_files + 1) + n_files


def groups_bytes(n, g):
    """a collapse result with rec_group: rep 4, yc 8, yx 8, yd 4, g_start 4, g_end 4 per group, rec_group 4 per record"""
    return 32 * g + 4 * n


def collapse_work_bytes(n):
    """oracle_ffi.collapse sizes its seven output arrays for one group per record (36 B) before it trims them; tbo_collapse itself
    holds st, en (4 B each) and the joined pointers (8 B) per record"""
    return groups_bytes(max(n, 1), max(n, 1)) + 16 * (n + 1)


def cov_input_bytes(g, gcig):
    """soa.CovInput: tid pos 4, flag 2, yc 8, strand 1, yx 8 per record, cig_off 4 (g + 1), cig 4"""
    return 27 * g + 4 * (g + 1) + 4 * gcig


def cov_input_temp_bytes(n, g, gcig):
    """synth.collapsed_to_cov_input's int64 temporaries: the tile's cig_off, rep / ncig / the gather base per group, three index
    arrays per CIGAR word"""
    return 8 * (n + 1) + 24 * g + 24 * gcig


def cov_capacity(g, gcig):
    """(intervals, junctions) oracle_ffi.coverage allocates for an input of g records and gcig CIGAR words"""
    return 2 * gcig + 2 * g + 16, gcig + 16


def cov_work_bytes(g, gcig):
    ci, cj = cov_capacity(g, gcig)
    return 20 * ci + 21 * cj + 24            # (the sample track's arrays are one entry each)


def cov_bytes(ni, nj):
    """the nine coverage arrays: three int32 + a double per interval, three int32 + a byte + a double per junction"""
    return 20 * ni + 21 * nj


def memory_need(n, ncig, n_files, g, gcig, ni, nj, cov_share=1.0):
    """Peak host bytes of one exact comparison: the host tile and the GPU's results stay throughout; on top of them the oracle's
    collapse (work arrays, then its trimmed result), then the tiecov input being built, then the oracle's tiecov (work arrays and
    the trimmed result, and once more the result while the parts are joined).  `cov_share`: the part of the tiecov input that one
    oracle call sees — 1 for a single call, the largest reference's share when the call is split by reference."""
    base = tile_bytes(n, ncig, n_files) + groups_bytes(n, g) + cov_bytes(ni, nj)
    a = collapse_work_bytes(n) + groups_bytes(n, g)
    b = groups_bytes(n, g) + cov_input_bytes(g, gcig) + cov_input_temp_bytes(n, g, gcig)
    c = groups_bytes(n, g) + cov_input_bytes(g, gcig) + int(cov_work_bytes(g, gcig) * min(cov_share, 1.0)) + 2 * cov_bytes(ni, nj)
    return base + max(a, b, c)


def nbytes_of(obj):
    """bytes of the numpy arrays of a tile, a CovInput or a result dict"""
    vals = obj.values() if isinstance(obj, dict) else vars(obj).values()
    return sum(int(v.nbytes) for v in vals if isinstance(v, np.ndarray))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's tiecov, whole or per reference

def _cov_slice(cin, a, b):
    from tiebrush_amd.soa import CovInput
    co = cin.cig_off
    lo, hi = int(co[a]), int(co[b])
    return CovInput(tid=cin.tid[a:b], pos=cin.pos[a:b], flag=cin.flag[a:b], cig_off=(co[a:b + 1] - co[a]).astype(np.uint32),
                    cig=cin.cig[lo:hi], yc=cin.yc[a:b], strand=None if cin.strand is None else cin.strand[a:b],
                    yx=None if cin.yx is None else cin.yx[a:b])


def oracle_coverage(cin, split=None):
    """orc.coverage(cin).  The oracle keeps its interval capacity (2 * ncig + 2 * n + 16) in a 32-bit field: an input that would
    reach 2^32 — or `split=True` — goes one reference sequence at a time (runs of equal tid: intervals, junctions and bundles never
    cross a reference) and the rows are concatenated, the two base counters added."""
    from oracle import oracle_ffi as orc
    n = cin.n_records
    if split is None:
        split = cov_capacity(n, int(cin.cig.shape[0]))[0] >= 2**32
    if not split or n == 0:
        return orc.coverage(cin)
    cut = np.concatenate([[0], np.flatnonzero(cin.tid[1:] != cin.tid[:-1]) + 1, [n]])
    parts = [orc.coverage(_cov_slice(cin, int(a), int(b))) for a, b in zip(cut[:-1], cut[1:])]
    out = {k: np.concatenate([p[k] for p in parts]) for k in COV_KEYS}
    for k in ("n_intervals", "n_junctions", "n_bases", "span_bases"):
        out[k] = sum(int(p[k]) for p in parts)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the comparator

def _file_of(tile, rec):
    return int(np.searchsorted(np.asarray(tile.file_off).astype(np.int64), int(rec), side="right") - 1)


def _hint(desc, tid, start):
    return ("\n  reproduce on a small tile (the YD lists restart at every reference, SURVEY.md §3.3):\n"
            "    tile = %s\n    small = synth_dev.tile_to_host(tile, window=(%d, 0, %d))"
            % (desc or "<the tile of this test>", int(tid), max(int(start), 0) + WINDOW_MARGIN))


def _group_line(tile, res, i, who):
    r = int(res["rep"][i])
    return "%s: group %d = (tid %d, g_start %d, g_end %d, strand %s), rep %d in file %d" % (
        who, i, int(tile.tid[r]), int(res["g_start"][i]), int(res["g_end"][i]), chr(int(tile.strand[r])), r, _file_of(tile, r))


def _diff(name, got, want):
    """None when equal, else (number of differing entries, first differing index, text) — a length difference counts the tail"""
    got, want = np.asarray(got), np.asarray(want)
    m = min(len(got), len(want))
    ne = got[:m] != want[:m]
    bad = int(np.count_nonzero(ne)) + abs(len(got) - len(want))
    if bad == 0:
        return None
    first = int(np.argmax(ne)) if ne.any() else m
    txt = "%s: %d of %d entries differ, first at index %d" % (name, bad, max(len(got), len(want)), first)
    if len(got) != len(want):
        txt += " (lengths: got %d, oracle %d)" % (len(got), len(want))
    return bad, first, txt


def _val(a, i):
    return repr(a[i].item()) if i < len(a) else "<absent>"


def compare_results(tile, got, want, cov_got, cov_want, desc=None):
    """`got` / `want`: collapse results (numpy, with rec_group and the coordinates) of the HIP path and of the oracle on the host
    tile `tile`; `cov_got` / `cov_want`: their tiecov results.  Raises AssertionError on the first array that differs."""
    for k in ("n_groups", "n_passed"):
        assert int(got[k]) == int(want[k]), "%s: got %d, oracle %d" % (k, int(got[k]), int(want[k]))
    for k in GROUP_KEYS:
        d = _diff(k, got[k], want[k])
        if d is None:
            continue
        _, i, txt = d
        if k == "rec_group":                  # indexed by record
            txt += "\n  record %d = (tid %d, pos %d, file %d): got group %s, oracle group %s" % (
                i, int(tile.tid[i]), int(tile.pos[i]), _file_of(tile, i), _val(got[k], i), _val(want[k], i))
            tid, start = int(tile.tid[i]), int(tile.pos[i])
        else:
            txt += "\n  got %s, oracle %s" % (_val(got[k], i), _val(want[k], i))
            tid = start = 0
            for who, res in (("oracle", want), ("got", got)):
                if i < len(res["rep"]) and int(res["rep"][i]) < tile.n_records:
                    txt += "\n  " + _group_line(tile, res, i, who)
            if i < len(want["rep"]):
                tid, start = int(tile.tid[int(want["rep"][i])]), int(want["g_start"][i])
        raise AssertionError(txt + _hint(desc, tid, start))
    for k in COV_KEYS:
        d = _diff(k, cov_got[k], cov_want[k])
        if d is None:
            continue
        _, i, txt = d
        p = k.split("_")[0]
        txt += "\n  got %s, oracle %s" % (_val(cov_got[k], i), _val(cov_want[k], i))
        tid = start = 0
        for who, res in (("oracle", cov_want), ("got", cov_got)):
            if i < len(res[p + "_tid"]):
                txt += "\n  %s: row %d = (tid %d, start %d, end %d)" % (who, i, int(res[p + "_tid"][i]), int(res[p + "_start"][i]),
                                                                       int(res[p + "_end"][i]))
        if i < len(cov_want[p + "_tid"]):
            tid, start = int(cov_want[p + "_tid"][i]), int(cov_want[p + "_start"][i])
        raise AssertionError(txt + _hint(desc, tid, start))
    for k in ("n_bases", "span_bases"):
        assert int(cov_got[k]) == int(cov_want[k]), "%s: got %d, oracle %d" % (k, int(cov_got[k]), int(cov_want[k]))


# ---------------------------------------------------------------------------------------------------------------------
# what the tile holds

def chain_stats(tile, want, device="cpu"):
    """The YD chains of a collapsed plain tile, rebuilt from the oracle's result `want` (torch on `device`, as an array processor).
    An item is a (file, group) pair with a member of the group in the file; it sits in the file's '+' list, its '-' list or — a
    representative of strand '.' — both, in group order.  An item opens a chain when it is the first of its list, when its reference
    differs from the item before it, or when it starts beyond every `end + 1` of the list's earlier items on that reference: the
    list machine holds no node there (YD).  Returns dict(items, chains, longest)."""
    import torch
    n, g = tile.n_records, int(want["n_groups"])
    fo = torch.from_numpy(np.asarray(tile.file_off).astype(np.int64)).to(device)
    rg = torch.from_numpy(np.ascontiguousarray(want["rec_group"])).to(device).to(torch.int64)
    fidx = torch.repeat_interleave(torch.arange(tile.n_files, device=device), fo[1:] - fo[:-1])
    plain = torch.from_numpy(np.asarray(tile.tbmerged) == 0).to(device)
    pair = torch.unique((fidx * g + rg)[(rg >= 0) & plain[fidx]])            # sorted: by file, then group
    del rg, fidx
    f, grp = pair // g, pair % g
    del pair
    rep = np.asarray(want["rep"]).astype(np.int64)
    tid = torch.from_numpy(np.asarray(tile.tid)[rep].astype(np.int64)).to(device)[grp]
    strand = torch.from_numpy(np.asarray(tile.strand)[rep]).to(device)[grp]
    start = torch.from_numpy(np.asarray(want["g_start"]).astype(np.int64)).to(device)[grp]
    end = torch.from_numpy(np.asarray(want["g_end"]).astype(np.int64)).to(device)[grp]
    out = dict(items=0, chains=0, longest=0)
    for s in (ord("+"), ord("-")):
        m = (strand == s) | (strand == ord("."))
        k = int(m.sum())
        if k == 0:
            continue
        seg = f[m] * (1 << 20) + tid[m] + 1                                   # (file, reference) runs; non-decreasing
        st, en = start[m], end[m]
        run = torch.cummax(seg * (1 << 32) + en + 1, 0)[0]                   # the segment in the high bits restarts the maximum
        head = torch.ones(k, dtype=torch.bool, device=device)
        head[1:] = (seg[1:] != seg[:-1]) | (seg[1:] * (1 << 32) + st[1:] > run[:-1])
        at = torch.nonzero(head).flatten()
        ln = torch.diff(at, append=torch.tensor([k], device=device))
        out["items"] += k
        out["chains"] += int(at.numel())
        out["longest"] = max(out["longest"], int(ln.max()))
    return out


def content_checks(tile, want, min_longest_chain=None, device="cpu"):
    """The tile holds what a YD / representative test needs (asserted from the oracle's result); returns the chain statistics."""
    st = chain_stats(tile, want, device)
    assert int(np.asarray(want["yd"]).max()) > 0, "no group of the tile has a YD"
    rep = np.asarray(want["rep"]).astype(np.int64)
    assert bool((rep >= int(tile.file_off[1])).any()), "every representative lies in file 0"
    if min_longest_chain is not None:
        assert st["longest"] >= min_longest_chain, "longest YD chain %d < %d" % (st["longest"], min_longest_chain)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# the whole comparison

class TileTooLarge(Exception):
    def __init__(self, need, avail):
        Exception.__init__(self, "the exact comparison needs %d bytes of host memory, %d are available" % (need, avail))
        self.need, self.avail = need, avail


def _gpu_results(ctx, dt, kw):
    """collapse + tiecov on the GPU; the counts that size everything else, and a function that fetches the arrays"""
    import torch
    from tiebrush_amd import api
    res = ctx.collapse(dt, want_rec_group=True, **kw)
    view = ctx.groups_to_cov_in(res)
    cov = ctx.coverage(view)
    counts = dict(g=int(res["n_groups"]), gcig=int(view.n_cigar_ops), ni=int(cov["n_intervals"]), nj=int(cov["n_junctions"]))
    # the largest reference's share of the groups, a quarter added for CIGARs that are longer there than elsewhere
    per_ref = torch.bincount(dt.tid[res["rep"].to(torch.int64) & 0xFFFFFFFF].to(torch.int64) + 1)
    counts["share"] = min(1.0, 1.25 * int(per_ref.max()) / max(counts["g"], 1))

    def fetch():
        return api.to_numpy({k: res[k] for k in GROUP_KEYS + ("n_groups", "n_passed")}), \
            api.to_numpy({k: cov[k] for k in COV_KEYS + ("n_intervals", "n_junctions", "n_bases", "span_bases")})

    return counts, fetch


def prefix_window(tile, fraction):
    """(tid, 0, hi): the prefix of the tile's first reference sequence that holds about `fraction` of the tile's records (all of
    that reference when it holds fewer)"""
    import torch
    t0 = int(tile.tid.min())
    pos = torch.sort(tile.pos[tile.tid == t0])[0]
    k = int(tile.n_records * fraction)
    hi = int(pos[k]) if k < pos.numel() else int(pos[-1]) + 1
    return (t0, 0, hi)


def exact_at_scale(ctx, make_tile, desc, budget=None, too_large="raise", log=print, **kw):
    """`make_tile()` returns a synth_dev device tile (or a numpy tile, sent with api.to_device); `kw`: the collapse options.
    Returns (host tile, the oracle's collapse result, the oracle's tiecov result, info) after every array compared equal.
    A tile whose comparison does not fit the host raises TileTooLarge — or, with too_large="window", is cut to the largest
    prefix of its first reference sequence that fits: the windowed tile goes back to the device and is compared whole."""
    import time
    import torch
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, synth, synth_dev
    budget = host_memory_budget() if budget is None else budget
    okw = dict(kw)
    if "strategy" in okw:
        okw["strategy"] = STRATEGY[okw["strategy"]]
    tile = make_tile()
    on_dev = api._is_torch(tile.tid)
    host = None if on_dev else tile
    dt = tile if on_dev else api.to_device(tile, "cuda:0")
    del tile
    info = dict(window=None, budget=budget)
    while True:
        n, ncig, nf = dt.n_records, int(dt.cig.shape[0]), dt.n_files
        counts, fetch = _gpu_results(ctx, dt, kw)
        need1 = memory_need(n, ncig, nf, counts["g"], counts["gcig"], counts["ni"], counts["nj"])
        over32 = cov_capacity(counts["g"], counts["gcig"])[0] >= 2**32
        split = over32 or need1 > budget
        need = memory_need(n, ncig, nf, counts["g"], counts["gcig"], counts["ni"], counts["nj"], counts["share"] if split else 1.0)
        info.update(n=n, need=need, split=split, **counts)
        log("exact %s: %d records, %d groups; host need %d B (%.1f GiB), budget %d B (%.1f GiB)%s"
            % (desc, n, counts["g"], need, need / 2**30, budget, budget / 2**30, ", tiecov oracle per reference" if split else ""))
        if need <= budget:
            break
        del fetch
        if too_large != "window" or info["window"] is not None or not on_dev:
            raise TileTooLarge(need, budget)
        info["full_need"] = need
        info["window"] = prefix_window(dt, 0.9 * budget / need)
        host = synth_dev.tile_to_host(dt, window=info["window"])
        del dt
        torch.cuda.empty_cache()
        dt = api.to_device(host, "cuda:0")
        desc = "synth_dev.tile_to_host(%s, window=%r)" % (desc, info["window"])
        log("windowed: %r, %d of %d records" % (info["window"], host.n_records, n))
    t0 = time.time()
    got, cov_got = fetch()
    if host is None:
        host = synth_dev.tile_to_host(dt)
    del dt, fetch
    torch.cuda.empty_cache()
    t1 = time.time()
    want = orc.collapse(host, want_rec_group=True, **okw)
    t2 = time.time()
    cov_want = oracle_coverage(synth.collapsed_to_cov_input(host, want), split=True if split else None)
    t3 = time.time()
    compare_results(host, got, want, cov_got, cov_want, desc)
    info.update(t_fetch=t1 - t0, t_oracle_collapse=t2 - t1, t_oracle_coverage=t3 - t2, t_compare=time.time() - t3)
    log("exact %s: equal; to host %.1f s, oracle collapse %.1f s, oracle tiecov %.1f s, compare %.1f s"
        % (desc, info["t_fetch"], info["t_oracle_collapse"], info["t_oracle_coverage"], info["t_compare"]))
    return host, want, cov_want, info
