"""A CPU model of the window path's partition and tiers (tiebrush_amd/csrc/wgroup.hip), in plain numpy.

It mirrors the HOST arithmetic of tbk_window_groups and the splitter rules of wg_tidchunks_k / wg_sample(_raw)_k / wg_split_k — the
constants carry the names they have there — and not the kernels: which window a record falls into is decided here by one
searchsorted over the bounds, not by the streaming offsets pass, and the number of distinct groups of a window comes from the
oracle's record -> group map.  From that it predicts what tbk_last_route reports under wg_stats=1: the windows, the windows that
hold records, the windows that overflow the first and the second group table, and whether one of the latter is a pile-up the LDS
sort cannot take (the tile then falls back to the sort path).

Thresholds, from the constants: a table of gcap slots takes a window whose distinct groups ("claims") number at most
(gcap >> 2) * 3, with gcap = (LDS - (8 k + 8)) / (44 + 4 * ceil(k / 32)) and LDS = WG_LDS_HASH (first tier) or WG_LDS_HASH2
(second); the raw form of at most 64 files has the compile-time tables WG_GC64 = 767 and WG_GC64_2 = 1250 slots: 573 and 936."""
import numpy as np

WG_NT = 512
WG_E = 8
WG_CAP = WG_NT * WG_E
WG_T = 1024
WG_KS = 2048
WG_TC = 4096
WG_OC = 2048
WG_OG = 8
WG_LDS_HASH = 40448
WG_LDS_HASH2 = 64 * 1024
WG_GC64 = (WG_LDS_HASH - (8 * 64 + 8)) // (44 + 4 * 2)
WG_GC64_2 = (WG_LDS_HASH2 - (8 * 64 + 8)) // (44 + 4 * 2)
WINDOW_MAX_FILES = 1024                 # tbk_window_supported
UNPLACED = 1 << 62                      # raw_key of tid < 0


def stride(k):
    """s (sample stride), g (samples per splitter): while (s * 2 * k <= WG_KS && s * 2 <= WG_T) s *= 2; g = WG_T / s"""
    s = 1
    while s * 2 * k <= WG_KS and s * 2 <= WG_T:
        s *= 2
    return s, WG_T // s


def gcaps(k, raw):
    """table slots of the two tiers for k files in the raw / compacted form"""
    if raw and k <= 64:
        return WG_GC64, WG_GC64_2
    nwords = (k + 31) // 32
    return tuple((lds - (8 * k + 8)) // (44 + 4 * nwords) for lds in (WG_LDS_HASH, WG_LDS_HASH2))


def thresholds(k, raw):
    """the most distinct groups a window may hold in the first and in the second table"""
    return tuple((g >> 2) * 3 for g in gcaps(k, raw))


def filter_mask(tile, keep_supplementary=False, keep_secondary=False, min_qual=-1, max_nh=2**31 - 1, **_):
    """passes_options as record_key (strategy.hpp) applies it"""
    fl = tile.flag.astype(np.uint32)
    ok = (fl & 4) == 0
    if not keep_supplementary:
        ok &= (fl & 0x800) == 0
    if not keep_secondary:
        ok &= (fl & 0x100) == 0
    ok &= tile.mapq.astype(np.int64) >= min_qual
    nh = tile.nh.astype(np.int64)
    nh = np.where(nh == -(2**31), 0, nh)
    ok &= nh <= max_nh
    return ok


def raw_key(tid, pos):
    tid = np.asarray(tid, np.int64)
    pos = np.asarray(pos, np.int64)
    return np.where(tid < 0, np.uint64(UNPLACED), (tid.astype(np.uint64) << np.uint64(31)) | (pos.astype(np.uint64) & np.uint64(0x7FFFFFFF)))


def tid_chunks(tile):
    """ctid of wg_tidchunks_k: the reference id of every chunk of WG_TC records that lies in one file and whose first and last record
    agree, None-coded as INT32_MIN otherwise"""
    n = tile.n_records
    fo = tile.file_off.astype(np.int64)
    k = tile.n_files
    nch = -(-n // WG_TC)
    a = np.arange(nch, dtype=np.int64) * WG_TC
    b = np.minimum(a + WG_TC - 1, n - 1)
    f = np.clip(np.searchsorted(fo[:k], a, side="right") - 1, 0, k - 1)     # last f < k with file_off[f] <= a
    same = (b < fo[f + 1]) & (tile.tid[b] == tile.tid[a])
    return np.where(same, tile.tid[a], np.int32(-(2**31))).astype(np.int32)


def split_bounds(Y, g, nsp):
    """wg_split_k: splitter i = Y[(i + 1) * g]; two bounds each — the first of a run of equal splitters (v, v + 1 if the run is longer
    than one, else v), the others (v + 1, v + 1).  Returns the bounds and, per splitter, whether its own window [v, v + 1) is a heavy one"""
    W = np.zeros(2 * nsp, np.uint64)
    if nsp == 0:
        return W, np.zeros(0, bool)
    v = Y[(np.arange(nsp) + 1) * g]
    pv = np.concatenate([[0], v[:-1]]).astype(np.uint64)
    nv = np.concatenate([v[1:], [0]]).astype(np.uint64)
    has_prev = np.arange(nsp) > 0
    has_next = np.arange(nsp) + 1 < nsp
    first = ~has_prev | (pv != v)
    heavy = (has_prev & (pv == v)) | (has_next & (nv == v))
    one = np.uint64(1)
    W[0::2] = np.where(first, v, v + one)
    W[1::2] = np.where(first & ~heavy, v, v + one)
    return W, first & heavy


class Partition:
    """the windows of one tile in one form"""

    def __init__(self, tile, raw, **opts):
        self.tile, self.raw, self.k = tile, raw, tile.n_files
        n = tile.n_records
        self.mask = filter_mask(tile, **opts)
        fo = tile.file_off.astype(np.int64)
        file_of = np.searchsorted(fo, np.arange(n), side="right") - 1
        if raw:
            self.rec = np.arange(n)
            self.keys = raw_key(tile.tid, tile.pos)
            ct = tid_chunks(tile) if n else np.zeros(0, np.int32)
        else:
            self.rec = np.flatnonzero(self.mask)
            t = tile.tid[self.rec].astype(np.int64) + 1
            p = tile.pos[self.rec].astype(np.int64) + 1
            self.keys = (t.astype(np.uint64) << np.uint64(31)) | p.astype(np.uint64)     # chi >> 2
        self.file = file_of[self.rec]
        m = self.m = len(self.rec)
        self.s, self.g = stride(self.k)
        self.ns = -(-m // self.s) if m else 0
        self.nsp = (self.ns - 1) // self.g if self.ns > 1 else 0
        self.nW = 2 * self.nsp
        self.nw = self.nW + 1
        if self.nsp:
            d = np.minimum(np.arange(self.ns, dtype=np.int64) * self.s, m - 1)
            if raw:
                c = ct[d // WG_TC]
                self.samples = np.sort(raw_key(np.where(c == -(2**31), tile.tid[d], c), tile.pos[d]))
            else:
                self.samples = np.sort(self.keys[d])
        else:
            self.samples = np.zeros(0, np.uint64)
        self.W, heavy_first = split_bounds(self.samples, self.g, self.nsp)
        # window of a record: the bounds that are <= its key (row r of the offsets matrix = first record with key >= W[r - 1])
        self.win = np.searchsorted(self.W, self.keys, side="right")
        self.count = np.bincount(self.win, minlength=self.nw)
        self.nw_live = int((self.count > 0).sum())
        # a window [v, v + 1) of a repeated splitter is a pile-up on one base: the only kind that may exceed the LDS sort
        self.heavy = np.zeros(self.nw, bool)                                              # (window 2 i + 1 lies between splitter i's two bounds)
        self.heavy[1::2] = heavy_first
        self.window_bound = 2 * WG_T + self.k * self.s                                    # a non-heavy window holds fewer records

    def pieces(self, w):
        """records of every file in window w"""
        return np.bincount(self.file[self.win == w], minlength=self.k)

    def groups_per_window(self, rec_group):
        """distinct groups of every window, from the oracle's record -> group map (passing records only)"""
        rg = np.asarray(rec_group)[self.rec].astype(np.int64)
        ok = self.mask[self.rec]
        pair = np.unique(self.win[ok].astype(np.int64) * (int(rg.max(initial=0)) + 2) + rg[ok])
        return np.bincount(pair // (int(rg.max(initial=0)) + 2), minlength=self.nw)

    def offsets_og(self, wg_og=0):
        """chunks per block of wg_offsets_stream_k (wg_offsets_build): eight where that leaves a few thousand blocks — one below
        2 * WG_OC * 2048 = 8.4 M records, so only the test hook wg_og reaches the carried state on a small tile"""
        return min(WG_OG, max(1, wg_og if wg_og else self.m // (WG_OC * 2048)))

    def offsets_branches(self, wg_og=0):
        """how wg_offsets_stream_k finds the bounds of every run segment (a run's records inside one chunk of WG_OC records): counts of
        'first' (the segment begins its run: searched from bound 0), 'run_end' (it continues the segment the block's chunk before ended
        with and ends the run: every bound that is left), 'probe' (it continues and spans fewer than 256 bounds: the probes fetched a
        chunk ahead), 'search' (it continues and spans 256 or more, or it lies in the first chunk of a block: the search over all
        of W, the key before it read from memory), and the largest span among the continued ones"""
        og = self.offsets_og(wg_og)
        fo = np.concatenate([[0], np.cumsum(np.bincount(self.file, minlength=self.k))])
        ub = lambda i: int(np.searchsorted(self.W, self.keys[i], side="right"))
        out = dict(first=0, run_end=0, probe=0, search=0, max_span=0)
        for f in range(self.k):
            a, b = int(fo[f]), int(fo[f + 1])
            i0 = a - a % WG_OC
            while i0 < b and a < b:
                sa, sb = max(a, i0), min(b, i0 + WG_OC)
                cont = (i0 // WG_OC) % og != 0
                if sa == a:
                    out["first"] += 1
                elif not cont:
                    out["search"] += 1
                elif sb == b:
                    out["run_end"] += 1
                else:
                    span = ub(sb - 1) - ub(sa - 1)
                    out["probe" if span < 256 else "search"] += 1
                    out["max_span"] = max(out["max_span"], span)
                i0 += WG_OC
        return out


def predict(tile, raw, rec_group, **opts):
    """what tbk_last_route reports for the window attempt of this form, and the route: dict(nw, nw_live, ovf1, ovf2, big_bucket,
    thr1, thr2, groups (per window), part (the Partition))"""
    P = Partition(tile, raw, **opts)
    thr1, thr2 = thresholds(P.k, raw)
    grp = P.groups_per_window(rec_group)
    live = P.count > 0
    o1 = live & (grp > thr1)
    o2 = o1 & (grp > thr2)
    big = o2 & (P.count > WG_CAP)
    return dict(nw=P.nw, nw_live=P.nw_live, ovf1=int(o1.sum()), ovf2=int((o2 & ~big).sum()), big_bucket=bool(big.any()), thr1=thr1, thr2=thr2,
                groups=grp, part=P)


def hashed_mask(tile):
    """records whose key word is a hash under the cigar strategy (record_key, strategy.hpp): everything but a single reference-consuming
    operation and the shape M N M with a first block < 2^10 and a gap < 2^20 — the records the verification pass compares"""
    off = tile.cig_off.astype(np.int64)
    nc = off[1:] - off[:-1]
    cig = np.concatenate([tile.cig.astype(np.int64), np.zeros(3, np.int64)])
    w0, w1, w2 = cig[off[:-1]], cig[off[:-1] + 1], cig[off[:-1] + 2]
    refop = ((0x18D >> (w0 & 15)) & 1) == 1
    one = (nc == 1) & refop
    mnm = (nc == 3) & ((w0 & 15) == 0) & ((w1 & 15) == 3) & ((w2 & 15) == 0) & ((w0 >> 4) < (1 << 10)) & ((w1 >> 4) < (1 << 20))
    return ~(one | mnm)
