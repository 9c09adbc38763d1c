"""Hand-built tiles that sit on the edges of the window path (tiebrush_amd/csrc/wgroup.hip): the thresholds of its two group tables
and of the LDS sort, its worklist loops, the shortcuts of its partition, the carries of its effective-end scan and its collision
checks.  tests/test_window_model_cpu.py proves with the CPU model (window_model.py) that every scene reaches the edge it is named
for; tests/test_gpu_window_edges.py runs them on the device against the oracle and the model's route.

A scene is built once per process (get) and so is the oracle's result for it (oracle)."""
import functools

import numpy as np

import window_model as wm
from tiebrush_amd import soa

M, I, D, N, S = 0, 1, 2, 3, 4
SNUM = {"cigar": 0, "full": 1, "clip": 2, "exon": 3}


def cw(*ops):
    return [(ln << 4) | op for ln, op in ops]


def mm(ln):
    return cw((ln, M))


# the pair of the collision scenes: equal start, end and exon count, only the inner exon differs — the key word is hashed, not exact
PAIR_A = cw((10, M), (20, N), (10, M), (30, N), (10, M))
PAIR_B = cw((10, M), (30, N), (10, M), (20, N), (10, M))


class Scene:
    def __init__(self, name, tile, opts=None, **edge):
        self.name, self.tile, self.opts, self.edge = name, tile, dict(opts or {}), edge

    def __repr__(self):
        return "Scene(%s: %d files, %d records)" % (self.name, self.tile.n_files, self.tile.n_records)


def F(tid, pos, shape, flag=0, mapq=60, strand="+", nh=1):
    """one file: arrays (or scalars, broadcast) in file order; `shape` indexes the scene's list of CIGARs"""
    n = max(np.size(x) for x in (tid, pos, shape, flag, mapq, nh))
    if any(np.ndim(x) and np.size(x) == 0 for x in (tid, pos, shape)):
        n = 0
    st = np.frombuffer(strand.encode(), np.uint8) if isinstance(strand, str) else np.asarray(strand, np.uint8)
    return dict(tid=np.broadcast_to(np.asarray(tid, np.int32), n), pos=np.broadcast_to(np.asarray(pos, np.int32), n),
                shape=np.broadcast_to(np.asarray(shape, np.int64), n), flag=np.broadcast_to(np.asarray(flag, np.uint16), n),
                mapq=np.broadcast_to(np.asarray(mapq, np.uint8), n), strand=np.broadcast_to(st, n), nh=np.broadcast_to(np.asarray(nh, np.int32), n))


EMPTY = F(np.zeros(0), np.zeros(0), np.zeros(0))


def tile_of(files, shapes):
    k = len(files)
    fo = np.zeros(k + 1, np.uint32)
    fo[1:] = np.cumsum([len(f["tid"]) for f in files])
    cat = {key: np.concatenate([f[key] for f in files]) if k else np.zeros(0) for key in ("tid", "pos", "shape", "flag", "mapq", "strand", "nh")}
    slen = np.array([len(s) for s in shapes], np.int64)
    soff = np.concatenate([[0], np.cumsum(slen)])
    flat = np.array([w for s in shapes for w in s], np.uint32)
    sh = cat["shape"].astype(np.int64)
    nc = slen[sh]
    off = np.concatenate([[0], np.cumsum(nc)])
    idx = np.repeat(soff[sh] - off[:-1], nc) + np.arange(int(off[-1]))
    return soa.SoATile(n_files=k, file_off=fo, tbmerged=np.zeros(k, np.uint8), tid=cat["tid"].astype(np.int32), pos=cat["pos"].astype(np.int32),
                       flag=cat["flag"].astype(np.uint16), mapq=cat["mapq"].astype(np.uint8), strand=cat["strand"].astype(np.uint8),
                       nh=cat["nh"].astype(np.int32), cig_off=off.astype(np.uint32), cig=flat[idx] if len(idx) else np.zeros(0, np.uint32))


def deal(k, tid, pos, shape, **kw):
    """records in coordinate order dealt round-robin to k files (every file stays sorted)"""
    pos = np.asarray(pos)
    tid, shape = (np.broadcast_to(np.asarray(x), len(pos)) for x in (tid, shape))
    kw = {key: np.asarray(v) for key, v in kw.items()}
    return [F(tid[f::k], pos[f::k], shape[f::k], **{key: (v[f::k] if v.ndim else v) for key, v in kw.items()}) if len(pos[f::k]) else EMPTY
            for f in range(k)]


SCENES = {}


def scene(name):
    def reg(fn):
        SCENES[name] = fn
        return fn
    return reg


@functools.lru_cache(maxsize=None)
def get(name):
    s = SCENES[name]()
    s.name = name
    return s


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle import oracle_ffi as orc
    s = get(name)
    kw = dict(s.opts)
    kw["strategy"] = SNUM[kw.get("strategy", "cigar")]
    return orc.collapse(s.tile, want_rec_group=True, **kw)


# ---- tiers, one window ------------------------------------------------------------------------------------------------------------
TIER_K = (1, 2, 32, 33, 64, 65, 1024)
EDGES = ("thr1", "thr1+1", "thr2", "thr2+1")
EDGE_ROUTE = {"thr1": (0, 0), "thr1+1": (1, 0), "thr2": (1, 0), "thr2+1": (1, 1)}      # (first-table overflows, second-table overflows)


def edge_groups(k, raw, edge):
    t1, t2 = wm.thresholds(k, raw)
    return {"thr1": t1, "thr1+1": t1 + 1, "thr2": t2, "thr2+1": t2 + 1}[edge]


def one_window(k, G):
    """at most 1024 records (one window for any k) in exactly G groups: G distinct starts, the records left over repeat some of them in
    other files (a group's sample bits span words where k > 32)"""
    n = min(1024, G + 37)
    pos = np.sort(np.concatenate([100 + 3 * np.arange(G), 100 + 3 * ((np.arange(n - G) * 29) % G)]))
    return tile_of(deal(k, 0, pos, 0), [mm(50)])


def _tier_scene(k, mode, edge):
    G = edge_groups(k, mode == "raw", edge)
    return Scene(None, one_window(k, G), mode=mode, groups=G, route=EDGE_ROUTE[edge])


TIER_SCENES = []
for _k in TIER_K:
    for _mode in ("raw", "compacted"):
        if _mode == "compacted" and wm.thresholds(_k, True) == wm.thresholds(_k, False):
            continue                                                     # (one set of thresholds: one set of scenes)
        for _e in EDGES:
            _n = "tier-k%d-%s-%s" % (_k, _mode, _e)
            SCENES[_n] = functools.partial(_tier_scene, _k, _mode, _e)
            TIER_SCENES.append(_n)


@scene("tier-k1025")
def _k1025():
    """one file more than the window path takes (tbk_window_supported): the sort path, whatever path= asks for"""
    return Scene(None, one_window(1025, 300), mode="raw", sort_path=True)


# ---- tiers, pile-up ---------------------------------------------------------------------------------------------------------------
def clip_shapes(n):
    """n distinct alignments of one start: soft clips of every length on both sides (hashed key words under the default strategy)"""
    out = []
    for a in range(40):
        for b in range(40):
            out.append(cw(*(([(a, S)] if a else []) + [(100 - a - b, M)] + ([(b, S)] if b else []))))
    assert n <= len(out)
    return out[:n]


def _pileup_scene(mode, edge):
    """one base, 3 files x 2100 records (a heavy window of more than WG_CAP records: the chunk loop runs), G distinct CIGARs whose members
    are spread over files and chunks; the first and the last record of the pile-up are in different groups; sparse records around it"""
    k, per = 3, 2100
    G = edge_groups(k, mode == "raw", edge)
    shapes = clip_shapes(G) + [mm(50)]
    files = []
    for f in range(k):
        i = np.arange(per) + f * per
        sh = (i * 7919 + (i // 512)) % G
        sh[:G // k + 1] = (np.arange(G // k + 1) * k + f) % G            # every shape occurs
        pre = np.arange(40) * 5 + f
        post = 9001 + np.arange(40) * 7 + f
        files.append(F(0, np.concatenate([pre, np.full(per, 5000), post]), np.concatenate([np.full(40, G), sh, np.full(40, G)])))
    big = edge == "thr2+1"
    return Scene(None, tile_of(files, shapes), mode=mode, groups=G, route=(EDGE_ROUTE[edge][0], 0 if big else EDGE_ROUTE[edge][1]), big_bucket=big)


PILEUP_SCENES = []
for _mode in ("raw", "compacted"):
    for _e in EDGES:
        _n = "pileup-%s-%s" % (_mode, _e)
        SCENES[_n] = functools.partial(_pileup_scene, _mode, _e)
        PILEUP_SCENES.append(_n)


# ---- the largest window the LDS sort takes ----------------------------------------------------------------------------------------
@scene("largest-sortable-window")
def _largest():
    """k = 64 (s = 32, g = 32).  File 0 lays 4000 records eight bases apart; every other file puts 31 records strictly between two of its
    own samples (its records 32 and 64; a sample is every 32nd record of the tile, and every file is a multiple of 32 long) into the stretch of file 0's records 1200 .. 1700, all keys unique.  Only file 0's samples
    fall there — 32 of them make one splitter — so the window between its two splitters (file 0's records 1088 .. 2111: 126 samples
    of the other files lie before file 0's first) holds 1024 records of file 0 and all 63 x 31 of the others.
    Achieved: 2977 records and 2977 groups in one window (bound: 2 * 1024 + 64 * 32 = 4096; thr2 = 936): six of the eight records per
    thread of wg_sort_k in use."""
    k = 64
    files = [F(0, 1_000_000 + 8 * np.arange(4000), 0)]
    for f in range(1, k):
        lo = 300_000 + 64 * np.arange(32) + f                            # records 0 .. 31 (sample: record 0)
        mid = 1_009_601 + 2 * ((f - 1) + 63 * np.arange(31))             # records 33 .. 63: odd bases, file 0's are even
        hi = 3_000_000 + 64 * np.arange(32) + f                          # record 64 (the next sample) and on: 96 records, three samples
        files.append(F(0, np.concatenate([lo, [900_000 + f], mid, hi]), 0))
    return Scene(None, tile_of(files, [mm(50)]), mode="raw", window=2977)


# ---- worklist loops ---------------------------------------------------------------------------------------------------------------
def _windows_k1(G_per_window, hashed_every=0):
    """k = 1: a splitter is every 1024th record; with unique boundary records the live windows are exactly 1024 records each.  Window w
    holds G_per_window[w] groups: that many distinct starts, the rest of its records on the last of them"""
    nwin = len(G_per_window)
    G = np.asarray(G_per_window, np.int64)
    j = np.tile(np.arange(1024), nwin)
    w = np.repeat(np.arange(nwin), 1024)
    pos = w * 2048 + np.minimum(j, G[w] - 1)
    shape = np.zeros(len(pos), np.int64)
    if hashed_every:                                                     # every other window: multi-exon reads (hashed key words) among them
        shape[(w % 2 == 1) & (j % hashed_every == 0)] = 1
    return tile_of([F(0, pos, shape)], [mm(50), PAIR_A])


@scene("worklist-tier2")
def _worklist2():
    """more than 512 windows on the second tier's worklist (its grid: 512 blocks), fitting and overflowing ones mixed at random, windows
    that fit the first table in between: 640 windows, 0.66 M records"""
    rng = np.random.default_rng(41)
    kind = rng.choice(3, 640, p=[0.12, 0.48, 0.40])
    return Scene(None, _windows_k1(np.array([300, 700, 1024])[kind]), mode="both", kinds=kind)


@scene("worklist-sort")
def _worklist_sort():
    """more than 1024 windows on the LDS sort's worklist (its grid: 1024 blocks): 1300 windows of 1024 distinct groups, every other one
    with multi-exon reads under the cigar strategy (the verification count of a block is non-zero in one window and zero in the next)"""
    return Scene(None, _windows_k1(np.full(1300, 1024), hashed_every=5), mode="both")


# ---- partition, raw ---------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385)


def _sorted_file(rng, n, ntid=3, span=60000, unplaced=0):
    tid = np.sort(rng.integers(0, ntid, n))
    pos = rng.integers(0, span, n)
    o = np.lexsort((pos, tid))
    f = F(tid[o], pos[o], rng.integers(0, 4, n), strand=rng.choice(np.frombuffer(b"+-", np.uint8), n))
    if unplaced:
        u = F(-1, -1, 4, flag=4, mapq=0, strand=".", nh=-(2**31))
        f = {key: np.concatenate([f[key], np.broadcast_to(u[key], unplaced)]) for key in f}
    return f


PART_SHAPES = [mm(50), mm(75), cw((20, M), (100, N), (30, M)), cw((5, S), (45, M)), []]


def _runs_scene(ln, lead):
    """runs of exactly `ln` records as first, middle and last file; empty and one-record files between them, before them (lead) and
    behind them"""
    rng = np.random.default_rng(ln)
    one = lambda: _sorted_file(rng, 1)
    files = ([EMPTY, one()] if lead else []) + [_sorted_file(rng, ln), EMPTY, one(), _sorted_file(rng, ln), one(), EMPTY, EMPTY, _sorted_file(rng, ln), EMPTY]
    return Scene(None, tile_of(files, PART_SHAPES), mode="raw", run=ln)


RUN_SCENES = []
for _ln in RUN_LENGTHS:
    for _lead in (0, 1):
        _n = "runs-%d%s" % (_ln, "-lead" if _lead else "")
        SCENES[_n] = functools.partial(_runs_scene, _ln, _lead)
        RUN_SCENES.append(_n)


@scene("tid-change-at-chunk-edges")
def _tid_edges():
    """the reference changes exactly at a 4096-record chunk edge, one record before it and one behind it (three files of 8192 records:
    the edge at record 4096, 4095 and 4097 of the file, the files themselves chunk-aligned); then a file that ends inside a chunk
    whose first and last records share a reference (the chunk must not get one id: the next file's records lie in it too)"""
    rng = np.random.default_rng(3)
    files = []
    for cut in (4096, 4095, 4097):
        tid = np.concatenate([np.zeros(cut), np.ones(8192 - cut)])
        pos = np.concatenate([np.sort(rng.integers(0, 50000, cut)), np.sort(rng.integers(0, 50000, 8192 - cut))])
        files.append(F(tid, pos, rng.integers(0, 4, 8192)))
    files.append(F(1, np.sort(rng.integers(0, 50000, 1000)), 0))        # ends inside chunk 6 ...
    files.append(F(np.concatenate([np.zeros(96), np.ones(3000)]), np.concatenate([np.sort(rng.integers(0, 50000, 96)),
                                                                                   np.sort(rng.integers(0, 50000, 3000))]), 1))  # ... which ends on tid 1 again
    return Scene(None, tile_of(files, PART_SHAPES), mode="raw")


@scene("400-files-of-5")
def _many_small():
    rng = np.random.default_rng(5)
    return Scene(None, tile_of([_sorted_file(rng, 5, ntid=2, span=3000) for _ in range(400)], PART_SHAPES), mode="raw")


def _dense_files(k):
    """k files of at least 4100 records over one coordinate range: a 2048-record chunk of one such run spans about half of the bounds
    (256 of 512 and more: the search over all of W); file 0 is three times as long and lies in a twentieth of the range, its chunks
    span a few bounds each (the 256 probes fetched ahead)"""
    rng = np.random.default_rng(k)
    files = [_sorted_file(rng, 12300, ntid=1, span=100_000)] + [_sorted_file(rng, 4100 + f % 3, ntid=1, span=2_000_000) for f in range(1, k)]
    return Scene(None, tile_of(files, PART_SHAPES), mode="raw")


SCENES["dense-64-files"] = functools.partial(_dense_files, 64)
SCENES["dense-96-files"] = functools.partial(_dense_files, 96)


@scene("unplaced-tail")
def _unplaced():
    """the unplaced reads (tid -1) behind every file's placed ones: a tail longer than a chunk, shorter ones, files without one"""
    rng = np.random.default_rng(8)
    files = [_sorted_file(rng, 3000, unplaced=u) for u in (5000, 0, 1, 2100, 0, 700)]
    return Scene(None, tile_of(files, PART_SHAPES), mode="raw")


@scene("extreme-coordinates")
def _extreme():
    """pos = 0, pos = 2^31 - 1 on the last reference (a secondary alignment without a CIGAR: a start past what a coordinate holds), a reference id
    whose tid << 31 needs the key's high word"""
    rng = np.random.default_rng(9)
    files = []
    for f in range(3):
        n = 1500
        tid = np.sort(rng.choice([0, 1, 3, 70000, 2_000_000], n))
        pos = rng.integers(0, 2**31 - 200, n)
        pos[:40] = 0
        o = np.lexsort((pos, tid))
        tid, pos = tid[o], pos[o]
        flag = np.zeros(n, np.uint16)
        pos[-1], flag[-1] = 2**31 - 1, 0x100
        pos[-2] = 2**31 - 60
        sh = rng.integers(0, 2, n)
        sh[-1], sh[-2] = 4, 0                                             # (50M from 2^31 - 60 ends below 2^31)
        files.append(F(tid, pos, sh, flag=flag))
    return Scene(None, tile_of(files, PART_SHAPES), mode="raw")


# ---- partition, both forms: pile-ups of more than 2 * 1024 records ----------------------------------------------------------------
def _piles(keys, k=2, filtered=None, sparse=400, empty_cigar=None):
    """pile-ups of 2600 records on each (tid, pos) of `keys`, sparse records around them on references 0 .. 2; pile `filtered` holds
    secondary alignments only (`empty_cigar`: without a CIGAR — on the last base a coordinate holds there is no room for one)"""
    rng = np.random.default_rng(len(keys) * 7 + k)
    files = []
    for f in range(k):
        t = [np.sort(rng.integers(0, 3, sparse))]
        p = [rng.integers(10, 90000, sparse)]
        fl = [np.zeros(sparse, np.uint16)]
        sh = [rng.integers(0, 4, sparse)]
        for q, (tid, pos) in enumerate(keys):
            t.append(np.full(2600 // k, tid))
            p.append(np.full(2600 // k, pos))
            fl.append(np.full(2600 // k, 0x100 if filtered == q else 0, np.uint16))
            sh.append(np.full(2600 // k, 4) if empty_cigar == q else rng.integers(0, 4, 2600 // k))
        t, p, fl, sh = np.concatenate(t), np.concatenate(p), np.concatenate(fl), np.concatenate(sh)
        o = np.lexsort((p, t))
        files.append(F(t[o], p[o], sh[o], flag=fl[o]))
    return tile_of(files, PART_SHAPES)


SCENES["piles-adjacent-bases"] = lambda: Scene(None, _piles([(1, 5000), (1, 5001)]), mode="both")
SCENES["piles-first-and-last-key"] = lambda: Scene(None, _piles([(0, 0), (2, 95000)]), mode="both")
SCENES["piles-across-references"] = lambda: Scene(None, _piles([(0, 2**31 - 1), (1, 0)], filtered=0, empty_cigar=0), mode="both")
SCENES["piles-one-record-between"] = lambda: Scene(None, _one_between(), mode="both")
SCENES["pile-all-filtered"] = lambda: Scene(None, _piles([(1, 5000), (1, 7000)], filtered=0), mode="both", filtered_pile=(1, 5000))
PILE_SCENES = ["piles-adjacent-bases", "piles-first-and-last-key", "piles-across-references", "piles-one-record-between", "pile-all-filtered"]


def _one_between():
    """two pile-ups separated by exactly one sparse record"""
    files = []
    for f in range(2):
        pos = np.concatenate([np.arange(50) * 3 + f, np.full(1300, 5000), [5001] if f == 0 else [], np.full(1300, 5002), 9000 + np.arange(50) * 3 + f])
        files.append(F(1, pos, (np.arange(len(pos)) * 3 + f) % 4))
    return tile_of(files, PART_SHAPES)


# ---- effective ends ---------------------------------------------------------------------------------------------------------------
EFF_SETTERS = (63, 511, 2047, 2499)      # file 0: last lane of a wave, last record of a 512-record chunk (raw kernel), of the 2048-record
EFF_LEN0 = 2500                          # chunk (compacted kernel), of the file's piece


def effective_ends(perturb=None):
    """One base — tid 0, pos 0, the first key there is: the one key whose records the key before a file's first record (none: 0) does not
    set apart, so only the piece boundary itself keeps file 1's first record out of file 0's run —, one heavy window, three files.  File 0's ends rise and fall below 90; at the records EFF_SETTERS the running maximum is
    set anew (200, 220 — by a secondary alignment, which raises it without a group —, 240, 260).  The record behind each of the
    first three is a 31M / 32M / 33M read: it inherits the maximum, so its group's representative is the member in file 1 whose
    effective end (190, 210, 230) lies between the old maximum and the new one.  The last setter ends file 0's piece: file 1's
    first record (34M, same start) must NOT inherit 260 — it is its group's representative with effective end 34, ahead of file 2's
    member (60).  An unmapped mate inside the run contributes no end.
    perturb = ("lower", j): setter j's end is 20 (no maximum: the record behind it becomes the representative);
    perturb = "join": files 0 and 1 are one file (file 1's first record inherits)."""
    shapes = [mm(x) for x in range(20, 270)] + [[]]
    sh = lambda ln: ln - 20
    UNM = len(shapes) - 1
    i = np.arange(EFF_LEN0)
    s0 = sh(40 + (i * 37) % 50)
    fl0 = np.zeros(EFF_LEN0, np.uint16)
    for j, (at, top) in enumerate(zip(EFF_SETTERS, (200, 220, 240, 260))):
        s0[at] = sh(20 if perturb == ("lower", j) else top)
        if j < 3:
            s0[at + 1] = sh(31 + j)
    fl0[511] = 0x100
    s0[1000], fl0[1000] = UNM, 4 | 8                                      # unmapped mate at its mate's position
    f0 = F(0, 0, s0, flag=fl0)
    s1 = np.concatenate([[sh(34), sh(190), sh(31), sh(210), sh(32), sh(230), sh(33)], sh(40 + (np.arange(300) * 11) % 50)])
    f1 = F(0, 0, s1)
    s2 = np.concatenate([[sh(50), sh(60), sh(34)], sh(40 + (np.arange(300) * 13) % 50)])
    f2 = F(0, 0, s2)
    if perturb == "join":
        return tile_of([{key: np.concatenate([f0[key], f1[key]]) for key in f0}, EMPTY, f2], shapes)
    return tile_of([f0, f1, f2], shapes)


SCENES["effective-ends"] = lambda: Scene(None, effective_ends(), mode="both")


def rep_of(tile, res, shape_len, pos=0):
    """the representative of the group of `shape_len`M reads at `pos` in a result"""
    gs, ge = np.asarray(res["g_start"]), np.asarray(res["g_end"])
    hit = np.flatnonzero((gs == pos + 1) & (ge == pos + shape_len))
    assert len(hit) == 1
    return int(np.asarray(res["rep"])[hit[0]])


# ---- hidden inversions ------------------------------------------------------------------------------------------------------------
def hidden_tid_inversion(filtered):
    """inside one 4096-record chunk of one file the records run tid 0 ... tid 1 ... tid 0: the chunk's ends agree, so the partition takes
    every record of it for tid 0; the one tid-1 record passes (TBK_EUNSORTED), or it and everything behind it in the file are secondary
    alignments (no error: the merge order is fixed on what passes and what came before it)"""
    n = 4096
    tid = np.zeros(n, np.int32)
    tid[2000] = 1
    pos = np.sort(np.random.default_rng(1).integers(0, 50000, n))
    fl = np.zeros(n, np.uint16)
    fl[2000:] = 0x100 if filtered else 0
    other = F(0, np.sort(np.random.default_rng(2).integers(0, 50000, 3000)), 1)
    return tile_of([F(tid, pos, 0, flag=fl), other], PART_SHAPES)


def pos_inversion(at, filtered, n=40000):
    """record `at` of one file lies before record at - 1 (a position inversion across a chunk edge of the offsets pass)"""
    pos = np.sort(np.random.default_rng(at).integers(1000, 500000, n))
    pos[at] = pos[at - 1] - 500
    fl = np.zeros(n, np.uint16)
    fl[at] = 0x100 if filtered else 0
    other = F(0, np.sort(np.random.default_rng(2).integers(0, 500000, 3000)), 1)
    return tile_of([F(0, pos, 0, flag=fl), other], PART_SHAPES)


# ---- collisions -------------------------------------------------------------------------------------------------------------------
def _with_pair(n_fill, k=2, pair_files=(0, 1), pile=0, dup=1):
    """n_fill filler groups of `dup` records each (distinct starts, exact key words) and the pair PAIR_A / PAIR_B on one start in files
    pair_files; pile > 0: that many filler records on the pair's start between its two members"""
    shapes = [mm(50), PAIR_A, PAIR_B]
    pos = np.repeat(100 + 3 * np.arange(n_fill), dup)
    files = deal(k, 0, pos, 0)
    at = 100 + 3 * (n_fill // 2) + 1
    out = []
    for f in range(k):
        extra_pos, extra_shape = [], []
        if f == pair_files[0]:
            extra_pos.append(at), extra_shape.append(1)
        if pile:
            extra_pos += [at] * (pile // k + 1)
            extra_shape += [0] * (pile // k + 1)
        if f == pair_files[1]:
            extra_pos.append(at), extra_shape.append(2)
        p = np.concatenate([files[f]["pos"], np.array(extra_pos, np.int64)])
        s = np.concatenate([files[f]["shape"], np.array(extra_shape, np.int64)])
        o = np.argsort(p, kind="stable")
        out.append(F(0, p[o], s[o]))
    return tile_of(out, shapes)


COLLISION_SCENES = {
    "collision-tier1": lambda: _with_pair(300),
    "collision-tier1-one-file": lambda: _with_pair(300, pair_files=(1, 1)),
    "collision-tier2": lambda: _with_pair(700),
    "collision-lds-sort": lambda: _with_pair(1022),
    "collision-pileup": lambda: _with_pair(300, pile=4300),
    "collision-only-hashed-of-their-window": lambda: _with_pair(2000, dup=4),
}
for _n, _fn in COLLISION_SCENES.items():
    SCENES[_n] = functools.partial(lambda fn: Scene(None, fn(), mode="both", collision=True), _fn)


def many_hashed_reads(seed, n=3000):
    """a few thousand three-exon reads on few starts whose inner exons vary: hashed key words, many true repeats"""
    rng = np.random.default_rng(seed)
    shapes = [cw((10, M), (20 + a, N), (10, M), (50 - a, N), (10, M)) for a in range(31)]
    files = []
    for f in range(3):
        pos = np.sort(rng.integers(0, 40, n // 3)) * 50
        files.append(F(0, pos, rng.integers(0, len(shapes), n // 3)))
    return tile_of(files, shapes)
