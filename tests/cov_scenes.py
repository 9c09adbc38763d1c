"""Hand-placed reads for the coverage kernels (tiebrush_amd/csrc/cov.hip): scene builders, the layout the kernels cut their work by,
and a plain per-base model of tiecov.  numpy only; importable without a GPU.

The kernels lay the bundles end to end in a compacted coordinate space and cut it into tiles of W = 8192 bases; the bundle passes
walk the records in blocks of 4096 (a thread four records, a wave 256, a row 1024), the junction sums in blocks of 4096 records with a
table of 1024 slots, the junction homes in blocks of 1024 records.  A scene puts one thing on one of these edges and says so in its
`claims`: facts about the input, checked on the CPU through layout() / model(), that make the scene what its name says
(tests/test_cov_scenes_cpu.py).  tests/test_gpu_cov_edges.py then runs every scene through every chain of the library.

Placing: a spacer of L bases in front (bundles of their own that fill whole tiles and never leave them: no spill piece comes from a
spacer) shifts everything behind it by exactly L compacted bases, so a feature sits at compacted offset k W + d by construction.

model() is written from the comment block at the head of cov.hip and from SURVEY.md (B.4), one bundle at a time on dense arrays; it
shares no code with oracle/tb_oracle.c, and the two must agree before the GPU is asked."""
import functools

import numpy as np

from tiebrush_amd import soa

M, I, D, N, S = 0, 1, 2, 3, 4
W = 8192                 # COV_W: compacted bases per tile
SW = 64                  # COV_SW: LDS window of the spill counting sorts, in tiles
CB_TILE = 4096           # records per block of the bundle passes
IV_TILE = 2048           # change points per block of iv_count_k / iv_emit_k
JA_REC, JA_SLOTS = 4096, 1024
JH_REC = 1024
TOP = 2**31 - 1          # the last base a BAM position can name (1-based)


# ---- input ---------------------------------------------------------------------------------------------------------------------------
def mk(recs, yx=None):
    """(tid, pos, flag, [(len, op) ...], yc, strand) tuples -> soa.CovInput"""
    tid = np.array([r[0] for r in recs], np.int32)
    pos = np.array([r[1] for r in recs], np.int32)
    flag = np.array([r[2] for r in recs], np.uint16)
    cigs = [[(l << 4) | o for l, o in r[3]] for r in recs]
    off = np.zeros(len(recs) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in cigs])
    cig = np.array([x for c in cigs for x in c], np.uint32)
    yc = np.array([r[4] for r in recs], np.float64)
    st = np.array([ord(r[5]) for r in recs], np.uint8)
    return soa.CovInput(tid, pos, flag, off, cig, yc, st, None if yx is None else np.asarray(yx, np.int64))


def records(cin):
    """the tuples mk() takes, back from a CovInput"""
    out = []
    for i in range(cin.n_records):
        c = cin.cig[int(cin.cig_off[i]):int(cin.cig_off[i + 1])]
        out.append((int(cin.tid[i]), int(cin.pos[i]), int(cin.flag[i]), [(int(x) >> 4, int(x) & 15) for x in c], float(cin.yc[i]),
                    chr(int(cin.strand[i]))))
    return out


def with_unmapped(cin, every=7):
    """the same input with an unmapped record (flag 4, a CIGAR and a YC of its own) behind every `every`-th record and one in front:
    the compaction of the mapped records is then no identity"""
    recs, out, yx = records(cin), [], []
    for i, r in enumerate(recs):
        if i % every == 0:
            out.append((r[0], r[1], 4, [(33, M), (70, N), (5, M)], 9.0, "+"))
            yx.append(5)
        out.append(r)
        yx.append(1 if cin.yx is None else int(cin.yx[i]))
    return mk(out, None if cin.yx is None else yx)


def mapped_only(cin):
    """the mapped records alone, flag = None: what the device chain hands over (every record counts, no compaction)"""
    keep = (np.asarray(cin.flag) & 4) == 0
    recs = [r for r, k in zip(records(cin), keep) if k]
    c = mk(recs, None if cin.yx is None else np.asarray(cin.yx)[keep])
    c.flag = None
    return c


def sample_yx(n, ns):
    """YX for the sample track: 1 + (7 i mod ns), and one value that is present and 0"""
    yx = 1 + (7 * np.arange(n, dtype=np.int64)) % ns
    if n:
        yx[n // 2] = 0
    return yx


def with_yc(cin, f):
    c = mk(records(cin), cin.yx)
    c.yc = f(c.yc)
    return c


# ---- layout --------------------------------------------------------------------------------------------------------------------------
def _ops(cin, i):
    c = cin.cig[int(cin.cig_off[i]):int(cin.cig_off[i + 1])]
    return [(int(x) >> 4, int(x) & 15) for x in c]


def layout(cin):
    """every mapped record's bundle, head flag and compacted start; the bundle table; S (compacted bases) and ntiles.
    Bundle rule (tiecov): a new bundle iff the reference changes or start > running max(end); span = b_end - b_start + 1 (0 for a
    bundle of one record that holds only S / I)."""
    idx = [i for i in range(cin.n_records) if not (int(cin.flag[i]) & 4)] if cin.flag is not None else list(range(cin.n_records))
    oplen = (np.asarray(cin.cig) >> 4).astype(np.int64)
    opc = np.asarray(cin.cig) & 15
    per = np.zeros(cin.n_records, np.int64)
    rec_of = np.repeat(np.arange(cin.n_records), np.diff(np.asarray(cin.cig_off).astype(np.int64)))
    np.add.at(per, rec_of, np.where((opc == M) | (opc == D) | (opc == N), oplen, 0))
    start = np.asarray(cin.pos).astype(np.int64)[idx] + 1
    end = start - 1 + per[idx]
    tid = np.asarray(cin.tid).astype(np.int64)[idx]
    m = len(idx)
    bundle, head = np.zeros(m, np.int64), np.zeros(m, bool)
    b_tid, b_start, b_end = [], [], []
    for j in range(m):
        if j == 0 or tid[j] != b_tid[-1] or start[j] > b_end[-1]:
            b_tid.append(int(tid[j])), b_start.append(int(start[j])), b_end.append(int(end[j]))
            head[j] = True
        elif end[j] > b_end[-1]:
            b_end[-1] = int(end[j])
        bundle[j] = len(b_tid) - 1
    b_tid, b_start, b_end = (np.array(a, np.int64) for a in (b_tid, b_start, b_end))
    span = b_end - b_start + 1 if m else np.zeros(0, np.int64)
    b_off = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    cs = b_off[bundle] + start - b_start[bundle] if m else np.zeros(0, np.int64)
    total = int(b_off[-1])
    return dict(idx=np.array(idx, np.int64), start=start, end=end, tid=tid, bundle=bundle, head=head, cs=cs, b_tid=b_tid, b_start=b_start,
                b_end=b_end, b_off=b_off, span=span, S=total, ntiles=-(-total // W))


def segments(cin, lay, j):
    """the operations of mapped record j that take reference bases, in compacted coordinates: [(op, first, end)) ...]"""
    p, out = int(lay["cs"][j]), []
    for ln, op in _ops(cin, int(lay["idx"][j])):
        if op in (M, D, N):
            out.append((op, p, p + ln))
            p += ln
    return out


def pieces(cin, lay, j):
    """the M bases of mapped record j cut at the tile seams: [(tile, offset in the tile, length) ...]"""
    out = []
    for op, a, b in segments(cin, lay, j):
        while op == M and a < b:
            e = min(b, (a // W + 1) * W)
            out.append((a // W, a % W, e - a))
            a = e
    return out


def spill_pieces(cin, lay, j):
    """the pieces that do not lie in the record's home tile (the tile of its compacted start)"""
    home = int(lay["cs"][j]) // W
    return [p for p in pieces(cin, lay, j) if p[0] != home]


def is_spilling(lay, j):
    """a record the kernels walk for spill pieces: its reference span reaches beyond its home tile (pieces or not)"""
    return int(lay["cs"][j]) % W + int(lay["end"][j] - lay["start"][j] + 1) > W


def tile_homes(lay, t):
    """the mapped records whose compacted start lies in tile t"""
    return np.flatnonzero(lay["cs"] // W == t)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def exons(pos, ops):
    """1-based inclusive exons of an alignment: M and D extend the current exon, N closes it and opens the next — except an N that follows
    an insertion which itself followed an N —, S and I take no reference base.  The last exon is closed at the end, empty or not."""
    out, ln, first, after_n, after_i = [], 0, pos, False, False
    for n, op in ops:
        if op == N and not (after_n and after_i):
            out.append((first + 1, pos + ln))
        if op in (M, D, N):
            ln += n
        if op == N:
            first, after_n = pos + ln, True
        elif op in (M, D, S):
            after_n = after_i = False
        elif op == I:
            after_i = True
    out.append((first + 1, pos + ln))
    return out


def _rle(v):
    n = len(v)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a = np.concatenate([[0], np.flatnonzero(v[1:] != v[:-1]) + 1])
    b = np.concatenate([a[1:], [n]])
    keep = v[a] != 0
    return a[keep], b[keep]


def model(cin, num_samples=0):
    """tiecov, per base: the oracle's keys.  Depth: YC added per M base in record order in float64; rows: run-length encoding on exact
    equality, zero runs skipped, never across a bundle; junctions: summed per bundle in record order, sorted by (start, end, strand
    char); sample track: float32 running mean of YX per base in record order, mean += (val - mean) / cnt from (0, 1), ceil on output."""
    lay = layout(cin)
    f32 = np.float32
    iv = [[], [], [], []]
    jn = [[], [], [], [], []]
    sm = [[], [], [], [], []]
    n_bases = 0
    m = len(lay["idx"])
    j = 0
    for b in range(len(lay["b_tid"])):
        b0, span, tid = int(lay["b_start"][b]), int(lay["span"][b]), int(lay["b_tid"][b])
        depth = np.zeros(span, np.float64)
        mean, cnt = np.zeros(span, f32), np.ones(span, np.uint64)
        juncs = {}
        while j < m and lay["bundle"][j] == b:
            i = int(lay["idx"][j])
            ops = _ops(cin, i)
            yc = float(cin.yc[i]) if cin.yc is not None else 1.0
            val = f32(int(f32(int(cin.yx[i])))) if cin.yx is not None else f32(1)
            p = int(cin.pos[i]) + 1 - b0
            for ln, op in ops:
                if op == M:
                    depth[p:p + ln] += yc
                    n_bases += ln
                    if num_samples > 0:
                        mean[p:p + ln] += (val - mean[p:p + ln]) / cnt[p:p + ln].astype(f32)
                        cnt[p:p + ln] += np.uint64(1)
                if op in (M, D, N):
                    p += ln
            ex = exons(int(cin.pos[i]), ops)
            st = int(cin.strand[i]) if cin.strand is not None else ord(".")
            for (_, e0), (s1, _) in zip(ex[:-1], ex[1:]):
                key = (e0 + 1, s1 - 1, st)
                juncs[key] = juncs[key] + yc if key in juncs else yc
            j += 1
        a, e = _rle(depth)
        iv[0].append(np.full(len(a), tid)), iv[1].append(b0 - 1 + a), iv[2].append(b0 - 1 + e), iv[3].append(depth[a])
        for key in sorted(juncs):
            for q, v in enumerate((tid, key[0] - 1, key[1], key[2], juncs[key])):
                jn[q].append(v)
        if num_samples > 0:
            c = np.ceil(mean).astype(np.uint64)
            heat = (c.astype(f32) / f32(num_samples)) * (f32(1.5) - f32(0.1)) + f32(0.1)
            a, e = _rle(c)
            sm[0].append(np.full(len(a), tid)), sm[1].append(b0 - 1 + a), sm[2].append(b0 - 1 + e), sm[3].append(c[a]), sm[4].append(heat[a])

    def cat(parts, dt):
        return np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)

    res = dict(n_intervals=sum(len(x) for x in iv[0]), iv_tid=cat(iv[0], np.int32), iv_start=cat(iv[1], np.int32), iv_end=cat(iv[2], np.int32),
               iv_val=cat(iv[3], np.float64), n_junctions=len(jn[0]), j_tid=np.array(jn[0], np.int32), j_start=np.array(jn[1], np.int32),
               j_end=np.array(jn[2], np.int32), j_strand=np.array(jn[3], np.uint8), j_val=np.array(jn[4], np.float64),
               n_sample=sum(len(x) for x in sm[0]), s_tid=cat(sm[0], np.int32), s_start=cat(sm[1], np.int32), s_end=cat(sm[2], np.int32),
               s_count=cat(sm[3], np.int64), s_heat=cat(sm[4], np.float32), n_bases=n_bases, span_bases=lay["S"])
    return res


def depth_at(cin, lay, c):
    """integral depth of compacted base c (sum of YC over the M segments that cover it)"""
    d = 0.0
    for j in range(len(lay["idx"])):
        for op, a, b in segments(cin, lay, j):
            if op == M and a <= c < b:
                d += float(cin.yc[int(lay["idx"][j])])
    return d


def junction_items(cin, lay):
    """what reaches the junction homes on the default route: one item per distinct (reference, start, end, strand) and block of JA_REC
    records -> {home block (of JH_REC records): number of items}.  The home of an item is the last block whose first record starts at
    or before the junction's first base, in (reference, start) order."""
    seen = set()
    for j in range(len(lay["idx"])):
        i = int(lay["idx"][j])
        ex = exons(int(cin.pos[i]), _ops(cin, i))
        for (_, e0), (s1, _) in zip(ex[:-1], ex[1:]):
            seen.add((j // JA_REC, int(cin.tid[i]), e0 + 1, s1 - 1, int(cin.strand[i])))
    nblk = -(-len(lay["idx"]) // JH_REC)
    bkey = [(int(lay["tid"][q * JH_REC]), int(lay["start"][q * JH_REC])) for q in range(nblk)]
    homes = {}
    for _, tid, js, _, _ in seen:
        h = 0
        for q in range(nblk):
            if bkey[q] <= (tid, js):
                h = q
        homes[h] = homes.get(h, 0) + 1
    return homes


# ---- building blocks -------------------------------------------------------------------------------------------------------------------
F_TID, F_POS = 1, 1000     # where a scene's feature bundle starts: reference 1, behind the spacer's reference 0


def spacer(L):
    """L compacted bases in front of everything else: reads on reference 0 that abut (start == end + 1: every one a bundle of its own),
    each inside one tile — no piece leaves its home tile"""
    out, p = [], 0
    while p < L:
        n = min(W, L - p)
        out.append((0, p, 0, [(n, M)], 1.0, "."))
        p += n
    return out


def _feature(off, before, recs):
    """`recs` (positions relative to the feature bundle's first base) behind a spacer of off - before bases: the bundle's base
    `before` then sits at compacted offset off"""
    assert off - before >= 0
    return spacer(off - before) + [(F_TID, F_POS + r[0]) + tuple(r[1:]) for r in recs]


def _first_feature(cin, lay):
    return int(np.flatnonzero(lay["tid"] == F_TID)[0])


SWEEP_D = (-1, 0, 1)      # (-2 .. 2 at first: thinned to the seam and its two neighbours for the GPU file's time)
SWEEP_K = (1, 2)


# ---- tile scenes: (cin, claims) ----------------------------------------------------------------------------------------------------------
def t1(k, d):
    """a read starts at the offset as a bundle head (d = 0: the tile's first change point is a head, not tentative)"""
    off = k * W + d
    cin = mk(_feature(off, 0, [(0, 0, [(50, M)], 3.0, "."), (10, 0, [(30, M)], 2.0, ".")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    return cin, {"offset": int(lay["cs"][j]), "want_offset": off, "is_head": bool(lay["head"][j])}


def t2(k, d):
    """a read's last base is at the offset: on the tile's last base no spill, one base further a spill piece of length 1"""
    off = k * W + d
    cin = mk(_feature(off, 99, [(0, 0, [(100, M)], 2.0, "."), (5, 0, [(20, M)], 1.0, ".")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    sp = spill_pieces(cin, lay, j)
    want = [] if off % W >= 99 else [(off // W, 0, off % W + 1)]
    return cin, {"offset": int(lay["cs"][j]) + 99, "want_offset": off, "spill": sp, "want_spill": want, "spilling": is_spilling(lay, j),
                 "want_spilling": bool(want)}


def t3(k, d, second):
    """one read covers the seam at constant depth: one row, the tentative change point is dropped; with a second read starting at the
    offset the depth changes there and the point (tentative at d = 0) is kept"""
    off = k * W + d
    recs = [(0, 0, [(200, M)], 2.0, ".")] + ([(100, 0, [(50, M)], 1.0, ".")] if second else [])
    cin = mk(_feature(off, 100, recs))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    rows = model(cin)
    nrows = int(np.sum(rows["iv_tid"] == F_TID))
    c = {"offset": int(lay["cs"][j]) + 100, "want_offset": off, "rows": nrows, "want_rows": 3 if second else 1,
         "covers": int(lay["cs"][j]) < k * W - 2 and int(lay["cs"][j]) + 200 > k * W + 2}
    if second:
        c["second_is_head"] = bool(lay["head"][j + 1])
        c["want_second_is_head"] = False
        c["offset"] = int(lay["cs"][j + 1])
    return cin, c


def t4(k, d, edge):
    """the depth falls to 0 at the offset inside a bundle (an intron opens there), or rises again there (the intron's last base is
    offset - 1)"""
    off = k * W + d
    before = 60 if edge == "fall" else 560
    cin = mk(_feature(off, before, [(0, 0, [(60, M), (500, N), (40, M)], 2.0, "+"), (0, 0, [(60, M), (500, N), (40, M)], 1.0, "+"),
                                    (20, 0, [(30, M)], 1.0, ".")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    seg = segments(cin, lay, j)
    edge_at = seg[1][1] if edge == "fall" else seg[1][2]
    return cin, {"offset": edge_at, "want_offset": off, "depths": (depth_at(cin, lay, off - 1), depth_at(cin, lay, off)),
                 "want_depths": (3.0, 0.0) if edge == "fall" else (0.0, 3.0), "one_bundle": int(len(set(lay["bundle"][j:]))), "want_one_bundle": 1}


def t5(k, d, far):
    """a bundle ends with depth 2 on base offset - 1 and the next begins with depth 2 on the offset (adjacent reference coordinates,
    or far apart): two rows, never one"""
    off = k * W + d
    cin = mk(_feature(off, 40, [(0, 0, [(40, M)], 2.0, "."), (5040 if far else 40, 0, [(40, M)], 2.0, ".")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    rows = model(cin)
    return cin, {"offset": int(lay["cs"][j + 1]), "want_offset": off, "is_head": bool(lay["head"][j + 1]),
                 "adjacent": int(lay["start"][j + 1] - lay["end"][j]) == 1, "want_adjacent": not far,
                 "depths": (depth_at(cin, lay, off - 1), depth_at(cin, lay, off)), "want_depths": (2.0, 2.0),
                 "rows": int(np.sum(rows["iv_tid"] == F_TID)), "want_rows": 2}


def t6(k, d):
    """(3 W + 7) M from the offset: whole tiles that hold a tentative change point and nothing else (the lean writer's forward search
    runs over two tiles and more); starting on a seam, full-tile spill pieces (offset 0, length 8192)"""
    off = k * W + d
    cin = mk(_feature(off, 0, [(0, 0, [(3 * W + 7, M)], 3.0, ".")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    sp = spill_pieces(cin, lay, j)
    full = [p for p in sp if p[1] == 0 and p[2] == W]
    return cin, {"offset": int(lay["cs"][j]), "want_offset": off, "full_tile_pieces": len(full), "want_full_tile_pieces": 3 if d < 0 else 2, "home_tile_piece_is_full": (d == 0) == (off % W == 0),
                 "rows": int(np.sum(model(cin)["iv_tid"] == F_TID)), "want_rows": 1}


def t7(k, d, dp):
    """10M (2 W + dp)N 10M from the offset and nothing else there: whole tiles at depth 0 inside a bundle, without a home record"""
    off = k * W + d
    cin = mk(_feature(off, 0, [(0, 0, [(10, M), (2 * W + dp, N), (10, M)], 4.0, "-")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    t = (off + 10) // W + 1   # the tile behind the one the first exon ends in
    return cin, {"offset": int(lay["cs"][j]), "want_offset": off, "empty_tile_homes": len(tile_homes(lay, t)), "want_empty_tile_homes": 0,
                 "empty_tile_depth": max(depth_at(cin, lay, t * W), depth_at(cin, lay, t * W + W - 1)), "want_empty_tile_depth": 0.0,
                 "empty_tile_in_bundle": int(lay["b_off"][lay["bundle"][j]]) < t * W and int(lay["b_off"][lay["bundle"][j] + 1]) >= (t + 1) * W}


def t8(window, behind, straddle=False):
    """10M xN 10M whose second exon lands in tile tbase + window of its block (window 63: the last tile of the LDS window; 64, 65:
    beyond it, the global counters).  behind = False: the read is the input's first record, tbase its home tile; True: a few short
    reads in the tile before it come first, so tbase is not its home.  straddle: the second exon lies across the seam into that tile"""
    pre = [(0, 100 + 3 * q, 0, [(20, M)], 1.0, ".") for q in range(5)] + [(0, 120, 0, [(W + 80, M)], 1.0, ".")] if behind else []
    # (behind: reference 0 holds one bundle of W + 100 bases — 1-based 101 .. W + 200 —, its first record's home tile 0, the feature's tile 1)
    start = W + 100 if behind else 0
    target = window * W + (-3 if straddle else 5)      # compacted start of the second exon (tbase = 0)
    x = target - start - 10
    cin = mk(pre + [(F_TID, F_POS, 0, [(10, M), (x, N), (10, M)], 2.0, "+"), (F_TID, F_POS + 2, 0, [(5, M)], 1.0, ".")])
    lay = layout(cin)
    j = _first_feature(cin, lay)
    return cin, {"tbase": int(lay["cs"][0]) // W, "want_tbase": 0, "home": int(lay["cs"][j]) // W, "want_home": 1 if behind else 0,
                 "spill_tiles": [p[0] for p in spill_pieces(cin, lay, j)], "want_spill_tiles": [window - 1, window] if straddle else [window]}


def t9(k, d):
    """two reads M D M I M N M S in one bundle; with d = 0: an M longer than a tile cut into three pieces, the second beginning on a
    seam; an M that ends on a tile's last base with a D behind it; a D that begins in the home tile and ends in the next"""
    off = k * W + d
    r1 = [(100, M), (30, D), (2 * W + 20, M), (2, I), (20, M), (300, N), (40, M), (5, S)]
    r2 = [(50, M), (20, D), (30, M), (3, I), (10, M), (100, N), (10, M), (2, S)]
    cin = mk(_feature(off, 100, [(0, 0, r1, 2.0, "+"), (40, 0, r2, 1.0, "-")]))
    lay = layout(cin)
    j = _first_feature(cin, lay)
    s1, s2 = segments(cin, lay, j), segments(cin, lay, j + 1)
    long_m = [p for p in pieces(cin, lay, j) if p[0] in (off // W, off // W + 1, off // W + 2)]
    return cin, {"offset": s1[0][2], "want_offset": off,                              # the first M ends on base offset - 1
                 "d_behind_it": s1[1][0] == D and s1[1][1] == off,
                 "long_m_pieces": len([p for p in pieces(cin, lay, j) if (p[0] * W + p[1]) >= s1[2][1] and (p[0] * W + p[1]) < s1[2][2]]),
                 "want_long_m_pieces": 3, "piece_on_seam": any(p[1] == 0 and p[0] * W > s1[2][1] for p in long_m),
                 "d_across": (s2[1][0] == D, s2[1][1], s2[1][2]), "want_d_across": (True, off - 10, off + 10)}


def t10(k, d, place):
    """a read that ends in D across the seam — a spilling record without a piece, its bundle's end extended by bases nothing covers —
    and a record of only S / I (reference span 0) that starts at the offset: the input's first record, its last, or in between"""
    off = k * W + d
    empty = [(5, S), (3, I), (4, S)]
    if place == "first":      # the empty record opens the input: a bundle of span 0 at compacted 0, then the rest
        recs = [(0, 0, 0, empty, 5.0, ".")] + _feature(off, 50, [(0, 0, [(40, M), (20, D)], 2.0, "."), (70, 0, [(30, M)], 1.0, ".")])
    elif place == "last":     # ... closes it, behind the last covered base: a bundle of span 0 at compacted S
        recs = _feature(off, 50, [(0, 0, [(40, M), (20, D)], 2.0, "."), (60, 0, empty, 5.0, ".")])
    elif place == "inside":   # ... starts at the offset, under the D of the read before it: no bundle of its own
        recs = _feature(off, 50, [(0, 0, [(40, M), (20, D)], 2.0, "."), (50, 0, empty, 5.0, "."), (55, 0, [(30, M)], 1.0, ".")])
    else:                     # "between": a bundle of span 0 at the offset between two bundles
        recs = _feature(off, 60, [(0, 0, [(40, M), (20, D)], 2.0, "."), (60, 0, empty, 5.0, "."), (60, 0, [(30, M)], 1.0, ".")])
    cin = mk(recs)
    lay = layout(cin)
    j = _first_feature(cin, lay)
    e = int(np.flatnonzero(lay["end"] < lay["start"])[0])
    c = {"d_read_pieces": spill_pieces(cin, lay, j), "want_d_read_pieces": [], "empty_span": int(lay["end"][e] - lay["start"][e] + 1),
         "want_empty_span": 0, "empty_is_head": bool(lay["head"][e]), "want_empty_is_head": place != "inside",
         "bundle_end": int(lay["b_end"][lay["bundle"][j]] - lay["start"][j]) + 1, "want_bundle_end": 60 if place != "inside" else 85}
    if place != "inside":     # (inside: a later read lies under the D)
        c.update(bundle_end_uncovered=depth_at(cin, lay, int(lay["cs"][j]) + 59), want_bundle_end_uncovered=0.0)
    if place != "between":     # the D of the first read lies across the offset: off - 10 .. off + 9
        c.update(d_read_spilling=is_spilling(lay, j), want_d_read_spilling=(off - 10) // W != (off + 9) // W)
    if place == "first":
        c.update(offset=int(lay["cs"][j]) + 50, want_offset=off, empty_at=int(lay["cs"][e]), want_empty_at=0, empty_record=e, want_empty_record=0)
    elif place == "last":
        c.update(offset=int(lay["cs"][j]) + 50, want_offset=off, empty_at=int(lay["cs"][e]), want_empty_at=lay["S"], empty_record=e,
                 want_empty_record=len(lay["idx"]) - 1)
    else:
        c.update(offset=int(lay["cs"][e]), want_offset=off)
    return cin, c


def t11(total):
    """S = total compacted bases: the last tile full, one base short of full, or one base"""
    if total == 1:
        cin = mk([(F_TID, F_POS, 0, [(1, M)], 3.0, ".")])
    else:
        cin = mk(_feature(total - 30, 0, [(0, 0, [(30, M)], 2.0, "."), (10, 0, [(20, M)], 1.0, ".")]))
    lay = layout(cin)
    return cin, {"S": lay["S"], "want_S": total, "ntiles": lay["ntiles"], "want_ntiles": -(-total // W), "last_tile_bases": (total - 1) % W + 1}


def t12_homes(n):
    """n reads whose homes are one tile: the rounds of 1024 home records of the tile kernel"""
    cin = mk([(F_TID, F_POS + (50 * i) // n, 0, [(20 + i % 13, M)], float(1 + i % 3), ".") for i in range(n)])
    lay = layout(cin)
    return cin, {"homes_of_tile_0": len(tile_homes(lay, 0)), "want_homes_of_tile_0": n, "ntiles": lay["ntiles"], "want_ntiles": 1}


def t12_spills(n=600):
    """n reads that all cross one seam: more spill pieces in one tile than the tile kernels have threads (512, 256)"""
    cin = mk(_feature(W, 95, [((80 * i) // n, 0, [(100, M)], float(1 + i % 4), ".") for i in range(n)]))
    lay = layout(cin)
    j0 = _first_feature(cin, lay)
    n_in = sum(1 for j in range(j0, len(lay["idx"])) for p in spill_pieces(cin, lay, j) if p[0] == 1)
    return cin, {"spill_pieces_in_tile_1": n_in, "want_spill_pieces_in_tile_1": n}


def t13(s):
    """staircase: a carrier read with one N gap, a second bundle, and 1M reads on every covered base with YC cycling 1 .. 7 — every
    compacted base is a change point.  Shift s = 0 .. 4: the zero-depth point (the intron's first base) is change point 2045 + s, over
    the seam 2047 / 2048 of the interval passes; the second bundle's head, at the depth of the base before it, sits on compacted
    base 8190 + s (s = 2: the tile's first base is a head; otherwise a tentative point with a changed depth)"""
    e1, gap, e2, e3 = 2045 + s, 5, 6140, 300
    recs = [(F_TID, F_POS, 0, [(e1, M), (gap, N), (e2, M)], 1.0, "+")]
    q = 0
    yc_last = 0
    for p in list(range(e1)) + list(range(e1 + gap, e1 + gap + e2)):
        yc_last = 1 + q % 7
        recs.append((F_TID, F_POS + p, 0, [(1, M)], float(yc_last), "."))
        q += 1
    p2 = F_POS + e1 + gap + e2 + 1000
    recs.append((F_TID, p2, 0, [(e3, M)], 1.0, "."))
    q = yc_last - 1      # the second bundle's first base repeats the depth of the first bundle's last
    for p in range(e3):
        recs.append((F_TID, p2 + p, 0, [(1, M)], float(1 + q % 7), "."))
        q += 1
    recs.sort(key=lambda r: (r[0], r[1]))       # (stable: the carriers stay in front of the 1M reads on their first base)
    cin = mk(recs)
    lay = layout(cin)
    rows = model(cin)
    head2 = int(np.flatnonzero(lay["head"])[1])
    lens = rows["iv_end"] - rows["iv_start"]
    zero_cp = int(np.sum(rows["iv_start"] < F_POS + e1))          # change points before the intron's first base = its index
    return cin, {"every_row_one_base": bool(np.all(lens == 1)), "rows": rows["n_intervals"], "want_rows": e1 + e2 + e3,
                 "zero_point_index": zero_cp, "want_zero_point_index": 2045 + s, "head_at": int(lay["cs"][head2]), "want_head_at": W - 2 + s,
                 "same_depth_over_the_head": depth_at(cin, lay, W - 3 + s) == depth_at(cin, lay, W - 2 + s), "S_beyond_a_tile": lay["S"] > W}


# ---- record-seam scenes -----------------------------------------------------------------------------------------------------------------
SEAM_N = 2 * CB_TILE + 5
SEAM_K = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, SEAM_N - 1)
SEAM_EVENTS = ("gap1", "touch", "far", "ref", "carried", "carried_in")


def seam(event, k):
    """2 * 4096 + 5 reads of 30M five bases apart, one bundle — but for record k:
    gap1: it starts one base behind the running maximum of the ends (a new bundle); touch: on that maximum (the same bundle);
    far: 10000 bases behind it; ref: on the next reference, at a lower position;
    carried / carried_in: a long read near the start of the input ends one base before record k starts / on its first base, and
    every read between them ends before that: the maximum that decides comes from blocks earlier"""
    recs = []
    shift = {"gap1": 25, "touch": 24, "far": 25 + 9999, "ref": 0, "carried": 225, "carried_in": 224}[event]
    for i in range(SEAM_N):
        tid, pos = F_TID, F_POS + 5 * i
        if i >= k:
            pos += shift
            if event == "ref":
                tid, pos = F_TID + 1, 50 + 5 * (i - k)
        recs.append((tid, pos, 0, [(30, M)], float(1 + i % 3), "."))
    if event in ("carried", "carried_in"):
        c = 0 if k < 3 else 1          # the long read: record 1 (record 0 for the first seams), to 200 bases behind record k - 1's end
        p = recs[c][1]
        recs[c] = (F_TID, p, 0, [(recs[k - 1][1] + 30 + 200 - p, M)], 2.0, ".")
    cin = mk(recs)
    lay = layout(cin)
    prev_max = int(np.max(lay["end"][:k][lay["tid"][:k] == lay["tid"][k - 1]]))
    head = event not in ("touch", "carried_in")
    c = {"record_k_is_head": bool(lay["head"][k]), "want_record_k_is_head": head,
         "bundles": len(lay["b_tid"]), "want_bundles": 2 if head else 1}
    if event != "ref":
        c.update(start_minus_running_max=int(lay["start"][k]) - prev_max,
                 want_start_minus_running_max={"gap1": 1, "touch": 0, "far": 10000, "carried": 1, "carried_in": 0}[event])
    else:
        c.update(start_goes_down=bool(lay["start"][k] < lay["start"][k - 1]), reference_changes=bool(lay["tid"][k] != lay["tid"][k - 1]))
    if event in ("carried", "carried_in"):
        c.update(maximum_from_the_long_read=int(np.argmax(lay["end"][:k])), want_maximum_from_the_long_read=0 if k < 3 else 1)
    return cin, c


# ---- accumulator scenes -------------------------------------------------------------------------------------------------------------------
def _pile(ycs):
    recs = [(F_TID, F_POS + 3 * i, 0, [(30, M), (100, N), (20, M)] if i % 2 else [(50, M)], float(y), "+") for i, y in enumerate(ycs)]
    return mk(_feature(W, 20, [(r[1] - F_POS,) + r[2:] for r in recs]))


def acc_total(total):
    """|YC| total of 2^31 - 2, 2^31 - 1, 2^31 over reads that share bases: the accumulators turn 64 bits wide at 2^31"""
    small = total - 2 * (2**30 - 1)
    ycs = [2**30 - 1, 2**30 - 1] + ([small] if small else [])
    cin = _pile(ycs)
    return cin, {"sum_abs_yc": float(np.sum(np.abs(cin.yc[cin.tid == F_TID]))) + float(np.sum(cin.tid == 0)), "want_sum_abs_yc": float(total + np.sum(cin.tid == 0)),
                 "every_yc_below_2_30": bool(np.all(np.abs(cin.yc) < 2**30))}


def acc_total_exact(total):
    """the same without a spacer (its reads add to the |YC| total): the total is exactly `total`"""
    small = total - 2 * (2**30 - 1)
    ycs = [2**30 - 1, 2**30 - 1] + ([small] if small else [])
    cin = mk([(F_TID, F_POS + 3 * i, 0, [(30, M), (100, N), (20, M)] if i % 2 else [(50, M)], float(y), "+") for i, y in enumerate(ycs)])
    lay = layout(cin)
    return cin, {"sum_abs_yc": float(np.sum(np.abs(cin.yc))), "want_sum_abs_yc": float(total), "every_yc_below_2_30": bool(np.all(np.abs(cin.yc) < 2**30)),
                 "depth": depth_at(cin, lay, 10), "want_depth": float(total)}


def acc_special(what):
    """a read of YC exactly 2^30 (not below it: the ordered path), a YC of 0 that is present, a YC of 0.5"""
    ycs = {"2^30": [3, 2**30, 5], "zero": [3, 0, 5, 0], "half": [3, 0.5, 5]}[what]
    cin = _pile(ycs)
    frac = bool(np.any(cin.yc != np.floor(cin.yc)) or np.any(np.abs(cin.yc) >= 2**30))
    return cin, {"takes_the_ordered_path": frac, "want_takes_the_ordered_path": what != "zero", "has": float(ycs[1]) in cin.yc.tolist()}


# ---- order scene ----------------------------------------------------------------------------------------------------------------------------
def order(reverse):
    """300 reads with YC 0.1, 0.2, 0.3 repeating (or that sequence reversed) that all cross one seam — spills on the far side, added in
    record order — with the same intron in every read; fractional home records of the far tile on top"""
    ycs = [(0.1, 0.2, 0.3)[i % 3] for i in range(300)]
    if reverse:
        ycs = ycs[::-1]
    recs = [(i // 3, 0, [(250 - i // 3, M), (50, N), (60, M)], ycs[i], "+") for i in range(300)]
    recs += [(160 + q, 0, [(40, M)], 0.7 if q % 2 else 0.15, ".") for q in range(30)]
    cin = mk(_feature(W, 150, recs))
    lay = layout(cin)
    j0 = _first_feature(cin, lay)
    return cin, {"reads_across_the_seam": sum(1 for j in range(j0, j0 + 300) if any(p[0] == 1 for p in spill_pieces(cin, lay, j))),
                 "want_reads_across_the_seam": 300, "homes_of_the_far_tile": len(tile_homes(lay, 1)), "want_homes_of_the_far_tile": 30}


# ---- junction scenes --------------------------------------------------------------------------------------------------------------------------
def j1(n):
    """n distinct introns on one start, strands cycling: 64 / 65 items in one home (wave sort / block sort), 1024 / 1025 (the home's
    capacity), and a table (1024 slots) that cannot hold them all"""
    cin = mk([(F_TID, F_POS, 0, [(10, M), (100 + i, N), (10, M)], float(1 + i % 4), "+-."[i % 3]) for i in range(n)])
    lay = layout(cin)
    homes = junction_items(cin, lay)
    return cin, {"distinct": model(cin)["n_junctions"], "want_distinct": n, "items_per_home": sorted(homes.values()), "want_items_per_home": [n]}


def j2(n=9000):
    """n reads on one start, alternating two introns, strands + - . cycling: the sums of six junctions meet across the blocks of 4096
    and of 1024 records; n >= 65536: the junction branch runs on the side context"""
    cin = mk([(F_TID, F_POS, 0, [(10, M), (100 + 50 * (i % 2), N), (10, M)], float(1 + i % 5), "+-."[i % 3]) for i in range(n)])
    res = model(cin)
    same = (res["j_start"][0] == res["j_start"][1] == res["j_start"][2]) and (res["j_end"][0] == res["j_end"][1] == res["j_end"][2])
    return cin, {"distinct": res["n_junctions"], "want_distinct": 6, "three_strands_in_char_order": bool(same) and bytes(res["j_strand"][:3]) == b"+-.",
                 "records": n}


def j3():
    """junctions that start 2^24 - 1 and 2^24 bases behind their block's first record (the widest relative start the block key
    holds, and the first it does not); a reference change inside a block with the same (start, length) on both references"""
    p0 = 100
    far = p0 + 2**24 - 12
    recs = [(F_TID, p0, 0, [(10, M), (50, N), (10, M)], 2.0, "+"), (F_TID, 500, 0, [(10, M), (50, N), (10, M)], 1.0, "+"),
            (F_TID, 500, 0, [(10, M), (50, N), (10, M)], 3.0, "+"),
            (F_TID, far, 0, [(10, M), (50, N), (10, M)], 1.0, "-"), (F_TID, far, 0, [(10, M), (50, N), (10, M)], 4.0, "-"),
            (F_TID, far + 1, 0, [(10, M), (50, N), (10, M)], 2.0, "-"), (F_TID, far + 1, 0, [(10, M), (50, N), (10, M)], 5.0, "-"),
            (F_TID + 1, 500, 0, [(10, M), (50, N), (10, M)], 7.0, "+"), (F_TID + 1, 500, 0, [(10, M), (50, N), (10, M)], 1.0, "+")]
    cin = mk(recs)
    res = model(cin)
    rel = sorted(set(int(s) + 1 - p0 for s, t in zip(res["j_start"], res["j_tid"]) if t == F_TID))
    return cin, {"relative_starts": rel[-2:], "want_relative_starts": [2**24 - 1, 2**24], "distinct": res["n_junctions"], "want_distinct": 5,
                 "same_on_both_references": sorted(res["j_tid"][res["j_start"] == 510].tolist()), "want_same_on_both_references": [F_TID, F_TID + 1]}


def j4():
    """0N; 24M 7N 2S, a CIGAR that ends in an intron; a read with four exons; reads without introns between"""
    recs = [(F_TID, F_POS, 0, [(40, M)], 1.0, "."), (F_TID, F_POS + 2, 0, [(10, M), (0, N), (10, M)], 2.0, "+"), (F_TID, F_POS + 3, 0, [(30, M)], 1.0, "."),
            (F_TID, F_POS + 9, 0, [(24, M), (7, N), (2, S)], 3.0, "."), (F_TID, F_POS + 12, 0, [(5, M), (20, N), (5, M), (30, N), (5, M), (40, N), (5, M)], 2.0, "-"),
            (F_TID, F_POS + 12, 0, [(25, M)], 1.0, "+"), (F_TID, F_POS + 12, 0, [(5, M), (20, N), (5, M), (30, N), (5, M), (40, N), (5, M)], 1.0, "-")]
    cin = mk(recs)
    res = model(cin)
    return cin, {"distinct": res["n_junctions"], "want_distinct": 5, "empty_intron": bool(np.any(res["j_end"] == res["j_start"])),
                 "intron_to_the_read_end": bool(np.any((res["j_start"] == F_POS + 9 + 24) & (res["j_end"] == F_POS + 9 + 31)))}


def j5(n_short):
    """10M 100000N 10M, then n_short short reads that start before the intron's first base, one of them (at nine tenths) with the
    same junction: its home is the last block of 1024 records, where the two meet"""
    recs = [(F_TID, F_POS, 0, [(10, M), (100000, N), (10, M)], 3.0, "+")]
    at = n_short * 9 // 10
    for i in range(n_short):
        p = (10 * i) // n_short
        recs.append((F_TID, F_POS + p, 0, [(10 - p, M), (100000, N), (10, M)] if i == at else [(5, M)], 2.0 if i == at else 1.0, "+" if i == at else "."))
    cin = mk(recs)
    lay = layout(cin)
    res = model(cin)
    homes = junction_items(cin, lay)
    return cin, {"distinct": res["n_junctions"], "want_distinct": 1, "sum": float(res["j_val"][0]), "want_sum": 5.0,
                 "home": sorted(homes), "want_home": [n_short // JH_REC], "items": sum(homes.values()), "want_items": 1 if n_short + 1 <= JA_REC else 2}


# ---- the top of the coordinate range ------------------------------------------------------------------------------------------------------------
def top():
    """a spliced read whose last base is 2^31 - 1, across a tile seam, under a second read"""
    p = TOP - 120
    cin = mk(spacer(W - 60) + [(F_TID, p - 30, 0, [(60, M)], 1.0, "."), (F_TID, p, 0, [(10, M), (100, N), (10, M)], 2.0, "+")])
    lay = layout(cin)
    return cin, {"last_base": int(lay["end"][-1]), "want_last_base": TOP, "seam_inside": int(lay["cs"][-1]) < W < int(lay["cs"][-1]) + 120}


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------------
def _sweep(f, *more):
    """{(k, d, ...): thunk} over SWEEP_K x SWEEP_D x the further axes"""
    out = {}
    axes = [[]]
    for m_ in more:
        axes = [a + [v] for a in axes for v in m_]
    for k in SWEEP_K:
        for d in SWEEP_D:
            for a in axes:
                out[(k, d) + tuple(a)] = functools.partial(f, k, d, *a)
    return out


# swept tile scenes: name -> {sweep value: thunk}; every thunk's claims hold "offset" / "want_offset"
SWEPT = {
    "t1": _sweep(t1), "t2": _sweep(t2), "t3": _sweep(t3, (False, True)), "t4": _sweep(t4, ("fall", "rise")), "t5": _sweep(t5, (False, True)),
    "t6": _sweep(t6), "t7": _sweep(t7, (-1, 0, 1)), "t9": _sweep(t9), "t10": _sweep(t10, ("first", "last", "inside", "between")),
}
TILE_SINGLES = {
    "t8": {(w, b, s): functools.partial(t8, w, b, s) for w in (63, 64, 65) for b in (False, True) for s in (False,)},
    "t8s": {(64, b, True): functools.partial(t8, 64, b, True) for b in (False, True)},
    "t11": {s: functools.partial(t11, s) for s in (1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)},
    "t12": dict([(n, functools.partial(t12_homes, n)) for n in (1023, 1024, 1025, 2049)] + [("spills", t12_spills)]),
    "t13": {s: functools.partial(t13, s) for s in range(5)},
}
TILE = dict(SWEPT, **TILE_SINGLES)
SEAM = {e: {k: functools.partial(seam, e, k) for k in SEAM_K} for e in SEAM_EVENTS}
ACC = {"acc": dict([(t, functools.partial(acc_total_exact, t)) for t in (2**31 - 2, 2**31 - 1, 2**31)] +
                   [("spaced-%d" % (t - 2**31), functools.partial(acc_total, t)) for t in (2**31 - 2, 2**31 - 1, 2**31)] +
                   [(w, functools.partial(acc_special, w)) for w in ("2^30", "zero", "half")])}
TOPS = {"top": {0: top}}
JUNC = {"j1": {n: functools.partial(j1, n) for n in (64, 65, 1024, 1025, 1100)}, "j2": {9000: functools.partial(j2, 9000)}, "j3": {0: j3}, "j4": {0: j4},
        "j5": {n: functools.partial(j5, n) for n in (3000, 5000)}, "top": {0: top}}
J2_SIDE = 66000
INTERVAL_SCENES = dict(TILE, **SEAM, **ACC, **TOPS)


@functools.lru_cache(maxsize=None)
def build(group, name, value):
    """(cin, claims) of one scene, built once"""
    table = {"interval": INTERVAL_SCENES, "junction": JUNC}[group]
    return table[name][value]()


def check_claims(claims):
    """every "want_X" equals "X"; every other boolean claim is true"""
    bad = []
    for key, v in claims.items():
        if key.startswith("want_"):
            if claims[key[5:]] != v:
                bad.append((key[5:], claims[key[5:]], v))
        elif isinstance(v, (bool, np.bool_)) and ("want_" + key) not in claims and not v:
            bad.append((key, v, True))
    return bad
