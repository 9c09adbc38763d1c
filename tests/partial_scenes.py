"""Hand-built partial rows for the owner's step of the multi-rank protocol: tbk_partial_reduce (tiebrush_amd/csrc/wgroup.hip from "group
partials: the owner's merge-reduce" on — pr_rowkeys_k, pr_sample_rank_k, wg_split_k, the offsets build, pr_merge_k, pr_compact_k).

A SCENE is a list of runs; a run is the list of records one rank holds, as helpers.tile_from_records takes them.  Every rank collapses
its records and packs its groups into rows (include/tbk.h: TBK_PARTIAL_ROW); the owner receives the runs end to end.  A scene may edit
words of the packed rows (effective end, YC, YX, YD: what a real rank would have computed from more reads than a test can hold), and it
says in one sentence which edge of the kernels it sits on.

The MODEL (partition) restates the host arithmetic of tbk_partial_reduce_device and the rules of pr_sample_rank_k / wg_split_k from the
places (tid, pos) of the rows alone.  The four constants are read out of wgroup.hip: a retune fails tests/test_partial_scenes_cpu.py
instead of moving the scenes off their edges unnoticed.

The EXPECTED result has nothing of the device in it: the received rows, read as a tile whose files are the runs (dist._partial_unpack_np:
all TieBrush-merged, explicit priorities), collapsed by the CPU oracle plus the priority rule (dist_helpers.OracleCompute).

tests/test_partial_scenes_cpu.py proves every scene's claim without a GPU; tests/test_gpu_partial_reduce.py runs the scenes."""
import functools
import os
import re

import numpy as np

from dist_helpers import OracleCompute
from helpers import tile_from_records
import window_model as wm

M, I, D, N, S = 0, 1, 2, 3, 4
E2BIG, EUNSUPPORTED, ECOLLISION = -4, -5, -8          # include/tbk.h

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tiebrush_amd", "csrc", "wgroup.hip")


def _constants():
    with open(_SRC) as fh:
        src = fh.read()
    env = {}
    for name in ("PR_T", "PR_KS", "PR_CAP", "PR_MAXRUNS"):
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, "constant %s not found in wgroup.hip" % name
        env[name] = int(eval(m.group(1), {"__builtins__": {}}, dict(env)))      # (PR_CAP = 3 * PR_T)
    m = re.search(r"constexpr\s+int\s+PR_NT\s*=\s*(\d+);", src)
    assert m, "constant PR_NT not found in wgroup.hip"
    env["PR_NT"] = int(m.group(1))
    return env


_C = _constants()
PR_T, PR_KS, PR_CAP, PR_MAXRUNS, PR_NT = _C["PR_T"], _C["PR_KS"], _C["PR_CAP"], _C["PR_MAXRUNS"], _C["PR_NT"]


# ---- the model ------------------------------------------------------------------------------------------------------------------
def stride(k):
    """s, g of tbk_partial_reduce_device: while (s * 2 * k <= PR_KS && s * 2 <= PR_T) s *= 2; g = PR_T / s"""
    s = 1
    while s * 2 * k <= PR_KS and s * 2 <= PR_T:
        s *= 2
    return s, PR_T // s


def place_keys(rows):
    """chi >> 2 of pr_rowkeys_k: (tid << 31) | pos of placed rows"""
    r = np.asarray(rows).astype(np.int64)
    return wm.raw_key(r[:, 0], r[:, 1])


def partition(place_keys_per_run):
    """The windows of tbk_partial_reduce for runs whose rows carry these places (one sorted uint64 array per run).
    -> dict(k, m, s, g, ns, nsp, nw, rank (of every sample), W (bounds), heavy (per window), win (window of every row, the runs end to
    end), count (rows per window), bound (what a window that is not heavy is claimed to stay below))"""
    k = len(place_keys_per_run)
    keys = np.concatenate([np.asarray(a, np.uint64) for a in place_keys_per_run]) if k else np.zeros(0, np.uint64)
    run_off = np.concatenate([[0], np.cumsum([len(a) for a in place_keys_per_run])]).astype(np.int64)
    m = len(keys)
    s, g = stride(k)
    ns = -(-m // s)
    nsp = (ns - 1) // g if ns > 1 else 0
    nw = 2 * nsp + 1
    samples = keys[np.arange(ns, dtype=np.int64) * s]
    rank = np.zeros(ns, np.int64)
    if nsp:
        # pr_sample_rank_k: j0[r] = first sample at or behind run r's first row; a sample's rank = its index in its own run's samples +
        # the samples before it in every other run (before: <, and = for the runs ahead of its own)
        j0 = np.concatenate([(run_off[:k] + s - 1) // s, [ns]])
        own = np.zeros(ns, np.int64)
        for q in range(1, k):
            own[np.arange(ns) >= j0[q]] = q                  # last q with j0[q] <= j
        rank = np.arange(ns) - j0[own]
        for q in range(k):
            sq = samples[j0[q]:j0[q + 1]]
            other = own != q
            before = np.where(q < own, np.searchsorted(sq, samples, side="right"), np.searchsorted(sq, samples, side="left"))
            rank = rank + np.where(other, before, 0)
        Y = np.zeros(ns, np.uint64)
        Y[rank] = samples                                     # (a rank taken twice would leave a hole: the CPU test checks the permutation)
    else:
        Y = samples
    W, heavy_first = wm.split_bounds(Y, g, nsp)
    win = np.searchsorted(W, keys, side="right")
    count = np.bincount(win, minlength=nw)
    heavy = np.zeros(nw, bool)
    heavy[1::2] = heavy_first
    return dict(k=k, m=m, s=s, g=g, ns=ns, nsp=nsp, nw=nw, rank=rank, W=W, heavy=heavy, win=win, count=count, bound=2 * PR_T + k * s)


# ---- records --------------------------------------------------------------------------------------------------------------------
def rec(pos, cig=None, span=50, tid=0, strand="+"):
    return (tid, int(pos), 0, 60, strand, 1, cig if cig is not None else [(int(span), M)])


def _spread(m, k, pos=lambda i: 100 + 10 * i):
    """m rows on m places, row i in run i % k"""
    runs = [[] for _ in range(k)]
    for i in range(m):
        runs[i % k].append(rec(pos(i)))
    return runs


# the tie sets: alignments with equal (tid, start, strand, span = 100)
ONE = [(100, M)]
MNM_A = [(10, M), (80, N), (10, M)]
MNM_B = [(20, M), (60, N), (20, M)]
EX3_A = [(10, M), (20, N), (10, M), (30, N), (30, M)]
EX3_B = [(10, M), (30, N), (10, M), (20, N), (30, M)]
EX3_C = [(20, M), (20, N), (10, M), (30, N), (20, M)]
INS_A = [(50, M), (2, I), (50, M)]
INS_B = [(50, M), (4, I), (50, M)]
DEL_A = [(40, M), (10, D), (50, M)]
CLIP_A = [(5, S), (100, M)]
CLIP_B = [(100, M), (7, S)]
EX3_A_CLIP = [(3, S)] + EX3_A


def _trio(pos, a, b, c, strands=("+", "+", "+")):
    """three alignments on one base, spread as {a, c}, {b, c}, {a, b} over three runs"""
    A, B, Cc = (rec(pos, x, strand=st) for x, st in zip((a, b, c), strands))
    return [[A, Cc], [B, Cc], [A, B]]


def _tie_runs():
    runs = [[], [], []]
    trios = [_trio(1000, ONE, MNM_A, MNM_B),                 # exact key words: one exon, M N M
             _trio(2000, EX3_A, EX3_B, EX3_C),               # hashed: three exons
             _trio(3000, INS_A, INS_B, DEL_A),               # hashed under cigar / clip; one exon, one group under exon
             _trio(4000, CLIP_A, ONE, CLIP_B),               # hashed under cigar; equal and exact under clip and exon
             _trio(5000, EX3_A, EX3_A_CLIP, EX3_B),          # hashed; the soft clip parts two of them under cigar only
             _trio(6000, ONE, ONE, ONE, ("+", "-", ".")),    # the three strands on one base
             _trio(7000, ONE, EX3_A, MNM_A)]                 # an exact and a hashed key word in one tie set
    for t in trios:
        for r in range(3):
            runs[r] += t[r]
    return runs


def _seam(n):
    """n rows on one base in 3 runs: every fifth span in all three runs, the others in one — a group of three begins every 7 sorted
    positions, so on every residue of a thread's range of 2, 3, 5 or 6 positions"""
    runs = [[], [], []]
    tot, i = 0, 0
    while tot < n:
        if i % 5 == 0 and tot + 3 <= n:
            for r in range(3):
                runs[r].append(rec(1000, span=i + 1))
            tot += 3
        else:
            runs[i % 3].append(rec(1000, span=i + 1))
            tot += 1
        i += 1
    return runs


def _pile(k, per_run, extra=0):
    """k runs x per_run spans on one base, interleaved (run r holds the spans 1 + r + k j); `extra` more in run 0"""
    runs = [[rec(1000, span=1 + r + k * j) for j in range(per_run)] for r in range(k)]
    runs[0] += [rec(1000, span=k * per_run + 1 + e) for e in range(extra)]
    return runs


def _heavy():
    runs = [[] for _ in range(4)]
    for j in range(1000):
        runs[j % 4].append(rec(100 + 10 * j))
    for r in range(4):
        runs[r] += [rec(20000, span=1 + r + 4 * t) for t in range(300)]
    for j in range(1000, 2000):
        runs[j % 4].append(rec(50000 + 10 * j))
    return runs


def _big_and_tiny():
    runs = []
    for r in range(64):
        if r == 17:
            runs.append([rec(100 + 10 * i) for i in range(4000)])
        else:
            runs.append([rec(100 + 10 * (60 * r) + (5 if r % 2 else 0))])      # even runs: a place of the long run; odd: one of their own
    return runs


def _empty_runs():
    live = [1, 2, 3, 5, 6]
    runs = [[] for _ in range(8)]
    for i in range(1250):
        runs[live[i % 5]].append(rec(100 + 10 * i))
        if i % 10 == 0:
            runs[live[(i + 1) % 5]].append(rec(100 + 10 * i))
    return runs


def _three_refs():
    def place(i):
        t = 0 if i < 256 else (1 if i < 768 else 2)
        return rec(100 + 10 * (i - (0, 256, 768)[t]), tid=t)
    run = [place(i) for i in range(1024)]
    return [list(run), list(run)]


def _group64():
    runs = [[] for _ in range(64)]
    for i in range(250):
        runs[i % 64].append(rec(1000, span=1 + i))
    for r in range(64):
        runs[r].append(rec(1000, span=300))
    for i in range(30):
        runs[i % 64].append(rec(1000, span=400 + i))
    return runs


def _last_single():
    runs = [[], [], []]
    for i in range(253):
        runs[i % 3].append(rec(1000, span=1 + i))
    for r in range(3):
        runs[r].append(rec(1000, span=254))
    runs[1].append(rec(1000, span=255))
    return runs


def _reduction():
    runs = [[rec(100 + 5 * (6 * i + r)) for i in range(20)] for r in range(6)]
    for r in range(6):
        runs[r] += [rec(p, span=150) for p in (1000, 2000, 3000, 4000, 5000)]
    edits = [(5, 1000, 3, 1100), (2, 1000, 3, 1100),                 # equal effective ends in runs 5 and 2
             (5, 2000, 3, 2001)]                                     # the smallest in the last run
    edits += [(r, 3000, 8, 0) for r in range(6)]                     # YD all 0
    edits += [(r, 4000, 8, (3, 9, 40, 9, 3, 1)[r]) for r in range(6)]  # YD maximum in a middle run
    edits += [(r, 5000, 6, r + 1) for r in range(6)] + [(r, 5000, 7, r + 10) for r in range(6)]
    return runs, edits


def _same_place(k, extra=3):
    return [[rec(100 + 10 * (k * i + r)) for i in range(extra)] + [rec(1000, span=150)] for r in range(k)]


def _collision():
    runs = [[rec(100 + 10 * r), rec(1000, EX3_A), rec(3000 + 10 * r)] for r in range(4)]
    runs.append([rec(140), rec(1000, EX3_B), rec(3040)])
    return runs


class Scene:
    def __init__(self, edge, runs, strategy="cigar", edits=(), expect=0, mask=None, reverse=True, **claim):
        self.edge, self.runs, self.strategy, self.edits, self.expect, self.mask, self.reverse, self.claim = \
            edge, runs, strategy, list(edits), expect, mask, reverse, claim
        for run in runs:      # a rank's records are coordinate-sorted
            assert all((a[0], a[1]) <= (b[0], b[1]) for a, b in zip(run, run[1:])), edge

    @property
    def k(self):
        return len(self.runs)


def _scenes():
    sc = {}
    for k in (1, 64):
        for m in (1, 511, 512, 513):
            sc["split_%dx%d" % (k, m)] = Scene("%d run(s), %d rows on distinct places: the first splitter appears between 512 and 513 rows" % (k, m),
                                               _spread(m, k), windows=1 if m <= 512 else 3, groups=m, members={1: m})
    for k in (2, 7):
        sc["split_%dx1025" % k] = Scene("%d runs, 2 * 512 + 1 rows: the second splitter" % k, _spread(1025, k), windows=5, groups=1025,
                                        members={1: 1025})
    sc["big_and_tiny"] = Scene("64 runs, one of 4000 rows among 63 of one row: most runs hold no sample at all", _big_and_tiny(),
                               windows=15, groups=4031, members={1: 3999, 2: 32})
    sc["empty_runs"] = Scene("8 runs with the first, a middle and the last one empty: j0[] repeats a value, pieces of length 0",
                             _empty_runs(), windows=5, groups=1250, members={1: 1125, 2: 125}, empty_runs=[0, 4, 7])
    sc["reverse_ranges"] = Scene("4 runs on disjoint coordinate ranges in reverse rank order: every window is one run's",
                                 [[rec((3 - r) * 100000 + 10 * i) for i in range(300)] for r in range(4)], windows=5, groups=1200,
                                 members={1: 1200})
    sc["identical64"] = Scene("64 identical runs: every group has 64 members, one per run", [[rec(100 + 10 * i) for i in range(20)]] * 64,
                              windows=5, groups=20, members={64: 20})
    sc["three_refs"] = Scene("rows on three references, the first place of the second and of the third reference is a splitter",
                             _three_refs(), windows=7, groups=1024, members={2: 1024}, splitters=[(1, 100), (2, 100)])
    sc["heavy"] = Scene("1200 rows on one base inside 2000 light rows: equal consecutive splitters, a heavy window [v, v + 1)", _heavy(),
                        windows=13, groups=3200, members={1: 3200}, heavy=1200)
    sc["cap_1x1536"] = Scene("exactly PR_CAP rows on one base from one run: merged", _pile(1, 1536), windows=5, groups=1536,
                             members={1: 1536}, heavy=1536)
    sc["cap_64x24"] = Scene("exactly PR_CAP rows on one base, 24 from each of 64 runs, interleaved: merged", _pile(64, 24), windows=5,
                            groups=1536, members={1: 1536}, heavy=1536)
    sc["cap_64x24_plus1"] = Scene("PR_CAP + 1 rows on one base: refused, the general path takes the tile", _pile(64, 24, 1), expect=E2BIG,
                                  windows=7, groups=1537, members={1: 1537}, heavy=1537)
    sc["pile_4x1537"] = Scene("PR_CAP + 1 rows on one base in 4 runs: refused (the scene the loopback driver runs)", _pile(4, 384, 1),
                              expect=E2BIG, windows=7, groups=1537, members={1: 1537}, heavy=1537)
    for n in (255, 256, 257, 512, 513, 1280, 1281):
        s3, g3 = stride(3)
        ns = -(-n // s3)
        sc["seam_%d" % n] = Scene("one window of %d rows in 3 runs: thread t owns ceil(%d / 256) sorted positions, groups of three cross "
                                  "the ranges" % (n, n), _seam(n), windows=2 * ((ns - 1) // g3 if ns > 1 else 0) + 1, one_window=n)
    sc["seam_group64"] = Scene("a group of 64 members on the sorted positions 250 - 313 of one window", _group64(), windows=1,
                               groups=281, members={1: 280, 64: 1}, one_window=344, group_at=(250, 64))
    sc["seam_last_single"] = Scene("a group of one member on the last sorted position (256, the one position of thread 128)",
                                   _last_single(), windows=1, groups=255, members={1: 254, 3: 1}, one_window=257, group_at=(256, 1))
    for st in ("cigar", "clip", "exon"):
        sc["ties_%s" % st] = Scene("tie sets under %s: three alignments on one key spread as {A, C}, {B, C}, {A, B} over three runs, exact and "
                                   "hashed key words, pairs the strategy calls equal, three strands" % st, _tie_runs(), strategy=st,
                                   windows=1, ties=True)
    runs, edits = _reduction()
    sc["reduction"] = Scene("the representative on equal effective ends (runs 5 and 2) and in the last run; YD all 0 and largest in a middle "
                            "run; YC, YX sums", runs, edits=edits, windows=1, groups=125, members={1: 120, 6: 5},
                            rep_run={1000: (5, 2), 2000: (5,)}, sums={5000: (21.0, 75), 4000: (None, None, 40), 3000: (None, None, 0)})
    sc["yc_big"] = Scene("YC of 2^31 - 1 in 64 runs: the sum is exact in a double", _same_place(64, 1),
                         edits=[(r, 1000, 6, 2**31 - 1) for r in range(64)], windows=1, groups=65, members={1: 64, 64: 1},
                         sums={1000: (64.0 * (2**31 - 1), None)})
    yx = (2**31 - 1, 2**31 - 1, 1)
    sc["yx_fits"] = Scene("YX of three runs summing to 2^32 - 1: accepted", _same_place(3), edits=[(r, 1000, 7, yx[r]) for r in range(3)],
                          windows=1, groups=10, members={1: 9, 3: 1}, sums={1000: (3.0, 2**32 - 1)})
    sc["yx_over"] = Scene("YX of three runs summing to 2^32: refused", _same_place(3),
                          edits=[(r, 1000, 7, yx[r] + (r == 2)) for r in range(3)], expect=E2BIG, windows=1, groups=10,
                          members={1: 9, 3: 1}, sums={1000: (3.0, 2**32)})
    sc["runs65"] = Scene("65 runs: more than a wave's piece table", _spread(65, 65), expect=EUNSUPPORTED, reverse=False, groups=65,
                         members={1: 65})
    sc["no_rows"] = Scene("n2 = 0: no groups, status 0", [[], []], reverse=False, windows=1, groups=0, members={})
    sc["odd_last"] = Scene("a place with one alignment in four runs and another of the same span in the fifth: two groups", _collision(),
                           windows=1, groups=12, members={1: 11, 4: 1})
    sc["odd_last_masked"] = Scene("the same with the hash word masked away at the pack: five rows share a key word, the odd alignment is "
                                  "the last member: refused", _collision(), mask="0", expect=ECOLLISION, reverse=False, windows=1,
                                  groups=12, members={1: 11, 4: 1})
    return sc


SCENES = _scenes()
LOOPBACK = ("pile_4x1537", "odd_last_masked", "heavy")        # through dist.run_loopback, unedited, against the flat oracle


# ---- rows of a scene, on the host ------------------------------------------------------------------------------------------------
def order_of(name, reverse=False):
    """run ids in the order the owner receives them (reverse: the ranks hold the runs in reversed order)"""
    k = SCENES[name].k
    return list(range(k))[::-1] if reverse else list(range(k))


def tiles_of(name, reverse=False):
    """one tile per rank in rank order (None for a rank without records), and every rank's first global file index"""
    sc = SCENES[name]
    return [tile_from_records([sc.runs[r]]) if sc.runs[r] else None for r in order_of(name, reverse)], list(range(sc.k))


def apply_edits(name, rows, run_off, reverse=False):
    """rows [n2, 12] int32 (host) with the scene's edits: (run id, pos, word, value) sets `word` of every row of that run on `pos`"""
    sc = SCENES[name]
    rows = np.array(rows, np.int32)
    where = {r: p for p, r in enumerate(order_of(name, reverse))}
    for run, pos, word, value in sc.edits:
        a, b = int(run_off[where[run]]), int(run_off[where[run] + 1])
        hit = np.flatnonzero(rows[a:b, 1] == pos) + a
        assert len(hit) == 1, (name, run, pos)
        rows[hit, word] = np.array([value], np.uint32).view(np.int32)[0]
    return rows


@functools.lru_cache(maxsize=None)
def packed(name, reverse=False):
    """the rows as received, packed on the host (dist._partial_pack_np after the oracle's local collapses; word 10 absent), edits
    applied -> (rows, run_off, cig words)"""
    from tiebrush_amd import dist
    sc = SCENES[name]
    tiles, first = tiles_of(name, reverse)
    rows_all, cig_all, cnt = [np.zeros((0, dist.PROW), np.int32)], [np.zeros(0, np.uint32)], []
    for t, f in zip(tiles, first):
        if t is None:
            cnt.append(0)
            continue
        fin = OracleCompute().collapse(t, strategy=sc.strategy, want_effend=True)
        key, _, bad = dist._partial_keys_np(t, fin)
        assert not bad
        rows, cigw, tab = dist._partial_pack_np(t, fin, key, None, 1, f)
        rows_all.append(rows)
        cig_all.append(np.asarray(cigw, np.uint32)[:int(tab[0, 2])])
        cnt.append(int(tab[0, 1]))
    run_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    rows = apply_edits(name, np.concatenate(rows_all), run_off, reverse)
    rows.setflags(write=False)
    return rows, run_off, np.concatenate(cig_all)


def unpacked_tile(rows, run_off, cig):
    """the tile tbk_partial_unpack describes: files = runs, all TieBrush-merged, prio_hi / prio_lo from the rows"""
    from tiebrush_amd import dist
    from tiebrush_amd.soa import SoATile
    A = dist._partial_unpack_np(np.asarray(rows))
    k = len(run_off) - 1
    return SoATile(n_files=k, file_off=np.asarray(run_off, np.uint32), tbmerged=np.ones(k, np.uint8), cig=np.asarray(cig, np.uint32), **A)


def expected(rows, run_off, cig, strategy):
    """-> (tile of the received rows, the oracle's collapse of it under the priority rule, with the record -> group map)"""
    t2 = unpacked_tile(rows, run_off, cig)
    want = OracleCompute().collapse(t2, strategy=strategy, keep_supplementary=True, keep_secondary=True)
    return t2, want


@functools.lru_cache(maxsize=None)
def expected_of(name, reverse=False):
    rows, run_off, cig = packed(name, reverse)
    return expected(rows, run_off, cig, SCENES[name].strategy)


@functools.lru_cache(maxsize=None)
def partition_of(name, reverse=False):
    rows, run_off, _ = packed(name, reverse)
    keys = place_keys(rows)
    return partition([keys[int(run_off[r]):int(run_off[r + 1])] for r in range(len(run_off) - 1)])


def flat_tile(name, reverse=False):
    """all records of the scene as one tile, the files in rank order"""
    sc = SCENES[name]
    return tile_from_records([sc.runs[r] for r in order_of(name, reverse)])


def exact_key_word(cig, strategy):
    """record_key (tiebrush_amd/csrc/strategy.hpp): is the key word of this CIGAR an exact code (bit 31 set) under the strategy — a single
    reference-consuming operation (soft clips stripped under clip), one exon under exon, or M N M / two exons with a first block < 2^10
    and a gap < 2^20 — or a hash the owner must verify?"""
    ops = [(l, o) for l, o in cig]
    if strategy == "exon":
        nex = 1 + sum(1 for _, o in ops if o == N)
        return nex <= 2                      # (the scenes' blocks and gaps are far below the limits)
    if strategy == "clip":
        while ops and ops[0][1] == S:
            ops = ops[1:]
        while ops and ops[-1][1] == S:
            ops = ops[:-1]
    if len(ops) == 1:
        return ops[0][1] in (M, D, N, 7, 8)
    return [o for _, o in ops] == [M, N, M] and ops[0][0] < (1 << 10) and ops[1][0] < (1 << 20)
