"""Hand-built scenes on the edges of the multi-rank cut search (tiebrush_amd/csrc/shard.hip: tbk_partial_stage_keys / _cands / _pack):
the padded bitonic sort of the samples, the walk in steps of 256 groups with its ballots, the three sources of a horizon, the
comparisons of partial_choose_k where one unit decides, and keys whose bits above 2^32 are live.  tests/test_cut_model_cpu.py shows
on the CPU model (cut_model.py) that every scene sits on the edge it is named for; tests/test_gpu_cut_search.py demands the model's
arrays of the device.

Three kinds of scene:
  TABLE   per-rank key / keyed-end arrays and sample rows written by hand (tbk_partial_stage_cands takes bare device arrays);
  CHOOSE  gathered candidate lists and targets written by hand (tbk_partial_stage_pack reads them as given) over one tiny tile;
  TILE    real reads, one read per group, single-M CIGARs, as per-rank files for helpers.tile_from_records / dist_helpers.split_tile.
Every scene carries the sentence that says which edge it sits on."""
import functools

import numpy as np

import cut_model as cm

INF, K = cm.INF, cm.K
M = 0
BIG_TID = 70000                 # (tid + 1) << 31 has bits above 2^47


class Rank:
    """one rank's groups as the cut search sees them: start keys in order, each group's own keyed end, and the running maximum"""

    def __init__(self, key, endk):
        self.key, self.endk = np.asarray(key, np.int64).reshape(-1), np.asarray(endk, np.int64).reshape(-1)
        assert len(self.key) == len(self.endk) and np.all(self.key[1:] >= self.key[:-1]) and np.all(self.endk > self.key)
        self.emax = np.maximum.accumulate(self.endk) if len(self.key) else np.zeros(0, np.int64)

    @property
    def ng(self):
        return len(self.key)


def rank_of(groups):
    """(tid, start, end) triples in (tid, start) order"""
    g = np.asarray(groups, np.int64).reshape(-1, 3)
    return Rank(((g[:, 0] + 1) << 31) | g[:, 1], ((g[:, 0] + 1) << 31) | (g[:, 2] + 1))


EMPTY = Rank([], [])


def chain(tid, start, heads, length=6, gap=2):
    """groups from a list of booleans: a head starts `gap` beyond the farthest end so far (gap 2 is the closest clean start, gap 1
    touches and opens nothing), every other group one base behind its predecessor, inside what came before; all `length` long"""
    out, s, far = [], start, None
    for h in heads:
        s = s + 1 if (far is None or not h) else far + gap
        out.append((tid, s, s + length - 1))
        far = s + length - 1 if far is None else max(far, s + length - 1)
    return out


def head_flags(n, head_at):
    f = np.zeros(n, bool)
    f[list(head_at)] = True
    return f.tolist()


class TableScene:
    def __init__(self, name, doc, ranks, allmeta, **edge):
        self.name, self.doc, self.ranks, self.allmeta, self.edge = name, doc, ranks, np.asarray(allmeta, np.int64), edge
        self.world = len(ranks)
        assert self.allmeta.shape == (self.world, cm.META)

    def __repr__(self):
        return "TableScene(%s: world %d, groups %s)" % (self.name, self.world, [r.ng for r in self.ranks])


def rows_for_targets(world, tg):
    """sample rows that make partial_targets_k choose exactly `tg` (ascending, world - 1 of them): rank j repeats tg[j] 64 times, the last
    rank has no samples — the j * nvalid // world quantile of the 64 * (world - 1) valid samples lies in rank j - 1's run"""
    assert len(tg) == world - 1 and list(tg) == sorted(tg)
    rows = np.full((world, cm.META), 0, np.int64)
    for r in range(world):
        rows[r, :cm.SAMPLES] = tg[r] if r < world - 1 else INF
        rows[r, cm.SAMPLES:] = (1, r, 0, 0)
    return rows


def own_rows(ranks):
    """the rows the ranks would gather themselves (tbk_partial_stage_keys)"""
    return np.stack([cm.meta_row(r.key, 1, i) for i, r in enumerate(ranks)])


TABLE = {}
CHOOSE = {}
TILE = {}


def _table(name, doc, ranks, tg=None, allmeta=None, **edge):
    assert name not in TABLE
    def build():
        rk = ranks() if callable(ranks) else ranks
        return TableScene(name, doc, rk, rows_for_targets(len(rk), tg) if allmeta is None else allmeta(rk), **edge)
    TABLE[name] = build


@functools.lru_cache(maxsize=None)
def table(name):
    return TABLE[name]()


# ---- TABLE: no groups -------------------------------------------------------------------------------------------------------------------
_OTHER = rank_of(chain(1, 100, [True, False, True, True, False, True]))          # a small rank with four bundles on tid 1
_table("empty-one-rank", "one rank has no groups: its samples are 1 << 62, its list says -1, no horizon and no bundle",
       [EMPTY, _OTHER], allmeta=own_rows, empty=[0])
_table("empty-all-ranks", "no rank has a group: no valid sample, every target 1 << 62 and nothing to cut",
       [EMPTY, EMPTY, EMPTY], allmeta=own_rows, empty=[0, 1, 2], no_targets=True)

# ---- TABLE: few groups (sample indices i * ng // 64 repeat below 64 groups, leave groups out above) --------------------------------------------------
for _n in (1, 63, 64, 65):
    _r = [rank_of(chain(2, 50, [i % 3 == 0 for i in range(_n)])), rank_of(chain(2, 60, [i % 2 == 0 for i in range(_n)]))]
    _table("few-groups-%d" % _n, "both ranks hold %d groups: the samples i * ng // 64 %s" % (_n, "repeat" if _n < 64 else "are every group" if _n == 64 else "never reach the last group"),
           _r, allmeta=own_rows, ng=_n)

# ---- TABLE: where the target lies among the keys --------------------------------------------------------------------------------------
# tid 70000: three groups in one bundle, then a head held by three groups, a non-head, and two more bundles
_POS = rank_of([(BIG_TID, 100, 140), (BIG_TID, 110, 120), (BIG_TID, 130, 160),
                (BIG_TID, 200, 205), (BIG_TID, 200, 230), (BIG_TID, 200, 210), (BIG_TID, 220, 225),
                (BIG_TID, 300, 310), (BIG_TID, 400, 410)])
_POS2 = rank_of([(BIG_TID, 150, 170), (BIG_TID, 250, 260)])
for _name, _t, _doc, _idx0 in (
        ("target-below-first-key", K(BIG_TID, 50), "the target lies below every key of rank 0: idx0 = 0 and nothing lies before the first head (-1)", 0),
        ("target-above-last-key", K(BIG_TID, 500), "the target lies above every key of rank 0: idx0 == ng, no head, the word before is emax[ng - 1]", 9),
        ("target-on-head", K(BIG_TID, 300), "the target equals a key that opens a bundle", 7),
        ("target-on-non-head", K(BIG_TID, 130), "the target equals a key inside a bundle: the stretch up to the next head counts as before the target", 2),
        ("target-on-shared-key", K(BIG_TID, 200), "the target equals a key three groups hold: the lower bound takes the first of them, a head", 3)):
    _table(_name, _doc, [_POS, _POS2], tg=[_t], idx0=_idx0, tid=BIG_TID)


# ---- TABLE: 14 .. 17 heads behind the target -------------------------------------------------------------------------------------------
def _heads_rank(n):
    # three groups in one bundle before the target, then n bundles of two groups: the second reaches farther than the first
    g = [(3, 100, 150), (3, 120, 130), (3, 140, 180)]
    for b in range(n):
        g += [(3, 1000 + 100 * b, 1000 + 100 * b + 20), (3, 1000 + 100 * b + 10, 1000 + 100 * b + 60)]
    return rank_of(g)


for _n in (14, 15, 16, 17):
    _table("heads-%d" % _n, "%d bundle heads behind the target: %s" % (
        _n, "all listed, no horizon, the last pair ends at emax[ng - 1]" if _n <= 15 else
        "the 16th is the horizon, the 15th pair ends at emax[heads[15] - 1]" + (", the 17th is never seen" if _n == 17 else "")),
        [_heads_rank(_n), rank_of([(3, 1030, 1050), (3, 2455, 2500)])], tg=[K(3, 999)], heads=_n)


# ---- TABLE: where the walk's ballots place the heads --------------------------------------------------------------------------------
def _placed(offsets, total, before=100):
    """`before` groups in one bundle in front of the target (idx0 = before, no multiple of 256), then `total` groups with heads at the
    given offsets from idx0"""
    return rank_of(chain(4, 10, head_flags(before, [0]) + head_flags(total, offsets)))


def _placed_target(r, before=100):
    return int(r.key[before - 1]) + 1            # just behind the last group before idx0


_P1 = _placed([0, 63, 64, 255, 256, 257], 600)
_table("heads-at-wave-and-step-edges", "heads at offsets 0, 63, 64, 255, 256 and 257 from idx0 = 100: the last lane of a wave, the first of the next, "
       "the last lane of a step and the first two of the next", [_P1, _OTHER], tg=[_placed_target(_P1)], idx0=100, offsets=[0, 63, 64, 255, 256, 257])
_P2 = _placed(list(range(0, 150, 10)) + [255], 700)
_table("head16-last-lane-of-step", "the 16th head is the last lane of the first step: the walk ends there", [_P2, _OTHER], tg=[_placed_target(_P2)],
       idx0=100, head16=255)
_P3 = _placed(list(range(0, 150, 10)) + [256], 700)
_table("head16-first-lane-of-next-step", "the 16th head is the first lane of the second step: fifteen heads after the first step, the walk goes on",
       [_P3, _OTHER], tg=[_placed_target(_P3)], idx0=100, head16=256)
_P4 = _placed(list(range(256, 512)), 900)
_table("step-of-256-heads", "no head in the first step, 256 heads in the second (every lane of every wave): ranks beyond 15 are dropped",
       [_P4, _OTHER], tg=[_placed_target(_P4)], idx0=100, head16=271)

# ---- TABLE: a change of reference ---------------------------------------------------------------------------------------------------
_REF = rank_of([(5, 100, 2**31 - 2), (5, 200, 300), (6, 1, 50), (6, 30, 60), (BIG_TID, 1, 10)])
_table("reference-change", "the first group of the next reference is a head whatever reaches the end of the one before; the target lies exactly on "
       "(tid + 1) << 31 of reference 6", [_REF, rank_of([(5, 150, 160), (6, 70, 80)])], tg=[K(6, 0)], idx0=2)


# ---- TABLE: world sizes -------------------------------------------------------------------------------------------------------------
def _world_ranks(world, seed, empty=(), same=()):
    rng = np.random.default_rng(seed)
    ranks = []
    for r in range(world):
        if r in empty:
            ranks.append(EMPTY)
            continue
        if r in same:
            ranks.append(ranks[same[r]])
            continue
        n = int(rng.integers(3, 40))
        ranks.append(rank_of(chain(7 + int(rng.integers(0, 2)) * (BIG_TID - 7), int(rng.integers(1, 500)), (rng.random(n) < 0.5).tolist(),
                                   length=int(rng.integers(2, 30)), gap=int(rng.integers(2, 40)))))
    return ranks


for _w, _empty, _same in ((2, (), {}), (3, (1,), {}), (5, (0, 3), {4: 2}), (64, (0, 7, 31, 32, 63), {9: 8, 10: 8, 40: 20})):
    _rk = functools.partial(_world_ranks, _w, 1000 + _w, _empty, _same)
    _table("world-%d" % _w, "world %d with the ranks' own samples (%d of them, padded to a power of two for the sort)%s" % (
        _w, 64 * _w, "; ranks %s have none, ranks %s repeat another's" % (list(_empty), sorted(_same)) if _empty else ""),
        _rk, allmeta=own_rows, world=_w)


# ---- TABLE: the give-up limit (built where it is used: two arrays of 2^22 words) -------------------------------------------------------
def limit_scene(extra):
    """three groups before the target, then ONE bundle of 2^22 (+ extra) groups, one base apart, all reaching the same far end.
    Returns (key0, n, endk0, far): rank 0 = the three groups (key0[:3], endk0[:3]) followed by keys key0[3] + i, i < n, with keyed
    end `far`; rank 1 is small.  extra = 0: the walk runs off the end after 2^22 groups, no horizon; extra = 1: it gives up on the
    last group, whose key is the horizon."""
    n = cm.LIMIT + extra
    head = rank_of([(8, 10, 20), (8, 12, 30), (8, 15, 18)])
    first = K(8, 1000)
    far = K(8, 1000 + 2 * cm.LIMIT)
    return head, first, n, far


def limit_rank_np(extra):
    head, first, n, far = limit_scene(extra)
    return Rank(np.concatenate([head.key, first + np.arange(n, dtype=np.int64)]), np.concatenate([head.endk, np.full(n, far, np.int64)]))


# rank 1 reaches across the target, starts once inside the long bundle and once beyond its far end: that last start is the smallest clean
# key — without a horizon the lists settle on it, with the horizon of the give-up limit in front of it they cannot
LIMIT_BEYOND = 1000 + 2 * cm.LIMIT + 100
LIMIT_OTHER = rank_of([(8, 500, 1500), (8, 2000, 2100), (8, LIMIT_BEYOND, LIMIT_BEYOND + 50)])
LIMIT_TARGET = K(8, 1000)


# ---- CHOOSE: gathered lists written by hand ---------------------------------------------------------------------------------------------
def L(before, horizon=INF, pairs=()):
    """one rank's list for one cut"""
    out = np.empty(cm.CAND, np.int64)
    out[0], out[1] = before, horizon
    out[2::2], out[3::2] = INF, -1
    assert len(pairs) <= cm.BUNDLES
    for b, (s, e) in enumerate(pairs):
        out[2 + 2 * b], out[3 + 2 * b] = s, e
    return out


# the tiny tile whose groups the table of the exchange counts: (tid, 0-based position, CIGAR) per read, two files; the 1-based starts
# are 100, 200 (four groups), 300, 400 on reference TA and 10, 50 (two groups), 90 on reference TB
M_, N_, S_ = 0, 3, 4
TA, TB = 1, 2                   # the tiny tile's references: every key of the choose scenes lies above 2^32
CHOOSE_FILES = [
    [(TA, 99, [(30, M_)]), (TA, 199, [(10, M_)]), (TA, 199, [(20, M_), (50, N_), (10, M_)]), (TA, 199, [(30, M_)]), (TA, 299, [(5, S_), (20, M_)]),
     (TA, 399, [(25, M_)])],
    [(TA, 199, [(40, M_)]), (TB, 9, [(30, M_)]), (TB, 49, [(10, M_), (5, N_), (10, M_)]), (TB, 49, [(12, M_)]), (TB, 89, [(30, M_)])],
]
CARRY, N_FILES, FIRST_FIDX = 2**40 + 7, 37, 1234


def choose_tile():
    from helpers import tile_from_records
    return tile_from_records([[(t, p, 0, 60, "+", 1, c) for t, p, c in f] for f in CHOOSE_FILES])


def k0(s):
    return K(TA, s)


class ChooseScene:
    def __init__(self, name, doc, targets, lists, cuts, unsettled, raw_cuts=None):
        """lists[rank][cut]; cuts = what the scene claims comes out (after the ordering pass), raw_cuts = before it"""
        self.name, self.doc, self.world = name, doc, len(lists)
        self.targets = np.asarray(targets, np.int64)
        self.allcands = np.stack([np.stack(per_cut) for per_cut in lists])
        assert self.allcands.shape == (self.world, self.world - 1, cm.CAND)
        self.cuts, self.unsettled, self.raw_cuts = np.asarray(cuts, np.int64), unsettled, raw_cuts

    def __repr__(self):
        return "ChooseScene(%s: world %d)" % (self.name, self.world)


def _choose(name, doc, targets, lists, cuts, unsettled=False, raw_cuts=None):
    assert name not in CHOOSE
    CHOOSE[name] = ChooseScene(name, doc, targets, lists, cuts, unsettled, raw_cuts)


_choose("target-clean", "the target is beyond every rank's reach — rank 1's by one unit (reach x - 1) — and wins over every bundle start",
        [k0(250)], [[L(k0(240), INF, [(k0(301), k0(350)), (k0(401), k0(450))])], [L(k0(249), INF, [(k0(260), k0(300))])]], [k0(250)])
_choose("target-reached-by-one", "rank 1 reaches exactly the target (reach x): not clean, its next bundle start takes the cut",
        [k0(250)], [[L(k0(240), INF, [(k0(301), k0(350)), (k0(401), k0(450))])], [L(k0(250), INF, [(k0(260), k0(300))])]], [k0(260)])
_choose("third-rank-wins", "rank 0 blocks the target and rank 1's start, rank 1 blocks rank 0's start: the start of rank 2, which blocks nothing, wins",
        [k0(100), k0(100)], [[L(k0(190), INF, [(k0(201), k0(260))])] * 2, [L(k0(90), INF, [(k0(180), k0(220))])] * 2, [L(k0(50), INF, [(k0(301), k0(350))])] * 2],
        [k0(301), k0(301)])
_R1_15 = [(k0(110 + 10 * b), k0(115 + 10 * b)) for b in range(15)]
_choose("candidate-on-horizon", "rank 0's start equals rank 1's horizon: it is still judged (x > horizon is false), from the 15th pair's end",
        [k0(100)], [[L(k0(300), INF, [(k0(401), k0(450))])], [L(k0(90), k0(401), _R1_15)]], [k0(401)])
_choose("candidate-beyond-horizon", "rank 0's start lies one beyond rank 1's horizon: skipped, nothing else qualifies, the cut stays unsettled",
        [k0(100)], [[L(k0(300), INF, [(k0(401), k0(450))])], [L(k0(90), k0(400), _R1_15)]], [INF], unsettled=True)
_choose("nothing-qualifies", "rank 0 reaches across the target and every listed start, no horizon anywhere: 1 << 62 and flag bit 1",
        [k0(100)], [[L(k0(1000))], [L(k0(90), INF, [(k0(200), k0(230)), (k0(300), k0(320))])]], [INF], unsettled=True)
_choose("all-targets-inf", "no samples anywhere: every cut 1 << 62 and no flag, whatever the lists say",
        [INF, INF], [[L(-1), L(-1)], [L(k0(1000)), L(k0(1000))], [L(-1), L(-1)]], [INF, INF])
_choose("two-targets-one-bundle-w3", "both targets fall inside one long bundle of rank 0: both cuts land on rank 1's start behind it, destination 1 gets nothing",
        [k0(150), k0(250)], [[L(k0(299), INF, [(k0(400), k0(425))]), L(k0(299), INF, [(k0(400), k0(425))])],
                             [L(k0(130), INF, [(k0(300), k0(330))]), L(k0(130), INF, [(k0(300), k0(330))])],
                             [L(-1), L(-1)]], [k0(300), k0(300)])
_choose("two-targets-one-bundle-w5", "world 5: targets 2 and 3 fall inside one bundle of rank 4 and share a cut; the last cut lies beyond this rank's last key",
        [k0(150), k0(210), k0(250), K(TB, 60)],
        [[L(-1)] * 4, [L(k0(140)), L(k0(140), INF, [(K(TB, 10), K(TB, 40))]), L(k0(140), INF, [(K(TB, 10), K(TB, 40))]), L(K(TB, 62), INF, [(K(5, 10), K(5, 20))])],
         [L(-1)] * 4, [L(-1)] * 4,
         [L(k0(149)), L(k0(430)), L(k0(430)), L(K(TB, 59))]], [k0(150), K(TB, 10), K(TB, 10), K(5, 10)])
_choose("earlier-cut-lowered", "the lists of cut 0 judge rank 1's reach before start 200 as 250, those of cut 1 as 160: cut 0 comes out behind cut 1 and is "
        "lowered to it — a key four groups hold, which all go right",
        [k0(100), k0(150)], [[L(k0(120), INF, [(k0(200), k0(230)), (k0(300), k0(320))]), L(k0(120), INF, [(k0(200), k0(230)), (k0(300), k0(320))])],
                             [L(k0(250)), L(k0(160))], [L(k0(99)), L(k0(99))]], [k0(200), k0(200)], raw_cuts=[k0(300), k0(200)])



def _w64_lists():
    """world 64: rank 0 reaches across every target; the only clean start of cut 0 is rank 17's first pair, of cut 1 rank 40's 15th pair, of
    the last cut rank 63's 15th pair; every other cut finds rank 1's first pair"""
    blocked = [(k0(151 + b), k0(166)) for b in range(14)]              # fourteen starts inside rank 0's reach
    lists = [[L(-1) for _ in range(63)] for _ in range(64)]
    lists[0] = [L(k0(190)) for _ in range(63)]
    for c in range(2, 62):
        lists[1][c] = L(k0(90), INF, [(k0(300), k0(320))])
    lists[17][0] = L(k0(90), INF, [(k0(200), k0(230))])
    lists[40][1] = L(k0(90), INF, blocked + [(k0(300), k0(320))])
    lists[63][62] = L(k0(90), INF, blocked + [(K(TB, 50), K(TB, 70))])
    return lists


W64_WINNERS = {0: 1 + 17 * 15, 1: 1 + 40 * 15 + 14, 62: 1 + 63 * 15 + 14}       # cut -> index of its only clean candidate among the 961
_choose("world-64-winners-beyond-256", "world 64, 961 candidates per cut judged by 256 threads: the only clean candidate of three cuts is number 256 (the "
        "first of the second pass), 615 (third pass) and 960 (the last of all)",
        [k0(150)] * 63, _w64_lists(), [k0(200)] + [k0(300)] * 61 + [K(TB, 50)])


# ---- TILE: real reads ----------------------------------------------------------------------------------------------------------------------
class TileScene:
    """groups[rank] = (tid, start, end) triples in order, one read each; flags[rank] (optional) = the BAM flag of that rank's reads"""

    def __init__(self, name, doc, groups, flags=None, **edge):
        self.name, self.doc, self.world, self.edge = name, doc, len(groups), edge
        self.reads = [sorted(set(map(tuple, g))) for g in groups]
        assert all(len(a) == len(b) for a, b in zip(self.reads, groups)), "one read per group"
        self.flags = flags or [0] * self.world
        self.groups = [[] if self.flags[r] else self.reads[r] for r in range(self.world)]     # what passes the filters

    def ranks(self):
        return [rank_of(g) for g in self.groups]

    def files(self):
        return [[(t, s - 1, self.flags[r], 60, "+", 1, [(e - s + 1, M)]) for t, s, e in self.reads[r]] for r in range(self.world)]

    def tile(self):
        from helpers import tile_from_records
        return tile_from_records(self.files())

    def __repr__(self):
        return "TileScene(%s: world %d, reads %s)" % (self.name, self.world, [len(g) for g in self.reads])


def _tile(name, doc, groups, **kw):
    assert name not in TILE
    TILE[name] = lambda: TileScene(name, doc, groups() if callable(groups) else groups, **kw)


@functools.lru_cache(maxsize=None)
def tile(name):
    return TILE[name]()


STAIR_LENGTHS = (4, 12, 20, 24, 26, 27, 28, 29, 30, 31, 32, 33, 34, 36, 40, 60)


def _staircase(n):
    # rank 0: reads [1000 + 100 k, + 60), rank 1: [1050 + 100 k, + 60): every bundle of one rank bridges two of the other, n links long
    r0 = [(0, 11 + 5 * i, 40 + 5 * i) for i in range(40)] + [(0, 1001 + 100 * k, 1060 + 100 * k) for k in range(n)] + \
         [(0, 20001 + 7 * i, 20030 + 7 * i) for i in range(40)]
    r1 = [(0, 13 + 5 * i, 42 + 5 * i) for i in range(40)] + [(0, 1051 + 100 * k, 1110 + 100 * k) for k in range(n)] + \
         [(0, 20002 + 7 * i, 20031 + 7 * i) for i in range(40)]
    return [r0, r1]


for _n in STAIR_LENGTHS:
    _tile("staircase-%d" % _n, "two ranks whose bundles interlock for %d links between two piles" % _n, functools.partial(_staircase, _n), links=_n)


def _loci(tid, n, first, step, per, length, shift=0):
    return [(tid, first + step * i + 3 * j + shift, first + step * i + 3 * j + shift + length - 1) for i in range(n) for j in range(per)]


_tile("filtered-rank", "the middle rank's reads are all secondary alignments: filtered out, no groups, samples 1 << 62",
      [_loci(0, 60, 100, 500, 3, 40), _loci(0, 50, 130, 500, 2, 40), _loci(0, 60, 140, 500, 3, 40, shift=1)], flags=[0, 0x100, 0])
_tile("two-references", "as many groups on reference 0 as on reference 2: the cut falls on the first start of reference 2, across the empty reference 1",
      [_loci(0, 40, 100, 300, 2, 50) + _loci(2, 40, 100, 300, 2, 50), _loci(0, 40, 120, 300, 2, 50) + _loci(2, 40, 120, 300, 2, 50)])


def _touching(lead=3):
    # per locus: A on rank 0, B on rank 1 from A's end + 1 (touches: same bundle), C on rank 0 from B's end + 1, D on rank 1 from C's end + 1,
    # E on rank 0 from D's end + 2 (clean); `lead` reads in front on rank 0 move the median sample onto a touching start
    r0, r1 = [(1, 10 + 60 * i, 30 + 60 * i) for i in range(lead)], []
    for i in range(100):
        b = 1000 * (i + 1)
        r0 += [(1, b + 100, b + 149), (1, b + 200, b + 249), (1, b + 301, b + 350)]
        r1 += [(1, b + 150, b + 199), (1, b + 250, b + 299)]
    return [r0, r1]


_tile("touching-reads", "reads that start at another rank's end + 1 on both sides of the target: not clean; the first start at end + 2 is", _touching)
_tile("few-groups", "ranks of 1, 63, 64 and 65 groups: the sample indices i * ng // 64 of tbk_partial_stage_keys",
      [_loci(2, 1, 500, 100, 1, 30), _loci(2, 63, 100, 100, 1, 30), _loci(2, 32, 120, 200, 2, 30), _loci(2, 65, 90, 100, 1, 30)])
_tile("scan-tiles", "4,300 groups per rank (more than two scan tiles of 2,048) with one read early on that reaches across them: the running maximum "
      "of the ends is carried from tile to tile",
      lambda: [[(0, 50, 45000)] + _loci(0, 4299, 100, 10, 1, 8) + [(0, 50000, 50010)], _loci(0, 4300, 103, 10, 1, 8) + [(1, 5, 10)]], big=True)

# ---- TILE: seeded random scenes — loci separated by gaps common to all ranks ---------------------------------------------------------------
RANDOM_SEEDS = tuple(range(40))
RANDOM_WORLDS = (2, 3, 5, 8)


def random_groups(seed):
    """world from RANDOM_WORLDS, sometimes an empty rank; loci of several islands per rank — many short ones in some loci, so that a
    rank's list runs out before the locus ends — with a gap behind every locus that no rank's read crosses"""
    rng = np.random.default_rng(seed)
    world = RANDOM_WORLDS[seed % len(RANDOM_WORLDS)]
    empty = set(rng.choice(world, size=int(rng.integers(0, 2)) if world > 2 else 0, replace=False).tolist())
    groups = [set() for _ in range(world)]
    pos, tid = 100, 0
    for locus in range(int(rng.integers(30, 60))):
        if rng.random() < 0.05:
            tid, pos = tid + 1 + int(rng.integers(0, 2)), 100
        long_locus = rng.random() < 0.1
        width = int(rng.integers(2000, 4000)) if long_locus else int(rng.integers(200, 900))
        cover = np.zeros(width + 400, bool)
        for r in range(world):
            if r in empty:
                continue
            for _ in range(int(rng.integers(20, 40)) if long_locus else int(rng.integers(1, 12))):
                s = int(rng.integers(0, width))
                ln = int(rng.integers(20, 60))
                groups[r].add((tid, pos + s, pos + s + ln - 1))
                cover[s:s + ln] = True
        if long_locus and world > 1:          # one rank's long reads tie the locus together so that no start inside it is clean
            r = int(rng.choice([x for x in range(world) if x not in empty]))
            for s in range(0, width, 150):
                groups[r].add((tid, pos + s, pos + s + 199))
        pos += width + 400 + int(rng.integers(10, 300))
    return [sorted(g) for g in groups]


for _s in RANDOM_SEEDS:
    _tile("random-%d" % _s, "seeded random loci, seed %d" % _s, functools.partial(random_groups, _s), random=True)

TILE_NAMED = [n for n in TILE if not n.startswith("random-") and not n.startswith("staircase-")]
RANDOM = ["random-%d" % s for s in RANDOM_SEEDS]
STAIRS = ["staircase-%d" % n for n in STAIR_LENGTHS]


# ---- what the model says of a tile scene (shared by the CPU and the GPU tests) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def verdict(name):
    """(targets, allcands [world][world - 1][CAND], raw per-cut (cut, unsettled), cuts after the ordering pass, flag bit 1) of a tile scene"""
    s = tile(name)
    ranks = s.ranks()
    allmeta = own_rows(ranks)
    per = [cm.stage_cands(r.key, r.emax, allmeta, s.world) for r in ranks]
    tg = per[0][0]
    allc = np.stack([p[1] for p in per])
    raw = [cm.choose(allc[:, c, :], int(tg[c])) for c in range(s.world - 1)]
    cuts, flag = cm.stage_choose(allc, tg)
    return tg, allc, raw, cuts, flag


def stair_edge():
    """(the longest staircase the lists still settle, the shortest they give up) — the model decides"""
    settled = [n for n in STAIR_LENGTHS if not verdict("staircase-%d" % n)[4]]
    given_up = [n for n in STAIR_LENGTHS if verdict("staircase-%d" % n)[4]]
    return max(settled), min(given_up)
