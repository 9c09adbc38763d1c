"""Hand-built tiles for the compaction of the raw window form (wg_compact_k and wg_tie_k, tiebrush_amd/csrc/wgroup.hip) in its lean
form, where wg_tie_k takes a set member's values from window space — entry (group - first group of the window) — and the YD stage the
caller's representatives by output place.  What can go wrong there depends on where groups, tie sets, windows and listed records fall
relative to the rounds of 64 lanes and to blocks of 256 output groups (the unit of a layout by output, which was measured and is not
kept: DESIGN.md §8), so every scene is a list of GROUPS in key order — (records, CIGAR, same start as the group before) — which is
also the output order except inside a tie set, and whose record counts place the windows: with one file a window opens at every
record 1024 j whose key differs from the key before it (window_model.py).

tests/test_compact_scenes_cpu.py proves every scene's claim from the oracle and the model; tests/test_gpu_compact_lean.py runs the
scenes.  A scene and its oracle result are built once per process."""
import functools

import numpy as np

import window_scenes as ws

M, I, D, N = 0, 1, 2, 3
BLOCK = 256
PLAIN, LONG, HASHED, PAIR_A, PAIR_B, TIE0 = 0, 1, 2, 3, 4, 5
# members of a tie set: equal (tid, start, strand, end), different CIGARs — a M b D c M of span 40 (hashed key words); LONG has five
# operations on span 40 (the reference comparator puts it behind every tie shape); HASHED is an insertion (no exact key word)
TIE_SHAPES = [ws.cw((a, M), (b, D), (40 - a - b, M)) for a in range(1, 21) for b in range(1, 11)]
SHAPES = [ws.mm(40), ws.cw((10, M), (5, N), (10, M), (5, N), (10, M)), ws.cw((20, M), (2, I), (20, M)), ws.PAIR_A, ws.PAIR_B] + TIE_SHAPES
# three exons on span 40, each member its own exon coordinates: far groups (no item word says their exons), whose representative the
# YD stage fetches — a set of them tells whether it fetches the representative of the group at that OUTPUT place
FAR_SHAPES = [ws.cw((a, M), (5, N), (b, M), (5, N), (30 - a - b, M)) for a, b in ((4, 4), (6, 8), (8, 6), (10, 10), (12, 4), (5, 12), (3, 20), (14, 9))]
FAR0 = len(SHAPES)
SHAPES = SHAPES + FAR_SHAPES


def groups(G, cnt=1):
    """G groups of cnt records 40M, each on a start of its own"""
    return dict(cnt=np.full(G, cnt, np.int64), shape=np.zeros(G, np.int64), new=np.ones(G, bool))


def tie(g, *sets):
    """the groups at the indices of every tuple (consecutive) share the start of the tuple's first group; member j takes tie shape
    (7 j + 3) % 200, so a set's key order is not its output order"""
    for t in sets:
        for j, i in enumerate(t):
            g["shape"][i] = TIE0 + (7 * j + 3) % len(TIE_SHAPES)
            g["new"][i] = j == 0
    return g


def cat(*gs):
    return {key: np.concatenate([g[key] for g in gs]) for key in ("cnt", "shape", "new")}


def run(a, n):
    return tuple(range(a, a + n))


def tile_of(g, k=1):
    pos = 100 + 3 * (np.cumsum(g["new"]) - 1)
    return ws.tile_of(ws.deal(k, 0, np.repeat(pos, g["cnt"]), np.repeat(g["shape"], g["cnt"])), SHAPES)


# ---- the scenes: name -> (groups, claim) ---------------------------------------------------------------------------------------------
# A claim is checked by test_compact_scenes_cpu.py (the keys are explained there); every scene is of one file unless the tests deal it.
SCENES = {}


def scene(name, **claim):
    def reg(fn):
        SCENES[name] = (fn, claim)
        return fn
    return reg


for _n in (1, 255, 256, 257, 511, 512, 513):            # three records per group: 513 groups are 1539 records, two windows with groups
    scene("ng-%d" % _n, ng=_n)(functools.partial(groups, _n, 3))

N_LINE = 3 * 1024 + 500                                  # single-record groups: windows of 1024 groups open at groups 1024, 2048, 3072


def _shifted(d):
    """the first d groups hold two records: window 0 has 1024 - d groups, every later window begins d groups ahead of a block"""
    g = groups(N_LINE)
    g["cnt"][:d] = 2
    return g


scene("windows-on-blocks", ng=N_LINE, window_starts=[0, 1024, 2048, 3072], blocks_of_a_window=4)(functools.partial(_shifted, 0))
scene("windows-one-before-blocks", ng=N_LINE, window_starts=[0, 1023, 2047, 3071], blocks_of_a_window=5)(functools.partial(_shifted, 1))
scene("windows-one-behind-blocks", ng=N_LINE, window_starts=[0, 769, 1793, 2817], blocks_of_a_window=5)(functools.partial(_shifted, 255))

TIE_PLACES = {
    "ties-255-256": [(255, 256)],
    "ties-254-257": [run(254, 4)],
    "ties-256-258": [run(256, 3)],
    # sets on the first and the last groups of windows that end on a multiple of 256
    "ties-window-ends": [(0, 1), (1022, 1023), (1024, 1025), run(2045, 3), run(2048, 3), (N_LINE - 2, N_LINE - 1)],
    # a set in every quarter of a window of 1024 groups
    "ties-every-block": [(1024 + 10, 1024 + 11), run(1024 + 300, 3), (1024 + 600, 1024 + 601), run(1024 + 1000, 4)],
}
for _name, _sets in TIE_PLACES.items():
    scene(_name, ng=N_LINE, tie_sets=[(t[0], len(t)) for t in _sets])(functools.partial(lambda s: tie(groups(N_LINE), *s), _sets))


@scene("head-opens-a-block", ng=N_LINE, tie_sets=[(256, 2), (1024 + 512, 2)], long_at=[255, 1024 + 511])
def _head_opens_a_block():
    """The head of a set is lane 0 of a round (and the first group of a block of 256) and not the first group of its window, so its flag
    hangs on the carried key; the group before it is LONG: five operations on span 40, on a start of its own.  A head wrongly flagged
    as a follower would draw LONG into the set, where the reference comparator puts it behind the members (fewer operations first): it
    would leave its place.  (A follower in lane 0 is in 'ties-255-256' and 'ties-254-257'.)"""
    g = tie(groups(N_LINE), (256, 257), (1024 + 512, 1024 + 513))
    g["shape"][[255, 1024 + 511]] = LONG
    return g


@scene("ties-of-far-groups", ng=N_LINE, tie_sets=[(40, 8), (1024 + 100, 8)])
def _ties_of_far_groups():
    """two sets of eight groups of three exons each, every member with exon coordinates of its own (one, two, .. eight records): the
    members' places in the output are not their places in key order, and what the YD stage computes hangs on whose exons it walks"""
    g = tie(groups(N_LINE), run(40, 8), run(1024 + 100, 8))
    for a in (40, 1024 + 100):
        g["shape"][a:a + 8] = FAR0 + np.arange(8)
        g["cnt"][a:a + 8] = 1 + np.arange(8)
    return g


PILE = 154000                                            # identical records on one base: 150 equal splitters, some 300 empty windows


def _pile(where):
    one = dict(cnt=np.array([PILE]), shape=np.zeros(1, np.int64), new=np.ones(1, bool))
    line = tie(groups(700), (255, 256), (698, 699))
    return {"start": cat(one, line), "middle": cat(line, one, tie(groups(700), (0, 1))), "end": cat(line, one)}[where]


for _w in ("start", "middle", "end"):
    scene("empty-windows-at-the-%s" % _w, empty_run=290)(functools.partial(_pile, _w))


@scene("one-group-windows", ng=600, windows_in_a_block=[255, 256], listed_windows=500)
def _one_group_windows():
    """groups of 1024 identical records: every window with groups holds one — except the first, of two (512 records each), and one of two
    that lies across groups 511 | 512 — and an empty window follows each: block 0 meets 255 windows with groups, block 1 256 (no block
    can meet more: every such window but the first has its first group inside the block), walking more than 500 windows for them"""
    g = groups(600, 1024)
    g["cnt"][[0, 1, 511, 512]] = 512
    return tie(g, (255, 256))


ENTRIES = (0, 1, 64, 65, 256, 257)                       # listed records (hashed key words) of windows 0 .. 5 of the verify scenes
BIG_LIST = 1500                                          # ... and of the pile-up window behind them


def _verify(pair_in=None):
    """Window j holds ENTRIES[j] listed records: identical hashed reads two to a start (half of the entries are compared with another
    record), behind ten plain groups; the rest of its 1024 records are plain groups of one.  Then 1500 identical hashed reads on one
    base (one group, one window, more than 1024 entries) and 300 plain groups.  pair_in = j: the last two entries of window j are
    PAIR_A and PAIR_B on one start — two groups, a tie set; one key once the hash is masked away."""
    parts = []
    for j, e in enumerate(ENTRIES):
        cnt, shape, new = [2] * (e // 2) + [1] * (e % 2), [HASHED] * (e // 2 + e % 2), [True] * (e // 2 + e % 2)
        if pair_in == j:
            i = e // 2 - 1
            cnt[i:i + 1], shape[i:i + 1], new[i:i + 1] = [1, 1], [PAIR_A, PAIR_B], [True, False]
        h = dict(cnt=np.array(cnt, np.int64), shape=np.array(shape, np.int64), new=np.array(new, bool))
        parts += [groups(10), h, groups(1024 - 10 - e)]
    big = dict(cnt=np.array([BIG_LIST]), shape=np.array([HASHED]), new=np.ones(1, bool))
    return cat(*(parts + [big, groups(300)]))


scene("listed-records", entries=list(ENTRIES) + [BIG_LIST], split_listed_window=True)(_verify)
for _j in (3, 5):
    scene("collision-among-%d" % ENTRIES[_j], entries=list(ENTRIES) + [BIG_LIST], collision=True)(functools.partial(_verify, _j))


@functools.lru_cache(maxsize=None)
def get(name, k=1):
    return tile_of(SCENES[name][0](), k)


@functools.lru_cache(maxsize=None)
def oracle(name, k=1):
    from oracle import oracle_ffi as orc
    return orc.collapse(get(name, k), want_rec_group=True, strategy=0)


def output_tie_sets(res):
    """(first output place, members) of every tie set of several groups: runs of equal (start, end) in the output (one reference, one
    strand in these scenes)"""
    s, e = np.asarray(res["g_start"]), np.asarray(res["g_end"])
    head = np.ones(len(s), bool)
    head[1:] = (s[1:] != s[:-1]) | (e[1:] != e[:-1])
    first = np.flatnonzero(head)
    size = np.diff(np.concatenate([first, [len(s)]]))
    return [(int(a), int(n)) for a, n in zip(first, size) if n > 1]
