"""Hand-placed record streams for tbk_cov_stream_push (tiebrush_amd/csrc/stream.hip).  numpy only; importable without a GPU.

A scene is a list of pushes — (tile, final, tag_seen or None) — and what the scene is there for, stated by hand: `expect`, the info of
every push (n_view, n_carry, n_taken, cut).  tests/test_stream_model_cpu.py proves the statements with the model (stream_model.py) and
holds the rows of the views, one after the other, against the rows of the uncut stream (cov_scenes.model, per base);
tests/test_gpu_cov_stream.py then runs every scene on the device.

The passes that look for the last head walk carry and tile in blocks of T = CB_TILE records (a thread four records, a wave 256, a row
1024); the aggregates of the blocks meet in one spine.  The sizes below put heads, and the long read that decides them, on those edges."""
import numpy as np

import cov_scenes as cs
import stream_model as sm

M, I, D, N, S = cs.M, cs.I, cs.D, cs.N, cs.S
T = cs.CB_TILE            # records per block of the head passes (cb_tiles.hpp: CB_NT * 4 * CB_ROWS)
UNMAPPED = (0, 0, 4, [(33, M), (70, N), (5, M)], 9.0, "+")      # flag 4 with a CIGAR and a YC of its own: must never count


def rd(tid, pos, ln, yc=1.0, strand="."):
    return (tid, pos, 0, [(ln, M)], yc, strand)


def chain(tid, pos, k):
    """k reads of 3 bases, 2 apart: each starts inside the one before — one bundle, only the first can be a head"""
    return [rd(tid, pos + 2 * q, 3) for q in range(k)]


def sparse(tid, pos, k):
    """k reads of 3 bases, 10 apart: each starts beyond its neighbour's end — every one a head unless an earlier, longer read covers it"""
    return [rd(tid, pos + 10 * q, 3) for q in range(k)]


def info(n_view, n_carry, n_taken, cut):
    return dict(n_view=n_view, n_carry=n_carry, n_taken=n_taken, cut=cut)


class Scene:
    def __init__(self, name, tiles, expect, finals=None, seen=None, yx=True, num_samples=5):
        """tiles: lists of record tuples; the last push is final unless `finals` says otherwise"""
        self.name, self.expect, self.num_samples = name, expect, num_samples
        finals = finals if finals is not None else [False] * (len(tiles) - 1) + [True]
        seen = seen if seen is not None else [None] * len(tiles)
        self.pushes, k = [], 0
        for recs, f, sn in zip(tiles, finals, seen):
            n = len(recs)
            self.pushes.append((cs.mk(recs, (1 + (7 * np.arange(k, k + n, dtype=np.int64)) % num_samples) if yx else None), f,
                                None if sn is None else np.asarray(sn, np.uint8)))
            k += n
        assert len(expect) == len(tiles), name

    def __repr__(self):
        return self.name


def _small():
    out = []
    # a read at start == running max(end): no head; at max(end) + 1: a head.  a = [101, 150], b starts at 150, c at 200 = end(b) + 1
    a, b, c = rd(0, 100, 50), rd(0, 149, 50), rd(0, 199, 10)
    out.append(Scene("touch_then_gap", [[a, b, c]], [info(3, 0, 3, 3)]))
    out.append(Scene("touch_then_gap/cut", [[a, b, c], []], [info(2, 1, 2, 2), info(1, 0, 0, 0)]))
    out.append(Scene("touch_only", [[a, b], [rd(0, 198, 10)], []], [info(0, 2, 0, 0), info(0, 3, 0, 0), info(3, 0, 0, 0)]))
    # a long early read covers many later short ones: the running maximum decides, not the neighbour's end
    long_ = rd(0, 1000, 500)                                   # [1001, 1500]
    cov = sparse(0, 1010, 40)                                  # the last one ends at 1403
    out.append(Scene("long_covers", [[rd(0, 10, 5), long_] + cov + [rd(0, 1499, 5), rd(0, 1504, 5), rd(0, 1600, 5)]],
                     [info(45, 0, 45, 45)]))
    out.append(Scene("long_covers/cut", [[rd(0, 10, 5), long_] + cov[:20], cov[20:] + [rd(0, 1499, 5)], [rd(0, 1504, 5), rd(0, 1600, 5)], []],
                     [info(1, 21, 1, 1), info(0, 42, 0, 0), info(43, 1, 1, 1), info(1, 0, 0, 0)]))
    # a spliced read: its intron spans a gap in which short reads would otherwise open bundles
    sp = (0, 2000, 0, [(50, M), (1000, N), (50, M)], 2.0, "+")  # [2001, 3100]
    inside = sparse(0, 2200, 5)
    out.append(Scene("spliced_spans_gap", [[sp] + inside[:2], inside[2:] + [rd(0, 3099, 5), rd(0, 3104, 5)], []],
                     [info(0, 3, 0, 0), info(7, 1, 4, 4), info(1, 0, 0, 0)]))
    # the reference changes to a lower position: a head whatever the maximum was
    out.append(Scene("tid_change_lower", [[rd(0, 5000, 100), rd(0, 5050, 100)], [rd(1, 10, 5), rd(1, 12, 5)], []],
                     [info(0, 2, 0, 0), info(2, 2, 0, 0), info(2, 0, 0, 0)]))
    # unmapped records before, between and after: dropped, never a head, never in a carry; `cut` counts them as tile records
    u = UNMAPPED
    out.append(Scene("unmapped_around", [[u, u, rd(0, 100, 10), u, rd(0, 105, 10), u], [u, rd(0, 300, 10), u, rd(0, 400, 5), u, u], [u]],
                     [info(0, 2, 0, 2), info(3, 1, 1, 3), info(1, 0, 0, 1)]))
    # a head at index 0 only: everything carries, over pushes, until `final`
    out.append(Scene("head0_only", [chain(0, 100, 9)], [info(0, 9, 0, 0)], finals=[False]))
    out.append(Scene("carry_grows", [chain(0, 100, 9), chain(0, 118, 7), chain(0, 132, 5), []],
                     [info(0, 9, 0, 0), info(0, 16, 0, 0), info(0, 21, 0, 0), info(21, 0, 0, 0)]))
    # the last head at tile index n - 1
    out.append(Scene("head_last", [chain(0, 100, 6) + [rd(0, 500, 5)], chain(0, 502, 3) + [rd(0, 900, 5)], []],
                     [info(6, 1, 6, 6), info(4, 1, 3, 3), info(1, 0, 0, 0)]))
    # a tile of unmapped records only, with and without a carry; an empty tile with a carry
    out.append(Scene("unmapped_only", [[u, u, u], [rd(0, 100, 10)], [u, u], [], []],
                     [info(0, 0, 0, 0), info(0, 1, 0, 0), info(0, 1, 0, 0), info(0, 1, 0, 0), info(1, 0, 0, 0)]))
    out.append(Scene("empty_stream", [[], []], [info(0, 0, 0, 0), info(0, 0, 0, 0)]))
    # every record a head: the view takes all but the last
    out.append(Scene("all_heads", [sparse(0, 100, 70), sparse(0, 900, 3), []], [info(69, 1, 69, 69), info(3, 1, 2, 2), info(1, 0, 0, 0)]))
    # a CIGAR without reference bases (S and I only): end = pos, the next read at pos + 1 is a head; D extends the end (a read
    # at the D read's last base is none, the one behind the end of that is)
    out.append(Scene("odd_cigars", [[(0, 100, 0, [(5, S), (3, I)], 1.0, "."), rd(0, 100, 5), (0, 103, 0, [(2, M), (10, D), (2, M)], 3.0, "-"), rd(0, 116, 4),
                                     rd(0, 120, 4)], []], [info(4, 1, 4, 4), info(1, 0, 0, 0)]))
    # tag presence: YC / YX count where tag_seen says so, 1.0 / 1 elsewhere (bit 0: YC, bit 1: YX)
    w = [rd(0, 100 + 10 * q, 50, yc=float(2 + q)) for q in range(4)] + [rd(0, 900, 5, yc=7.0)]
    out.append(Scene("tag_seen", [w, []], [info(4, 1, 4, 4), info(1, 0, 0, 0)], seen=[[0, 1, 2, 3, 3], None]))
    return out


def _sized(s):
    """tiles of exactly s records.  Tile 1: a chain whose LAST record (index s - 1) is a head.  Tile 2: a long read at index 0 — a head
    — and s - 1 sparse reads that only it covers: the last head of the tile is its first record, however many blocks the tile has."""
    t1 = chain(1, 1000, s - 1) + [rd(1, 1000 + 2 * s + 100, 4)]
    p = 1000 + 2 * s + 200
    t2 = [rd(1, p, 10 * s + 50)] + sparse(1, p + 5, s - 1)
    if s == 1:
        return Scene("size/1", [t1, t2, []], [info(0, 1, 0, 0), info(1, 1, 0, 0), info(1, 0, 0, 0)])
    return Scene("size/%d" % s, [t1, t2, []], [info(s - 1, 1, s - 1, s - 1), info(1, s, 0, 0), info(s, 0, 0, 0)])


def _spine(d, touch, split):
    """the deciding long read d records before the head: [chain x 5][LONG][sparse x (d - 1), covered by LONG alone][X][chain x 3] with X
    at LONG's end + 1 (a head; touch: at LONG's end — no head, the last head is LONG).  split: where the stream is cut into tiles."""
    p = 1000
    pre = chain(2, p, 5)
    long_ = rd(2, p + 100, 10 * d + 20, yc=2.0)              # [p + 101, p + 120 + 10 d]
    mid = sparse(2, p + 105, d - 1)                            # the last one ends at p + 105 + 10 (d - 2) + 3 < LONG's end
    xpos = p + 120 + 10 * d - (1 if touch else 0)
    tail = [rd(2, xpos, 4)] + chain(2, xpos + 2, 3)
    recs = pre + [long_] + mid + tail
    n, ih = len(recs), 5 + d
    cuts = [0] + [c for c in split if 0 < c < n] + [n]
    tiles = [recs[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [[]]
    # what every push must report: the last head among the records seen so far is 0, 5 (LONG) or ih (X, unless it only touches)
    heads_at = [0, 5] + ([] if touch else [ih])
    expect, taken_to = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        last = max(h for h in heads_at if h < b)
        if last > taken_to:                                  # a head behind the open bundle's own: it lies in this tile
            assert last >= a
            expect.append(info(last - taken_to, b - last, last - a, last - a))
            taken_to = last
        else:
            expect.append(info(0, b - taken_to, 0, 0))
    expect.append(info(n - taken_to, 0, 0, 0))
    return Scene("spine/%d/%s/%s" % (d, "touch" if touch else "gap", "-".join(map(str, split)) or "whole"), tiles, expect)


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, T - 1, T, T + 1, 3 * T + 1)


def scenes():
    out = _small() + [_sized(s) for s in SIZES]
    for d in (T, 2 * T):
        for touch in (False, True):
            out.append(_spine(d, touch, []))                 # one tile: LONG and X in different blocks of the TILE
            out.append(_spine(d, touch, [6]))                # LONG alone in the carry
            out.append(_spine(d, touch, [5 + d]))            # the carry fills whole blocks exactly (d records); X is the tile's first record
            out.append(_spine(d, touch, [9 + d // 2, 9 + d // 2 + 64]))   # cut among the covered reads (d = 2 T: the carry spans two blocks), then a tile of one wave
    return out


def by_name():
    return {s.name: s for s in scenes()}
