"""Hand-built coverage rows for the bigWig builders (host/bigwig.cpp, bigwig.hip).  Every scene sits on one edge of the section packer
or of the zoom levels and says which; `check` states that claim about the model's output (tests/bigwig_model.py), so a scene that
drifts off its edge fails on the CPU before it means nothing on the GPU.

A scene: name, edge (one sentence), chroms [(name, length)], rows (tid int32, start int32, end int32, val float32), check(model).
Values travel to `tbh_tool bedgraph2bw` as 9 significant digits, which read back as the same float32."""
import functools

import numpy as np


class Scene:
    def __init__(self, name, edge, chroms, tid, start, end, val, check):
        self.name, self.edge, self.chroms, self.check = name, edge, chroms, check
        self.tid = np.asarray(tid, dtype=np.int32)
        self.start = np.asarray(start, dtype=np.int32)
        self.end = np.asarray(end, dtype=np.int32)
        self.val = np.asarray(val, dtype=np.float32)
        assert len(self.tid) == len(self.start) == len(self.end) == len(self.val)

    @property
    def n(self):
        return len(self.tid)

    def sam_header(self):
        return "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in self.chroms)

    def bedgraph(self):
        names = [c[0] for c in self.chroms]
        return "".join("%s\t%d\t%d\t%.9g\n" % (names[t], s, e, v) for t, s, e, v in zip(self.tid, self.start, self.end, self.val))

    def ref_len(self):
        return np.array([c[1] for c in self.chroms], dtype=np.uint32)


def _vals(n, seed=3):
    # fractional values: their float32 products and sums round at every step, so the order of a sum shows
    return (np.random.RandomState(seed).rand(n) * 9.0 + 0.125).astype(np.float32)


def _run(n, first=0, step=2, width=1):
    s = first + step * np.arange(n, dtype=np.int64)
    return s, s + width


def _data(m):
    return m["levels"][0]["sections"]


def _counts(m, level=0):
    per = 12 if level == 0 else 32
    head = 24 if level == 0 else 0
    return [(len(p) - head) // per for (_c, _s, _e, p) in m["levels"][level]["sections"]]


def _one_chrom(n):
    s, e = _run(n)
    return [("chr1", 10000)], np.zeros(n), s, e, _vals(n)


def _s1023():
    c, t, s, e, v = _one_chrom(1023)
    return Scene("items_1023", "one item short of a full section", c, t, s, e, v, lambda m: _counts(m) == [1023])


def _s1024():
    c, t, s, e, v = _one_chrom(1024)
    return Scene("items_1024", "exactly one full section, and no empty one behind it", c, t, s, e, v, lambda m: _counts(m) == [1024])


def _s1025():
    c, t, s, e, v = _one_chrom(1025)
    return Scene("items_1025", "a full section and a section of one item", c, t, s, e, v, lambda m: _counts(m) == [1024, 1])


def _change_at_1024():
    s0, e0 = _run(1024)
    s1, e1 = _run(10, first=7)
    return Scene("chrom_change_at_1024", "the chromosome changes where the section is full anyway: two sections, not three",
                 [("chr1", 10000), ("chr2", 500)], [0] * 1024 + [1] * 10, np.r_[s0, s1], np.r_[e0, e1], _vals(1034),
                 lambda m: _counts(m) == [1024, 10] and [x[0] for x in _data(m)] == [0, 1])


def _change_mid():
    s0, e0 = _run(300)
    s1, e1 = _run(1100, first=1)
    return Scene("chrom_change_mid_section", "a chromosome change cuts a section short; the next chromosome's count starts again",
                 [("chr1", 10000), ("chr2", 10000)], [0] * 300 + [1] * 1100, np.r_[s0, s1], np.r_[e0, e1], _vals(1400),
                 lambda m: _counts(m) == [300, 1024, 76])


def _many_chroms():
    n = 700
    return Scene("chroms_700", "700 chromosomes of one item: more than 256 sections a level, so the R-trees have two levels; most "
                 "chromosomes of a level have exactly one section", [("c%03d" % i, 1000 + i) for i in range(n)], np.arange(n),
                 10 + np.arange(n) % 7, 20 + np.arange(n) % 7, _vals(n),
                 lambda m: len(_data(m)) == 700 and len(m["levels"]) == 2 and len(m["levels"][1]["sections"]) == 700)


def _wide_item():
    # 399 one-base items pull the mean width down to 10, so the reduction is 44 and the 4000-base item crosses about 91 bins
    s, e = _run(399, first=4010, step=3)
    return Scene("item_across_90_bins", "one item opens about 90 zoom records; the item behind it starts in its last bin",
                 [("chr1", 20000)], np.zeros(400), np.r_[5, s], np.r_[4005, e], _vals(400),
                 lambda m: m["levels"][1]["reduction"] == 44 and m["opens"][0][0] == 4004 // 44 - 5 // 44 + 1 and m["opens"][0][1] == 0)


def _bin_edges():
    # reduction 32 (60 one-base items keep the mean width at 2)
    s, e = _run(60, first=400, step=5)
    return Scene("items_on_bin_edges", "items that start and end exactly on bin edges: [32,64) is one bin, [95,96) ends on an edge, "
                 "[96,129) starts on one and ends one base behind the next", [("chr1", 5000)], np.zeros(64), np.r_[32, 64, 95, 96, s],
                 np.r_[64, 65, 96, 129, e], _vals(64),
                 lambda m: m["levels"][1]["reduction"] == 32 and list(m["opens"][0][:4]) == [1, 1, 0, 2])


def _shared_bin():
    s, e = _run(200, first=3, step=7, width=2)
    return Scene("neighbours_share_a_bin", "several items in one bin: only the first opens the record, the others add to it in row order",
                 [("chr1", 5000)], np.zeros(200), s, e, _vals(200),
                 lambda m: m["levels"][1]["reduction"] == 32 and m["opens"][0][0] == 1 and list(m["opens"][0][1:4]) == [0, 0, 0])


def _two_chroms_same_bin():
    return Scene("two_chroms_same_bin_number", "the last item of one chromosome and the first of the next fall into bin 1 of their own "
                 "chromosomes: the bin number alone must not merge them", [("chr1", 500), ("chr2", 500)], [0, 0, 1, 1], [3, 40, 33, 70],
                 [9, 45, 36, 75], _vals(4),
                 lambda m: [(r[0], r[1]) for r in m["records"][0]] == [(0, 0), (0, 32), (1, 32), (1, 64)])


def _short_chrom():
    return Scene("end_clamp", "the last bin of chromosomes shorter than the bin: the record ends at the chromosome's length, or at the "
                 "item's end where that lies behind it", [("chr1", 20), ("chr2", 10), ("chr3", 100)], [0, 1, 2, 2, 2, 2], [3, 4, 5, 70, 80, 90],
                 [18, 12, 6, 71, 81, 91], _vals(6),
                 lambda m: m["levels"][1]["reduction"] == 32 and
                 [(r[0], r[1], r[2]) for r in m["records"][0]] == [(0, 0, 20), (1, 0, 12), (2, 0, 32), (2, 64, 96)])


def _dense():
    n = 40000
    s, e = _run(n, first=1, step=4, width=2)
    return Scene("dense_40k", "40,000 narrow spaced items with fractional values: three zoom levels, the coarsest bins hold 128 items "
                 "each, where the order of a float sum shows", [("chr1", 200000)], np.zeros(n), s, e, _vals(n),
                 lambda m: [lv["reduction"] for lv in m["levels"][1:]] == [32, 128, 512] and max(m["per_bin"][2]) >= 128)


def _sparse():
    n = 1100
    s, e = _run(n, first=0, step=100000, width=10)
    return Scene("sparse_discard", "every item alone in its bin at levels 0 and 1: level 1 does not shrink, is discarded and ends the plan",
                 [("chr1", 120000000)], np.zeros(n), s, e, _vals(n),
                 lambda m: len(m["levels"]) == 2 and m["levels"][1]["n_items"] >= 1000 and m["dropped"] == 1)


def _huge():
    return Scene("item_wider_than_2_29", "one item wider than 2^29: the first reduction is already 2^31 or more, no zoom level",
                 [("chr1", 1 << 30)], [0], [5], [(1 << 29) + 13], [2.5], lambda m: len(m["levels"]) == 1)


def _empty():
    return Scene("no_rows", "zero rows: one empty data level and nothing else", [("chr1", 1000)], [], [], [], [],
                 lambda m: len(m["levels"]) == 1 and m["levels"][0]["sections"] == [])


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(f() for f in (_s1023, _s1024, _s1025, _change_at_1024, _change_mid, _many_chroms, _wide_item, _bin_edges, _shared_bin,
                               _two_chroms_same_bin, _short_chrom, _dense, _sparse, _huge, _empty))


def names():
    return [s.name for s in scenes()]


def by_name(name):
    return next(s for s in scenes() if s.name == name)
