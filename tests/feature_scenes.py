"""Hand-placed rows and features for tbk_cov_summary (tiebrush_amd/csrc/featsum.hip), written in terms of the kernel's
two constants: FS_TILE rows share an aggregate, a run of more than FS_DIRECT rows reads the aggregates of its whole tiles.  numpy only;
importable without a GPU.  A scene is (rows, feats, claims): `claims` are facts about the input — which path a feature takes, how many
whole tiles it reads, what its columns must be — that tests/test_feature_model_cpu.py proves through feature_model before the GPU is
asked (tests/test_gpu_features.py)."""
import numpy as np

from cov_scenes import TOP
from feature_model import FS_DIRECT, FS_TILE

T, D = FS_TILE, FS_DIRECT


def rows_of(iv=(), jn=()):
    """[(tid, start, end, val)] and [(tid, start, end, strand char, val)] -> the dict Context.coverage returns"""
    return dict(iv_tid=np.array([r[0] for r in iv], np.int32), iv_start=np.array([r[1] for r in iv], np.int32), iv_end=np.array([r[2] for r in iv], np.int32),
                iv_val=np.array([r[3] for r in iv], np.float64), j_tid=np.array([r[0] for r in jn], np.int32), j_start=np.array([r[1] for r in jn], np.int32),
                j_end=np.array([r[2] for r in jn], np.int32), j_strand=np.array([ord(r[3]) for r in jn], np.uint8), j_val=np.array([r[4] for r in jn], np.float64))


def feats(fl):
    """[(tid, beg, end[, strand char])] -> the dict of arrays the model and Context.cov_summary take"""
    return dict(tid=np.array([f[0] for f in fl], np.int32), beg=np.array([f[1] for f in fl], np.int64), end=np.array([f[2] for f in fl], np.int64),
                strand=np.array([ord(f[3]) if len(f) > 3 else ord(".") for f in fl], np.uint8))


# ---- features and rows at their edges -------------------------------------------------------------------------------------------------
def edges():
    """references 0 and 3 carry no row, 5 lies behind the last one; 1 and 2 share their rows' coordinates"""
    iv = [(1, 100, 200, 3.0), (1, 200, 250, 5.0), (1, 300, 301, 7.0), (2, 100, 200, 11.0), (2, 200, 250, 13.0), (4, 10, 20, 2.0)]
    F, C = [], []

    def add(f, **claim):
        F.append(f), C.append(claim)
    add((1, 120, 180), covered=60, sum=180.0, max=3.0)                        # inside one row
    add((1, 100, 200), covered=100, sum=300.0, max=3.0)                       # equal to a row
    for b in (99, 100, 101):                                                  # begin and end at a row's edges, shifted
        for e in (199, 200, 201):
            add((1, b, e), covered=min(e, 250) - max(b, 100), sum=3.0 * (min(e, 200) - max(b, 100)) + 5.0 * max(0, e - 200), max=5.0 if e > 200 else 3.0)
    add((1, 90, 100), covered=0, sum=0.0, max=0.0)                            # abuts a row in front
    add((1, 250, 260), covered=0, sum=0.0, max=0.0)                           # abuts a row behind
    add((1, 260, 290), covered=0, sum=0.0, max=0.0)                           # wholly in a gap
    add((1, 0, 50), covered=0, sum=0.0, max=0.0)                              # before the reference's first row
    add((0, 0, 1000), covered=0, sum=0.0, max=0.0)                            # before the first row of all, on a reference without rows
    add((1, 400, 500), covered=0, sum=0.0, max=0.0)                           # after the reference's last row
    add((4, 30, 40), covered=0, sum=0.0, max=0.0)                             # after the last row of all
    add((3, 100, 200), covered=0, sum=0.0, max=0.0)                           # a reference without rows between two with rows
    add((5, 100, 200), covered=0, sum=0.0, max=0.0)                           # the reference behind the last
    add((2, 100, 200), covered=100, sum=1100.0, max=11.0)                     # the neighbour's rows share the coordinates
    add((2, 150, 230), covered=80, sum=50 * 11.0 + 30 * 13.0, max=13.0)
    add((1, 150, 230), covered=80, sum=50 * 3.0 + 30 * 5.0, max=5.0)
    add((1, 240, 1000), covered=11, sum=57.0, max=7.0)                        # the run ends at the reference's last row
    add((2, 240, 1000), covered=10, sum=130.0, max=13.0)
    add((1, 300, 301), covered=1, sum=7.0, max=7.0)                           # a single-base row
    add((1, 299, 302), covered=1, sum=7.0, max=7.0)
    add((1, 150, 151), covered=1, sum=3.0, max=3.0)                           # features of size 1: on a row, in a gap, a row's last base
    add((1, 250, 251), covered=0, sum=0.0, max=0.0)
    add((1, 199, 200), covered=1, sum=3.0, max=3.0)
    add((4, 0, 2 ** 33), covered=10, sum=20.0, max=2.0)                       # an end far beyond what a row can name
    return rows_of(iv), feats(F), C


def top():
    """the largest value over the longest row (cov_scenes.TOP): the product needs 62 bits, so `sum` is held to the bound"""
    iv = [(0, 0, TOP - 1, float(TOP)), (1, TOP - 2, TOP - 1, float(TOP))]
    F = [(0, 0, TOP - 1), (0, 1, TOP - 2), (0, 5, 6), (0, 0, 2 ** 33), (1, 0, TOP - 1), (1, TOP - 2, TOP), (0, TOP - 1, TOP)]
    C = [dict(covered=TOP - 1, max=float(TOP)), dict(covered=TOP - 3, max=float(TOP)), dict(covered=1, sum=float(TOP), max=float(TOP)),
         dict(covered=TOP - 1, max=float(TOP)), dict(covered=1, sum=float(TOP)), dict(covered=1, sum=float(TOP)), dict(covered=0, sum=0.0, max=0.0)]
    return rows_of(iv), feats(F), C


# ---- run and tile thresholds ----------------------------------------------------------------------------------------------------------
HEAD = 37                      # rows of reference 0 in front: the runs' tiles are cut in the rows of ALL references
N_RUN = 4 * T + 100


def run_rows(scale=1.0):
    """HEAD rows on reference 0, N_RUN on reference 1, 20 on reference 2: row i of a reference is [10 i, 10 i + 7) with value
    (i mod 13 + 1) x scale"""
    iv = []
    for t, n in ((0, HEAD), (1, N_RUN), (2, 20)):
        iv += [(t, 10 * i, 10 * i + 7, (i % 13 + 1) * scale) for i in range(n)]
    return iv


def run_feature(ga, gb, trim=1):
    """the feature on reference 1 whose run is rows [ga, gb) of the whole row list; its first and last row are cut by `trim` bases"""
    a, b = ga - HEAD, gb - HEAD
    assert 0 <= a < b <= N_RUN
    return (1, 10 * a + trim, 10 * (b - 1) + 7 - trim)


def runs(scale=1.0):
    F, C = [], []

    def add(ga, gb, path, tiles, trim=1):
        F.append(run_feature(ga, gb, trim)), C.append(dict(lo=ga, hi=gb, path=path, tiles=tiles))
    for n in (1, 2, 63, 64, 65, D - 1, D):                  # lane-strided walks: less than, exactly and more than a wave of rows
        add(40, 40 + n, "direct", 0)
    add(40, 40 + D + 1, "agg", 0)                           # the first run on the aggregate path: two partial tiles, no whole one
    add(T, T + D, "direct", 0)                              # a whole tile, walked row by row
    for ga in (T - 1, T, T + 1):                            # a run that begins on a tile boundary and one row off it
        add(ga, 3 * T + 50, "agg", 1 if ga >= T else 2)
    for gb in (3 * T - 1, 3 * T, 3 * T + 1):                # a run that ends on one: its last row is never in a whole tile
        add(50, gb, "agg", 1 if gb <= 3 * T else 2)
    add(T, 2 * T + 1, "agg", 0)                             # begins on a boundary, the whole tile of its first row walked by rows
    add(T - 1, 2 * T + 1, "agg", 1)
    add(T - 1, 3 * T + 1, "agg", 2)
    add(250, 250 + 2 * T + 20, "agg", 2)
    add(HEAD, HEAD + N_RUN, "agg", 3)                       # one feature over every row of the reference, cut at both ends
    add(HEAD, HEAD + N_RUN, "agg", 3, trim=0)               # and not cut
    F.append((1, 0, 2 ** 31 - 1)), C.append(dict(lo=HEAD, hi=HEAD + N_RUN, path="agg", tiles=3))
    F.append((0, 0, 10 * HEAD)), C.append(dict(lo=0, hi=HEAD, path="direct", tiles=0))
    F.append((2, 0, 500)), C.append(dict(lo=HEAD + N_RUN, hi=HEAD + N_RUN + 20, path="direct", tiles=0))   # the run ends at the last row of all
    return rows_of(run_rows(scale)), feats(F), C


def thirds():
    """the runs with values k / 3: no product is representable, `sum` is held to the bound; covered and max stay exact"""
    return runs(1.0 / 3.0)


# ---- feature lists --------------------------------------------------------------------------------------------------------------------
LIST_N = (1, 64, 65, 257)


def feature_list(n):
    """n features on the rows of runs(): duplicates, nested ones and a reversed order, both paths among them (n >= 64)"""
    F = []
    for k in range(n):
        a = HEAD + (k * 29) % (N_RUN - 2 * T - 10)
        ln = (1, 5, 70, D + 1 + k % 7, 2 * T + 3)[k % 5]
        F.append(run_feature(a, a + ln, trim=k % 3))
        if k % 4 == 1:
            F.append(F[-1])                                  # a duplicate
        if k % 4 == 2:
            f = F[-1]
            F.append((f[0], f[1] + 3, max(f[1] + 4, f[2] - 3)))   # nested in the one before
    F = F[:n][::-1]                                          # descending starts
    return rows_of(run_rows()), feats(F), [dict() for _ in F]


# ---- junction lookup ------------------------------------------------------------------------------------------------------------------
def junctions():
    jn = [(0, 100, 200, "+", 2.0), (0, 100, 200, "-", 3.0), (0, 100, 200, ".", 5.0), (0, 100, 300, "+", 7.0), (0, 150, 200, "-", 11.0),
          (1, 100, 200, "+", 13.0), (1, 500, 900, ".", 17.0)]
    F, C = [], []

    def add(f, junc):
        F.append(f), C.append(dict(junc=junc, covered=0, sum=0.0, max=0.0))
    for s, v in (("+", 2.0), ("-", 3.0), (".", 10.0)):       # the first row; one triple on three strands, asked with each and with '.'
        add((0, 100, 200, s), v)
    for s, v in (("+", 7.0), ("-", 0.0), (".", 7.0)):        # the same start with another end
        add((0, 100, 300, s), v)
    for f in ((0, 99, 200), (0, 101, 200), (0, 100, 199), (0, 100, 201), (0, 150, 201), (0, 149, 200)):   # a base off at either end
        add(f, 0.0)
    add((0, 150, 200, "-"), 11.0), add((0, 150, 200, "+"), 0.0), add((0, 150, 200), 11.0)
    add((1, 100, 200, "+"), 13.0), add((1, 100, 200, "-"), 0.0), add((1, 100, 200), 13.0)   # the same coordinates on the neighbour
    add((1, 100, 300), 0.0)
    add((1, 500, 900), 17.0), add((1, 500, 900, "+"), 0.0)   # the last row
    add((2, 100, 200), 0.0), add((0, 0, 50), 0.0)
    return rows_of([], jn), feats(F), C


def search_edges():
    """the searches are 64-ary: 128 rows (and junction rows) are two probes a lane short of none, and an answer behind the last row is
    found when every probe of a round fails"""
    iv = [(0, 10 * i, 10 * i + 7, float(i % 5 + 1)) for i in range(128)]
    jn = [(0, 10 * i + 7, 10 * i + 10, "+", float(i + 1)) for i in range(128)]
    F, C = [], []

    def add(f, **claim):
        F.append(f), C.append(claim)
    add((1, 0, 100), covered=0, junc=0.0, lo=128, hi=128)                      # behind the last row: every probe fails
    add((0, 1277, 1280, "-"), covered=0, junc=0.0, lo=128, hi=128)
    add((0, 1277, 1280, "+"), junc=128.0), add((0, 1277, 1280), junc=128.0)    # the last junction row
    add((0, 1270, 1280), covered=7, sum=21.0, lo=127, hi=128)                  # the last row
    add((0, 0, 7), covered=7, sum=7.0, lo=0, hi=1)                             # the first
    add((0, 7, 10, "-"), junc=0.0), add((0, 7, 10), junc=1.0)                  # the first junction row
    for i in (62, 63, 64, 65, 126):                                            # around the probes of the first round
        add((0, 10 * i, 10 * i + 10), covered=7, sum=7.0 * (i % 5 + 1), junc=0.0, lo=i, hi=i + 1)
        add((0, 10 * i + 7, 10 * i + 10), covered=0, junc=float(i + 1), lo=i + 1, hi=i + 1)
    add((0, 0, 1280), covered=7 * 128, lo=0, hi=128, path="direct")
    return rows_of(iv, jn), feats(F), C


SCENES = {"edges": edges, "top": top, "runs": runs, "thirds": thirds, "junctions": junctions, "search_edges": search_edges}
SCENES.update({"list%d" % n: (lambda n=n: feature_list(n)) for n in LIST_N})


# ---- a seeded random case ------------------------------------------------------------------------------------------------------------
def random_case(seed=20240607, n_rows=4000, n_feat=2000):
    """rows with values that are multiples of 1/8 on four references (one without rows), features of every length scale: more than half
    meet a row, more than a tenth read aggregates"""
    rng = np.random.RandomState(seed)
    iv, jn = [], []
    per = n_rows // 3
    for t in (0, 1, 3):
        gaps, lens = rng.randint(0, 6, per), rng.randint(1, 40, per)
        st = np.cumsum(gaps + np.concatenate([[0], lens[:-1]])) + 1000
        iv += [(t, int(s), int(s + l), float(v) / 8.0) for s, l, v in zip(st, lens, rng.randint(1, 4000, per))]
    seen = set()
    for _ in range(300):
        r = iv[rng.randint(len(iv))]
        key = (r[0], r[2], r[2] + int(rng.randint(50, 500)))
        for s in "+-."[:rng.randint(1, 4)]:
            seen.add(key + (s,))
    jn = [k + (float(rng.randint(1, 100)),) for k in sorted(seen, key=lambda k: (k[0], k[1], k[2], ord(k[3])))]
    F = []
    for k in range(n_feat):
        kind = k % 10
        if kind == 0:                                         # a junction's own coordinates
            j = jn[rng.randint(len(jn))]
            F.append((j[0], j[1], j[2], "+-."[rng.randint(3)]))
            continue
        r = iv[rng.randint(len(iv))]
        span = int((5, 40, 300, 3000, 3000, 9000, 9000, 20000, 40000)[kind - 1] * (0.5 + rng.rand()))
        b = max(0, r[1] + int(rng.randint(-20, 20)))
        F.append((r[0] if kind != 9 else (r[0] + 2) % 5, b, b + span, "+-."[rng.randint(3)]))
    return rows_of(iv, jn), feats(F)


# ---- the golden tracks ----------------------------------------------------------------------------------------------------------------
def read_tracks(cov_path, junc_path, names):
    """our own plain tracks (or the goldens) back as rows"""
    tid = {n: i for i, n in enumerate(names)}
    iv, jn = [], []
    for ln in open(cov_path).read().split("\n")[1:]:
        if ln:
            f = ln.split("\t")
            iv.append((tid[f[0]], int(f[1]), int(f[2]), float(f[3])))
    for ln in open(junc_path).read().split("\n")[1:]:
        if ln:
            f = ln.split("\t")
            jn.append((tid[f[0]], int(f[1]), int(f[2]), f[5], float(f[4])))
    return rows_of(iv, jn)


def golden_bed(rows, names, lens, seed=5):
    """BED lines for a golden's rows, as a user's annotation would mix them: "exons" (runs of rows that abut, whole and cut), every
    junction row as an intron with its own strand, with '.' and with the other strand, windows in gaps and across runs, a whole
    reference, an end beyond the reference (cut), unsorted, with duplicates, 3 to 6 columns, comment and track lines between"""
    rng = np.random.RandomState(seed)
    t, s, e = rows["iv_tid"], rows["iv_start"], rows["iv_end"]
    brk = np.flatnonzero((t[1:] != t[:-1]) | (s[1:] != e[:-1])) + 1
    a, z = np.concatenate([[0], brk]), np.concatenate([brk, [len(t)]])
    out = ["# features of the golden rows", "track name=annotation"]
    k = 0
    for i in rng.permutation(len(a))[:400]:
        tt, b, x = int(t[a[i]]), int(s[a[i]]), int(e[z[i] - 1])
        forms = [(b, x), (b + 1, x), (b, x + 7), (max(0, b - 5), b), (b + (x - b) // 2, x + 200), (max(0, b - 3000), x + 3000)]
        b, x = forms[k % len(forms)]
        f = [names[tt], str(b), str(max(b + 1, min(x, lens[tt])))] + ["exon%d" % k, "0", "+-."[k % 3]][:(0, 1, 3, 2)[k % 4]]
        out.append("\t".join(f))
        k += 1
    for i in range(len(rows["j_tid"])):
        tt, b, x, st = int(rows["j_tid"][i]), int(rows["j_start"][i]), int(rows["j_end"][i]), chr(int(rows["j_strand"][i]))
        other = "-" if st == "+" else "+"
        for s6 in (st, ".", other)[:1 + i % 3]:
            out.append("\t".join([names[tt], str(b), str(x), "intron%d" % i, "0", s6]))
        if i % 5 == 0:
            out.append(" ".join([names[tt], str(b + 1), str(x), "shifted%d" % i, "0", st]))
    tt = int(t[0])
    out += ["", "browser position x", "\t".join([names[tt], "0", str(lens[tt] + 1000), "whole"]), out[2], "\t".join([names[tt], "0", str(lens[tt])]) + "\r"]
    return out
