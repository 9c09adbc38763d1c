"""A numpy model of tbk_cov_summary (tiebrush_amd/csrc/featsum.hip) in two independent forms, and the text of the summary
file.  numpy only; importable without a GPU.  Nothing here calls the code under test.

Rows are the dict Context.coverage returns (iv_tid / iv_start / iv_end / iv_val, j_tid / j_start / j_end / j_strand / j_val as numpy
arrays), features a dict of arrays tid / beg / end / strand (uint8) as feature_scenes.feats builds it.

  per_row()   overlap arithmetic on the rows with exact rationals: covered, the exact sum S and the exact sum of |val x bases| (for the
              bound), the number m of rows on the feature, max, junc; and where the kernel's feature pass goes: the run [lo, hi) of rows,
              "direct" or "agg", and the number of whole tiles whose aggregates it reads
  per_base()  the depth of every base of the feature on a dense array, sliced: covered = the bases with a row, sum = math.fsum of
              their depths (the correctly rounded exact sum), max.  Features longer than PER_BASE_MAX bases are left to per_row().
"""
import math
from fractions import Fraction

import numpy as np

FS_TILE = 256      # featsum.hip: interval rows per aggregate
FS_DIRECT = 256    # featsum.hip: the longest run that is walked row by row
PER_BASE_MAX = 1 << 22
U = 2.0 ** -53


def gamma(k):
    """the standard bound of k roundings, as an exact rational"""
    ku = Fraction(k) * Fraction(U)
    return ku / (1 - ku)


def _junc(rows, t, b, e, s):
    if "j_tid" not in rows:
        return 0.0
    m = (rows["j_tid"] == t) & (rows["j_start"] == b) & (rows["j_end"] == e)
    if s != ord("."):
        m &= rows["j_strand"] == s
    j = 0.0
    for v in rows["j_val"][m]:          # row order
        j += float(v)
    return j


def per_row(rows, feats):
    """one dict per feature: covered, S, abs (Fractions), m, max, junc, lo, hi, path, tiles"""
    tid, st, en, val = (np.asarray(rows[k]) for k in ("iv_tid", "iv_start", "iv_end", "iv_val")) if "iv_tid" in rows else (np.zeros(0, np.int64),) * 4
    out = []
    for t, b, e, s in zip(feats["tid"], feats["beg"], feats["end"], feats["strand"]):
        t, b, e, s = int(t), int(b), int(e), int(s)
        idx = np.flatnonzero((tid == t) & (st < e) & (en > b))
        S, A, cov, mx = Fraction(0), Fraction(0), 0, 0.0
        for i in idx:
            ln = min(int(en[i]), e) - max(int(st[i]), b)
            p = Fraction(float(val[i])) * ln
            S, A, cov = S + p, A + abs(p), cov + ln
        if len(idx):
            mx = float(val[idx].max())
            assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1)), "the rows of a feature are one run"
        # the run as the kernel's two searches find it (an empty one lies where the rows behind the feature's begin start)
        lo = int(idx[0]) if len(idx) else int(np.count_nonzero((tid < t) | ((tid == t) & (en <= b))))
        hi = lo + len(idx)
        path, tiles = "direct", 0
        if hi - lo > FS_DIRECT:
            path, tiles = "agg", max(0, (hi - 1) // FS_TILE - (lo // FS_TILE + 1))
        out.append(dict(covered=cov, S=S, abs=A, m=len(idx), max=mx, junc=_junc(rows, t, b, e, s), lo=lo, hi=hi, path=path, tiles=tiles))
    return out


def per_base(rows, feats):
    """one dict per feature: covered, sum (float: the exact sum rounded once), max; None for a feature beyond PER_BASE_MAX bases"""
    tid, st, en, val = (np.asarray(rows[k]) for k in ("iv_tid", "iv_start", "iv_end", "iv_val"))
    out = []
    for t, b, e in zip(feats["tid"], feats["beg"], feats["end"]):
        t, b, e = int(t), int(b), int(e)
        if e - b > PER_BASE_MAX:
            out.append(None)
            continue
        depth, has = np.zeros(e - b, np.float64), np.zeros(e - b, bool)
        for i in np.flatnonzero(tid == t):
            a, z = max(int(st[i]), b), min(int(en[i]), e)
            if a < z:
                assert not has[a - b:z - b].any(), "rows are disjoint"
                depth[a - b:z - b], has[a - b:z - b] = val[i], True
        out.append(dict(covered=int(has.sum()), sum=math.fsum(depth[has]), max=float(depth[has].max()) if has.any() else 0.0))
    return out


def exact(m):
    """the dyadic rule of the contract for one per_row() entry: every product and partial sum of the feature is representable when
    the row values are multiples of 2^-3 and the sum of |val x bases| stays below 2^50 — then every order of additions gives S"""
    return m["abs"] < 2 ** 50 and (m["abs"] * 8).denominator == 1 and m.get("dyadic", True)


def mark_dyadic(rows, model):
    """adds m["dyadic"]: every row value on the feature is a multiple of 2^-3"""
    v = np.asarray(rows["iv_val"], np.float64) if "iv_tid" in rows else np.zeros(0)
    ok = (v * 8 == np.floor(v * 8))
    for m in model:
        m["dyadic"] = bool(ok[m["lo"]:m["hi"]].all())
    return model


def check_sum(got, m):
    """the numeric contract of `sum` for one feature: exact under the dyadic rule, else within gamma(m + 1) x the sum of |val x bases|"""
    if exact(m):
        assert Fraction(float(got)) == m["S"], (got, float(m["S"]))
    else:
        assert abs(Fraction(float(got)) - m["S"]) <= gamma(m["m"] + 1) * m["abs"], (got, float(m["S"]), m["m"])


def tsv(names, feats, model, want_name=True):
    """the bytes of the summary file for exact sums (the goldens: YC integral)"""
    out = ["#chrom\tstart\tend\tname\tstrand\tsize\tcovered\tsum\tmean0\tmean\tmax\tjunc\n"]
    for k, m in enumerate(model):
        b, e = int(feats["beg"][k]), int(feats["end"][k])
        s = float(m["S"])
        assert Fraction(s) == m["S"]
        mean0, mean = s / float(e - b), (s / float(m["covered"]) if m["covered"] else 0.0)
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\n" % (names[int(feats["tid"][k])], b, e, feats["name"][k] if want_name else ".",
                                                                                   chr(int(feats["strand"][k])), e - b, m["covered"], s, mean0, mean, m["max"], m["junc"]))
    return "".join(out).encode()
