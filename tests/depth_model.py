"""A numpy model of tbk_cov_thresholds (tiebrush_amd/csrc/depththr.hip) in two independent forms, and the text of the two
tables `--depth-summary` and `--feature-depth` write.  numpy only; importable without a GPU.  Nothing here calls the code under test.

Rows and features are feature_model's: the dict Context.coverage returns, and a dict of arrays tid / beg / end (/ strand, name).

  per_row()   overlap arithmetic on the rows: per feature covered and, per threshold, the bases under a row with value >= T
  per_base()  the depth of every base of the feature on a dense array, compared base by base (features up to PER_BASE_MAX bases)
  per_ref()   the per-reference table: feature_model.per_row on the features [0, LN) for covered / sum / max, per_row() here for ge
"""
from fractions import Fraction

import numpy as np

import feature_model as fm

PER_BASE_MAX = fm.PER_BASE_MAX
MAX_THRESHOLDS = 16


def per_row(rows, feats, thr):
    """covered (uint64 [n]) and ge (uint64 [n, len(thr)])"""
    tid, st, en, val = (np.asarray(rows[k]) for k in ("iv_tid", "iv_start", "iv_end", "iv_val")) if "iv_tid" in rows else (np.zeros(0, np.int64),) * 4
    thr = np.asarray(thr, np.float64)
    n = len(feats["tid"])
    cov, ge = np.zeros(n, np.uint64), np.zeros((n, len(thr)), np.uint64)
    for f, (t, b, e) in enumerate(zip(feats["tid"], feats["beg"], feats["end"])):
        t, b, e = int(t), int(b), int(e)
        idx = np.flatnonzero((tid == t) & (st < e) & (en > b))
        ln = np.minimum(en[idx].astype(np.int64), e) - np.maximum(st[idx].astype(np.int64), b)     # (int64: exact)
        cov[f] = np.uint64(int(ln.sum()))
        for k in range(len(thr)):
            ge[f, k] = np.uint64(int(ln[val[idx] >= thr[k]].sum()))          # inclusive, on the doubles
    return cov, ge


def per_base(rows, feats, thr):
    """one (covered, [ge per threshold]) per feature; None for a feature beyond PER_BASE_MAX bases"""
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
                depth[a - b:z - b], has[a - b:z - b] = val[i], True
        out.append((int(has.sum()), [int((has & (depth >= float(T))).sum()) for T in thr]))
    return out


def per_ref(rows, lens, thr):
    """the per-reference table for exact sums: a list of dicts covered, sum (float), max, ge (list) in header order; LN:0 and references
    without rows give zeros"""
    live = [r for r, ln in enumerate(lens) if ln > 0]
    feats = dict(tid=np.array(live, np.int32), beg=np.zeros(len(live), np.int64), end=np.array([lens[r] for r in live], np.int64),
                 strand=np.full(len(live), ord("."), np.uint8))
    out = [dict(covered=0, sum=0.0, max=0.0, ge=[0] * len(thr)) for _ in lens]
    if live:
        m = fm.per_row(rows, feats)
        cov, ge = per_row(rows, feats, thr)
        for i, r in enumerate(live):
            s = float(m[i]["S"])
            assert Fraction(s) == m[i]["S"] and m[i]["covered"] == int(cov[i])
            out[r] = dict(covered=m[i]["covered"], sum=s, max=m[i]["max"], ge=[int(x) for x in ge[i]])
    return out


def depth_tsv(names, lens, thr_text, table):
    """the bytes of the --depth-summary file"""
    out = ["#chrom\tlength\tcovered\tsum\tmean0\tmean\tmax" + "".join("\tge_" + t for t in thr_text) + "\n"]

    def line(name, ln, r):
        mean0, mean = (r["sum"] / float(ln) if ln else 0.0), (r["sum"] / float(r["covered"]) if r["covered"] else 0.0)
        return "%s\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f" % (name, ln, r["covered"], r["sum"], mean0, mean, r["max"]) + "".join("\t%d" % g for g in r["ge"]) + "\n"
    tot = dict(covered=0, sum=0.0, max=0.0, ge=[0] * len(thr_text))
    for name, ln, r in zip(names, lens, table):
        out.append(line(name, ln, r))
        tot["covered"] += r["covered"]
        tot["sum"] += r["sum"]                               # header order, in double
        tot["max"] = max(tot["max"], r["max"])
        tot["ge"] = [a + b for a, b in zip(tot["ge"], r["ge"])]
    out.append(line("total", sum(lens), tot))
    return "".join(out).encode(), tot


def feature_tsv(names, feats, thr_text, cov, ge):
    """the bytes of the --feature-depth file"""
    out = ["#chrom\tstart\tend\tname\tstrand\tsize\tcovered" + "".join("\tge_" + t for t in thr_text) + "\n"]
    for k in range(len(feats["tid"])):
        b, e = int(feats["beg"][k]), int(feats["end"][k])
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d" % (names[int(feats["tid"][k])], b, e, feats["name"][k], chr(int(feats["strand"][k])), e - b, int(cov[k])) +
                   "".join("\t%d" % int(g) for g in ge[k]) + "\n")
    return "".join(out).encode()
