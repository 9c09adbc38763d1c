"""A numpy model of tbk_tx_summary (tiebrush_amd/csrc/txsum.hip) in two independent forms, and the text of the
transcripts file.  numpy only; importable without a GPU.  Nothing here calls the code under test.

Rows are the dict Context.coverage returns, a transcript table the dict tx_scenes.table builds: tx_off (CSR into the exons), tid,
strand (uint8), ex_beg, ex_end, and the lists id / gene.

  per_row()   feature_model.per_row over the exons, the junction rows of every intron looked up by their key, and the fold per
              transcript with exact rationals: covered, the exact sum S and the exact sum of |val x bases| (for the bound), the number m
              of row pieces, max, exons_hit; introns_hit, junc_min, the exact junc_sum JS with its |.| sum and row count; the parts
  per_base()  the depth of every exonic base on a dense array: covered, sum = math.fsum of the depths (the exact sum rounded once),
              max, exons_hit; the introns through a dictionary of the junction rows.  Exons beyond feature_model.PER_BASE_MAX bases
              leave the coverage half to per_row().
"""
import math
from fractions import Fraction

import numpy as np

import feature_model as fm


def exon_feats(tx):
    """the exons as features ('.'), in table order"""
    off = np.asarray(tx["tx_off"], np.int64)
    tid = np.repeat(np.asarray(tx["tid"], np.int32), np.diff(off))
    return dict(tid=tid, beg=np.asarray(tx["ex_beg"], np.int64), end=np.asarray(tx["ex_end"], np.int64), strand=np.full(len(tid), ord("."), np.uint8))


def intron_feats(tx):
    """the introns as features under their transcript's strand, in table order, and the exon each lies behind"""
    off = np.asarray(tx["tx_off"], np.int64)
    t, b, e, s, at = [], [], [], [], []
    for k in range(len(off) - 1):
        for x in range(off[k], off[k + 1] - 1):
            t.append(tx["tid"][k]), b.append(tx["ex_end"][x]), e.append(tx["ex_beg"][x + 1]), s.append(tx["strand"][k]), at.append(x)
    return dict(tid=np.array(t, np.int32), beg=np.array(b, np.int64), end=np.array(e, np.int64), strand=np.array(s, np.uint8)), np.array(at, np.int64)


def _junc_rows(rows, t, b, e, s):
    """the values of the junction rows that ARE the intron, in row order"""
    if "j_tid" not in rows:
        return []
    m = (rows["j_tid"] == t) & (rows["j_start"] == b) & (rows["j_end"] == e)
    if s != ord("."):
        m &= rows["j_strand"] == s
    return [float(v) for v in rows["j_val"][m]]


def per_row(rows, tx):
    """one dict per transcript: covered, S, abs (Fractions), m, max, exons_hit, exons, introns, introns_hit, junc_min, junc (the
    introns' values), JS, Jabs (Fractions), jm, dyadic, and `parts`: the exons' feature_model entries"""
    off = np.asarray(tx["tx_off"], np.int64)
    ex = fm.mark_dyadic(rows, fm.per_row(rows, exon_feats(tx)))
    out = []
    for k in range(len(off) - 1):
        parts = ex[off[k]:off[k + 1]]
        t, s = int(tx["tid"][k]), int(tx["strand"][k])
        junc, JS, JA, jm, jdy = [], Fraction(0), Fraction(0), 0, True
        for x in range(off[k], off[k + 1] - 1):
            vals = _junc_rows(rows, t, int(tx["ex_end"][x]), int(tx["ex_beg"][x + 1]), s)
            j = 0.0
            for v in vals:                                   # row order, as tbk_cov_summary adds them
                j += v
                JS, JA = JS + Fraction(v), JA + abs(Fraction(v))
                jdy = jdy and v * 8 == math.floor(v * 8)
            junc.append(j)
            jm += len(vals)
        hit = [p for p in parts if p["covered"] > 0]
        out.append(dict(covered=sum(p["covered"] for p in parts), S=sum((p["S"] for p in parts), Fraction(0)), abs=sum((p["abs"] for p in parts), Fraction(0)),
                        m=sum(p["m"] for p in parts), max=max((p["max"] for p in hit), default=0.0), exons_hit=len(hit), exons=len(parts),
                        dyadic=all(p["dyadic"] for p in parts), introns=len(junc), introns_hit=sum(j > 0 for j in junc), junc_min=min(junc, default=0.0),
                        junc=junc, JS=JS, Jabs=JA, jm=jm, jdyadic=jdy, parts=parts))
    return out


def per_base(rows, tx):
    """one dict per transcript: covered, sum, max, exons_hit (None where an exon is beyond PER_BASE_MAX bases), introns_hit, junc_min,
    junc_sum (math.fsum of the introns' rows)"""
    off = np.asarray(tx["tx_off"], np.int64)
    have_iv = "iv_tid" in rows
    tid, st, en, val = (np.asarray(rows[k]) for k in ("iv_tid", "iv_start", "iv_end", "iv_val")) if have_iv else (np.zeros(0, np.int64),) * 4
    table = {}
    if "j_tid" in rows:
        for t, b, e, s, v in zip(rows["j_tid"].tolist(), rows["j_start"].tolist(), rows["j_end"].tolist(), rows["j_strand"].tolist(), rows["j_val"].tolist()):
            table.setdefault((t, b, e), []).append((s, v))
    out = []
    for k in range(len(off) - 1):
        t, s = int(tx["tid"][k]), int(tx["strand"][k])
        spans = [(int(tx["ex_beg"][x]), int(tx["ex_end"][x])) for x in range(off[k], off[k + 1])]
        d = dict(covered=None, sum=None, max=None, exons_hit=None)
        if all(e - b <= fm.PER_BASE_MAX for b, e in spans):
            depths, hits = [], 0
            for b, e in spans:
                depth, has = np.zeros(e - b, np.float64), np.zeros(e - b, bool)
                for i in np.flatnonzero((tid == t) & (st < e) & (en > b)):
                    a, z = max(int(st[i]), b), min(int(en[i]), e)
                    assert not has[a - b:z - b].any(), "rows are disjoint"
                    depth[a - b:z - b], has[a - b:z - b] = val[i], True
                depths.append(depth[has])
                hits += bool(has.any())
            flat = np.concatenate(depths) if depths else np.zeros(0)
            d = dict(covered=len(flat), sum=math.fsum(flat), max=float(flat.max()) if len(flat) else 0.0, exons_hit=hits)
        js = []
        for (_, e0), (b1, _) in zip(spans[:-1], spans[1:]):
            js.append([v for ss, v in table.get((t, e0, b1), []) if s == ord(".") or ss == s])
        d.update(introns_hit=sum(math.fsum(j) > 0 for j in js), junc_min=min((math.fsum(j) for j in js), default=0.0), junc_sum=math.fsum(v for j in js for v in j))
        out.append(d)
    return out


def exact(m):
    """the dyadic rule for `sum` of one transcript (feature_model.exact, over all its exons)"""
    return m["abs"] < 2 ** 50 and (m["abs"] * 8).denominator == 1 and m["dyadic"]


def jexact(m):
    return m["Jabs"] < 2 ** 50 and m["jdyadic"]


def check(got, model, k):
    """the numeric contract of transcript k: the integers, max and junc_min exact; sum and junc_sum exact under the dyadic rule, else
    within gamma(pieces + 1) x the sum of the absolute terms"""
    m = model[k]
    if "covered" in got:
        assert int(got["covered"][k]) == m["covered"], (k, got["covered"][k], m["covered"])
        assert float(got["max"][k]) == m["max"], (k, got["max"][k], m["max"])
        assert int(got["exons_hit"][k]) == m["exons_hit"], (k, got["exons_hit"][k], m["exons_hit"])
        g = Fraction(float(got["sum"][k]))
        if exact(m):
            assert g == m["S"], (k, float(g), float(m["S"]))
        else:
            assert abs(g - m["S"]) <= fm.gamma(m["m"] + 1) * m["abs"], (k, float(g), float(m["S"]), m["m"])
    if "junc_sum" in got:
        assert int(got["introns_hit"][k]) == m["introns_hit"], (k, got["introns_hit"][k], m["introns_hit"])
        assert float(got["junc_min"][k]) == m["junc_min"], (k, got["junc_min"][k], m["junc_min"])
        g = Fraction(float(got["junc_sum"][k]))
        if jexact(m):
            assert g == m["JS"], (k, float(g), float(m["JS"]))
        else:
            assert abs(g - m["JS"]) <= fm.gamma(m["jm"] + 1) * m["Jabs"], (k, float(g), float(m["JS"]), m["jm"])


HEADER = "#chrom\tstart\tend\ttranscript\tgene\tstrand\texons\tlength\tcovered\tsum\tmean0\tmean\tmax\texons_hit\tintrons\tintrons_hit\tjunc_min\tjunc_sum\n"


def tsv(names, tx, model):
    """the bytes of the transcripts file for exact sums (the goldens: YC integral)"""
    off = np.asarray(tx["tx_off"], np.int64)
    out = [HEADER]
    for k, m in enumerate(model):
        b, e = int(tx["ex_beg"][off[k]]), int(tx["ex_end"][off[k + 1] - 1])
        length = int(sum(int(tx["ex_end"][x]) - int(tx["ex_beg"][x]) for x in range(off[k], off[k + 1])))
        s, js = float(m["S"]), float(m["JS"])
        assert Fraction(s) == m["S"] and Fraction(js) == m["JS"]
        mean0, mean = s / float(length), (s / float(m["covered"]) if m["covered"] else 0.0)
        out.append("%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f\t%d\t%d\t%d\t%.3f\t%.3f\n" % (
            names[int(tx["tid"][k])], b, e, tx["id"][k], tx["gene"][k], chr(int(tx["strand"][k])), m["exons"], length, m["covered"], s, mean0, mean, m["max"],
            m["exons_hit"], m["introns"], m["introns_hit"], m["junc_min"], js))
    return "".join(out).encode()
