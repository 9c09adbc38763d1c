"""Support for the tests of `tiecov -R` / `tiebrush -R`: a BED writer, the normalisation of a region table restated in
plain Python, the contract on rows and track lines for a table U built on region_fixtures' one-region clips, and the brute-force
"overlaps any interval" filter.  Nothing here calls the code under test."""
import random

import numpy as np

import region_fixtures as rf


def write_bed(path, names, intervals, sep="\t", extra=None, eol="\n", head=()):
    """intervals [(tid, beg, end)] as BED lines `chrom start end[ extra...]`, after the lines of `head`, in the order given"""
    lines = list(head)
    for k, (t, b, e) in enumerate(intervals):
        f = [names[t], str(b), str(e)] + ([extra[k % len(extra)]] if extra else [])
        lines.append(sep.join(x for x in f if x != ""))
    with open(path, "w", newline="") as fh:
        fh.write("".join(ln + eol for ln in lines))
    return path


def normalise(intervals, lens):
    """the table U of a list of (tid, beg, end): ends cut to the reference, empty intervals dropped, sorted by (tid, beg), intervals that
    overlap or abut merged"""
    iv = sorted((t, b, min(e, lens[t])) for t, b, e in intervals if b < min(e, lens[t]))
    out = []
    for t, b, e in iv:
        if out and out[-1][0] == t and b <= out[-1][2]:
            out[-1] = (t, out[-1][1], max(out[-1][2], e))
        else:
            out.append((t, b, e))
    return out


def is_normalised(table):
    return len(table) >= 1 and all(t >= 0 and 0 <= b < e for t, b, e in table) and \
        all(p[0] < q[0] or (p[0] == q[0] and p[2] < q[1]) for p, q in zip(table, table[1:]))


def overlaps_any(tid, beg, end, table):
    """numpy arrays of records (or rows) -> the mask of those that overlap any interval of the table, by brute force"""
    m = np.zeros(len(tid), dtype=bool)
    for t, b, e in table:
        m |= (tid == t) & (beg < e) & (end > b)
    return m


def brute(recs, table):
    """the records (tid, beg, end, vbeg) of a fixture that overlap any interval, in file order, each once"""
    return [r for r in recs if any(r[0] == t and r[1] < e and r[2] > b for t, b, e in table)]


def _cat(parts, keys, like):
    return {k: (np.concatenate([p[k] for p in parts]) if parts else like[k][:0]) for k in keys}


def clip_cov_union(w, table):
    """whole-file rows -> the rows `-R` must give: the interval rows cut to every interval of U in turn (U is sorted: (tid, start) order; a
    row across a gap comes out once per interval), the junction rows that overlap any interval once, whole, in the file's order"""
    iv = ("iv_tid", "iv_start", "iv_end", "iv_val")
    out = _cat([{k: rf.clip_cov(w, t, b, e)[k] for k in iv} for t, b, e in table], iv, w)
    j = overlaps_any(w["j_tid"], w["j_start"], w["j_end"], table)
    out.update({k: w[k][j] for k in ("j_tid", "j_start", "j_end", "j_strand", "j_val")})
    return out


def clip_sample_union(w, table):
    keys = ("s_tid", "s_start", "s_end", "s_count", "s_heat")
    return _cat([rf.clip_sample(w, t, b, e) for t, b, e in table], keys, w)


def clip_track_lines_union(lines, names, table, junc=False):
    """the lines of a whole-file track file (header line first) -> the file `-R` must write, byte for byte"""
    out = [lines[0]]
    if not junc:
        for t, b, e in table:
            out += rf.clip_track_lines(lines, names[t], b, e)[1:]
        return out
    k = 0
    for ln in lines[1:]:
        f = ln.split("\t")
        a, z = int(f[1]), int(f[2])
        if any(f[0] == names[t] and a < e and z > b for t, b, e in table):
            k += 1
            f[3] = "JUNC%08d" % k
            out.append("\t".join(f))
    return out


def random_table(fx, seed, lo=2, hi=40):
    """a normalised table of lo..hi intervals drawn around the fixture's records, as the BED reader would make it of them: starts as
    region_fixtures.random_regions draws them, lengths short enough that most intervals stay apart (those that do not are merged, so a
    table can come out shorter; never empty)"""
    rng = random.Random(seed)
    iv, n = [], rng.randint(lo, hi)
    while len(iv) < n or not normalise(iv, fx.lens):
        r = fx.recs[rng.randrange(len(fx.recs))]
        b = max(0, r[1] + rng.randrange(-40000, 40000))
        iv.append((r[0], b, b + rng.choice([1, 1, 50, 50, 1000, 20000])))
    return normalise(iv, fx.lens)
