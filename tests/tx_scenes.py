"""Hand-placed rows and transcript tables for tbk_tx_summary (tiebrush_amd/csrc/txsum.hip).  numpy only; importable without
a GPU.  A scene is (rows, tx, claims): `claims` holds one dict per transcript with facts about the input — what its columns must be,
which path an exon takes — that tests/test_tx_model_cpu.py proves through tx_model before the GPU is asked (tests/test_gpu_transcripts.py).
A claim `parts` is a list of per-exon dicts (feature_model keys), `junc` the list of the introns' values."""
import numpy as np

import feature_scenes as fs
from cov_scenes import TOP
from feature_model import FS_DIRECT, FS_TILE

T, D = FS_TILE, FS_DIRECT
WAVE = 64


def table(txs):
    """[(tid, strand char, [(beg, end), ...][, id[, gene]])] -> the transcript table as the model and Context.tx_summary take it"""
    off, eb, ee = [0], [], []
    for x in txs:
        eb += [e[0] for e in x[2]]
        ee += [e[1] for e in x[2]]
        off.append(len(eb))
    return dict(tx_off=np.array(off, np.uint32), tid=np.array([x[0] for x in txs], np.int32), strand=np.array([ord(x[1]) for x in txs], np.uint8),
                ex_beg=np.array(eb, np.int64), ex_end=np.array(ee, np.int64), id=[x[3] if len(x) > 3 else "tx%d" % k for k, x in enumerate(txs)],
                gene=[x[4] if len(x) > 4 else "." for x in txs])


# ---- exon counts at the fold's lane edges ----------------------------------------------------------------------------------------------
SIZES = (1, 2, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1)
N_SIZE_ROWS = 2 * (2 * WAVE + 1) + 40


def exon_on_row(i, trim=1):
    """row i of a reference of sizes() / feature_scenes.run_rows() is [10 i, 10 i + 7): the exon inside it, cut by `trim` at both ends"""
    return (10 * i + trim, 10 * i + 7 - trim)


def sizes(scale=1.0):
    """one transcript per exon count of SIZES on reference 0 (row i is [10 i, 10 i + 7) with value (i mod 13 + 1) x scale): exon j of a
    transcript that starts at row a lies inside row a + 2 j, so every exon is hit; every intron has its junction row on '+', with the
    value (j mod 7 + 2) x scale, the smallest in the middle of the transcript where it has three introns or more"""
    iv = [(0, 10 * i, 10 * i + 7, (i % 13 + 1) * scale) for i in range(N_SIZE_ROWS)]
    txs, jn, C = [], {}, []
    for k, n in enumerate(SIZES):
        a = 3 + k
        ex = [exon_on_row(a + 2 * j, trim=k % 3) for j in range(n)]      # (the trims keep the introns of two transcripts apart)
        vals = [(j % 7 + 2) * scale for j in range(n - 1)]
        if n >= 4:
            vals[(n - 1) // 2] = 1 * scale
        for j in range(n - 1):
            key = (0, ex[j][1], ex[j + 1][0], "+")
            assert key not in jn
            jn[key] = vals[j]
        txs.append((0, "+", ex))
        C.append(dict(exons=n, exons_hit=n, covered=(7 - 2 * (k % 3)) * n, introns=n - 1, introns_hit=n - 1, junc_min=min(vals, default=0.0), junc=vals,
                      max=max(((a + 2 * j) % 13 + 1) * scale for j in range(n))))
    rows = fs.rows_of(iv, [k + (v,) for k, v in sorted(jn.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], ord(kv[0][3])))])
    return rows, table(txs), C


def thirds():
    """sizes() with values k / 3: no product is representable, `sum` and `junc_sum` are held to the bound; the rest stays exact"""
    return sizes(1.0 / 3.0)


# ---- lists of transcripts: the CSR offsets matter --------------------------------------------------------------------------------------
LIST_N = (1, 64, 65, 257)
LIST_SIZES = (1, 2, 5, 1, 3, 9, 1, WAVE + 1)


def tx_list(n):
    """n transcripts of mixed sizes on reference 1 of feature_scenes.run_rows(), with duplicates, in descending order of their starts"""
    txs = []
    for k in range(n):
        size = LIST_SIZES[k % len(LIST_SIZES)]
        a = (k * 29) % (fs.N_RUN - 2 * (WAVE + 1) - 10)
        txs.append((1, "+-."[k % 3], [exon_on_row(a + 2 * j, trim=k % 3) for j in range(size)]))
        if k % 4 == 1:
            txs.append(txs[-1])                                  # a duplicate
    txs = sorted(txs[:n], key=lambda x: -x[2][0][0])
    jn = [(1, 10 * i + 7 - t, 10 * (i + 2) + t, s, float(i % 5 + 1)) for i in range(0, fs.N_RUN - 2, 3) for t, s in ((0, "+"), (1, "-"), (2, "."))]
    jn.sort(key=lambda r: (r[0], r[1], r[2], ord(r[3])))
    return fs.rows_of(fs.run_rows(), jn), table(txs), [dict(exons=len(x[2])) for x in txs]


# ---- the last exon of a transcript ------------------------------------------------------------------------------------------------------
def last_exon(next_ref):
    """transcript A's last exon is directly followed in the exon arrays by transcript B's first one, with a junction row exactly on
    [A's last end, B's first begin): it counts for neither.  next_ref: B lies on the next reference at the same coordinates, and the row
    is there on both.  B's last exon is the table's very last; a junction row begins at its end"""
    tb = 1 if next_ref else 0
    iv = [(0, 100, 200, 2.0), (0, 300, 400, 3.0), (tb, 500, 600, 5.0), (tb, 700, 800, 7.0)]
    jn = [(0, 200, 300, "+", 2.0), (0, 400, 500, "+", 64.0)] + ([(1, 400, 500, "+", 128.0)] if next_ref else []) + [(tb, 600, 700, "+", 3.0), (tb, 800, 900, "+", 256.0)]
    txs = [(0, "+", [(100, 200), (300, 400)], "A"), (tb, "+", [(500, 600), (700, 800)], "B")]
    C = [dict(junc=[2.0], junc_min=2.0, introns_hit=1, covered=200, exons_hit=2, max=3.0, JS=2), dict(junc=[3.0], junc_min=3.0, introns_hit=1, covered=200, max=7.0, JS=3)]
    return fs.rows_of(iv, jn), table(txs), C


# ---- an exon's run at the threshold between the two paths, and whole tiles -------------------------------------------------------------
def run_exons():
    """multi-exon transcripts on reference 1 of feature_scenes.run_rows() whose middle exon has a run of FS_DIRECT - 1 / + 0 / + 1 rows,
    and one whose middle exon reads two whole tiles' aggregates"""
    txs, C = [], []

    def add(ga, gb, path, tiles):
        mid = fs.run_feature(ga, gb)[1:]
        first, last = exon_on_row(ga - fs.HEAD - 2), exon_on_row(gb - fs.HEAD + 1)
        txs.append((1, ".", [first, mid, last]))
        C.append(dict(exons=3, exons_hit=3, parts=[dict(path="direct", hi_lo=1), dict(path=path, tiles=tiles, lo=ga, hi=gb, hi_lo=gb - ga), dict(path="direct", hi_lo=1)]))
    for n in (D - 1, D, D + 1):
        add(40, 40 + n, "direct" if n <= D else "agg", 0)
    add(T - 1, 3 * T + 1, "agg", 2)
    return fs.rows_of(fs.run_rows()), table(txs), C


# ---- exons without a row, references without rows, the largest coordinates -------------------------------------------------------------
def empties():
    """the rows of feature_scenes.edges(): references 0 and 3 carry no row, 5 lies behind the last one"""
    rows = fs.edges()[0]
    txs = [(0, ".", [(0, 10), (20, 30)]), (1, ".", [(260, 290), (400, 500)]), (5, "+", [(100, 200)]), (3, "-", [(1, 2), (5, 6), (9, 10)]),
           (1, ".", [(0, 50), (120, 180), (251, 299), (300, 1000)]), (4, ".", [(0, 2 ** 33)])]
    zero = dict(covered=0, S=0, max=0.0, exons_hit=0, introns_hit=0, junc_min=0.0)
    C = [dict(zero), dict(zero), dict(zero, exons=1, introns=0), dict(zero), dict(covered=61, S=187, max=7.0, exons_hit=2, exons=4), dict(covered=10, S=20, max=2.0, exons_hit=1)]
    return rows, table(txs), C


def top():
    """cov_scenes.TOP: the largest value over the longest row; the product needs 62 bits, so that transcript's `sum` is held to the bound"""
    rows = fs.top()[0]
    rows.update({k: v for k, v in fs.rows_of([], [(0, 5, TOP - 10, "-", 3.0)]).items() if k[:2] == "j_"})
    txs = [(0, "-", [(0, 5), (TOP - 10, TOP - 1)]), (0, ".", [(0, TOP - 1)]), (1, "+", [(0, 10), (TOP - 2, TOP)])]
    C = [dict(covered=14, S=14 * TOP, max=float(TOP), junc=[3.0], introns_hit=1), dict(covered=TOP - 1, max=float(TOP)), dict(covered=1, S=TOP, exons_hit=1)]
    return rows, table(txs), C


# ---- introns ---------------------------------------------------------------------------------------------------------------------------
def introns():
    """the junction rows of feature_scenes.junctions() and a chain on reference 2; no interval row at all"""
    jn = [(0, 100, 200, "+", 2.0), (0, 100, 200, "-", 3.0), (0, 100, 200, ".", 5.0), (0, 100, 300, "+", 7.0), (0, 150, 200, "-", 11.0),
          (1, 100, 200, "+", 13.0), (1, 500, 900, ".", 17.0), (2, 100, 200, "+", 5.0), (2, 300, 400, "+", 2.0), (2, 500, 600, "+", 9.0)]
    txs, C = [], []

    def add(tid, strand, exons, **claim):
        txs.append((tid, strand, exons)), C.append(dict(claim, covered=0, exons_hit=0))
    for s, v in (("+", 2.0), ("-", 3.0), (".", 10.0)):               # rows on '+', '-' and '.', asked with each strand
        add(0, s, [(50, 100), (200, 250)], junc=[v], junc_min=v, JS=int(v), introns_hit=1)
    for s, v in (("+", 7.0), ("-", 0.0), (".", 7.0)):                # the same start with another end
        add(0, s, [(50, 100), (300, 350)], junc=[v], junc_min=v, introns_hit=int(v > 0))
    add(0, ".", [(50, 99), (200, 250)], junc=[0.0]), add(0, ".", [(50, 100), (201, 250)], junc=[0.0])       # a base off at either end
    add(0, "-", [(120, 150), (200, 260)], junc=[11.0]), add(0, "+", [(120, 150), (200, 260)], junc=[0.0])
    add(1, "-", [(50, 100), (200, 250)], junc=[0.0]), add(1, ".", [(50, 100), (200, 250)], junc=[13.0])    # the same coordinates on the neighbour
    add(1, "+", [(400, 500), (900, 950)], junc=[0.0]), add(1, ".", [(400, 500), (900, 950)], junc=[17.0])  # a '.' row against '+' and '.'
    add(0, "+", [(50, 100), (200, 210), (300, 350)], junc=[2.0, 0.0], introns=2, introns_hit=1, junc_min=0.0, JS=2)          # one unsupported among supported
    add(2, "+", [(50, 100), (200, 300), (400, 500), (600, 700)], junc=[5.0, 2.0, 9.0], introns_hit=3, junc_min=2.0, JS=16)   # a true minimum, in the middle
    add(2, "-", [(50, 100), (200, 300), (400, 500), (600, 700)], junc=[0.0, 0.0, 0.0], introns_hit=0, junc_min=0.0, JS=0)
    add(3, ".", [(50, 100), (200, 300)], junc=[0.0])                 # behind the last junction row
    return fs.rows_of([], jn), table(txs), C


# ---- isoforms --------------------------------------------------------------------------------------------------------------------------
def isoforms():
    """isoforms that share exons, a duplicate transcript, transcripts in descending order of their starts (feature_scenes.edges() rows)"""
    rows = fs.edges()[0]
    rows.update({k: v for k, v in fs.rows_of([], [(1, 200, 240, ".", 4.0), (1, 200, 300, "+", 6.0), (1, 250, 300, "-", 8.0)]).items() if k[:2] == "j_"})
    a, b = [(100, 200), (300, 301)], [(100, 200), (240, 250), (300, 301)]
    txs = [(2, ".", [(150, 230)], "late"), (1, "+", a, "A"), (1, ".", b, "B"), (1, "+", a, "A2"), (1, "-", b, "B-"), (1, ".", [(90, 100)], "early")]
    C = [dict(covered=80, S=50 * 11 + 30 * 13), dict(covered=101, S=307, junc=[6.0], max=7.0), dict(covered=111, S=357, junc=[4.0, 8.0], junc_min=4.0, JS=12),
         dict(covered=101, S=307, junc=[6.0]), dict(junc=[0.0, 8.0], introns_hit=1, junc_min=0.0), dict(covered=0, exons_hit=0)]
    return rows, table(txs), C


SCENES = {"sizes": sizes, "thirds": thirds, "last_exon_same_ref": lambda: last_exon(False), "last_exon_next_ref": lambda: last_exon(True), "run_exons": run_exons,
          "empties": empties, "top": top, "introns": introns, "isoforms": isoforms}
SCENES.update({"list%d" % n: (lambda n=n: tx_list(n)) for n in LIST_N})


# ---- a seeded random case --------------------------------------------------------------------------------------------------------------
def random_case(seed=20240611, n_tx=300):
    """the rows of feature_scenes.random_case (values that are multiples of 1/8; reference 2 carries no row) under transcripts of 1 to 12
    exons: random ones, ones built on a junction row (fully supported), ones with a second, invented intron (partly supported), long
    exons that read aggregates, transcripts on the reference without rows"""
    rows, _ = fs.random_case()
    rng = np.random.RandomState(seed)
    nj = len(rows["j_tid"])
    txs = []
    for k in range(n_tx):
        kind = k % 6
        if kind in (0, 1):
            j = int(rng.randint(nj))
            t, s, e, st = int(rows["j_tid"][j]), int(rows["j_start"][j]), int(rows["j_end"][j]), chr(int(rows["j_strand"][j]))
            ex = [(s - int(rng.randint(5, 60)), s), (e, e + int(rng.randint(5, 60)))]
            if kind == 1:
                ex.append((ex[-1][1] + int(rng.randint(1, 30)), ex[-1][1] + 200))
            txs.append((t, st if k % 4 else ".", ex))
            continue
        t = (0, 1, 3, 2)[int(rng.randint(4))] if kind != 5 else 2
        n = (1, 1, 2, 3, 5, 12)[int(rng.randint(6))]
        p, ex = int(rng.randint(900, 30000)), []
        for _ in range(n):
            ln = int(rng.randint(5, 300)) if kind != 4 else int(rng.randint(7000, 12000))
            ex.append((p, p + ln))
            p += ln + int(rng.randint(1, 400))
        txs.append((t, "+-."[int(rng.randint(3))], ex))
    return rows, table(txs)


# ---- the golden tracks -----------------------------------------------------------------------------------------------------------------
def golden_gtf(rows, names, lens, seed=7):
    """GTF lines for a golden's rows as an annotation would hold them: chains of the golden's own junction rows on one strand with
    flanking exons, single-exon transcripts on coverage rows, one transcript with an invented intron; `transcript` and `CDS` lines,
    comments and a blank line between, minus-strand transcripts listed descending, a quoted value with a ';', a bare value, a line
    without gene_id, CR at a line's end"""
    rng = np.random.RandomState(seed)
    out = ["# transcripts on the golden rows", "##format: gtf"]
    n = 0

    def emit(tid, strand, exons, gene=True):
        nonlocal n
        tx_id = "TX%03d.1" % n
        attr = 'transcript_id "%s";' % tx_id + (' gene_id "G%02d"; note "a;b";' % (n % 7) if gene else "") + " level 2;"
        if n % 5 == 3:
            attr = "gene_name X%d; transcript_id %s" % (n, tx_id) + ("; gene_id G%02d" % (n % 7) if gene else "")   # bare values
        chrom = names[tid]
        out.append("\t".join([chrom, "model", "transcript", str(exons[0][0] + 1), str(exons[-1][1]), ".", strand, ".", attr]))
        order = exons[::-1] if strand == "-" else (exons if n % 3 else [exons[k] for k in rng.permutation(len(exons))])
        for b, e in order:
            out.append("\t".join([chrom, "model", "exon", str(b + 1), str(e), ".", strand, ".", attr]) + ("\r" if n % 4 == 2 else ""))
            if n % 2:
                out.append("\t".join([chrom, "model", "CDS", str(b + 1), str(e), ".", strand, "0", attr]))
        n += 1
    J = sorted(zip(rows["j_tid"].tolist(), rows["j_strand"].tolist(), rows["j_start"].tolist(), rows["j_end"].tolist()))
    for start in range(len(J)):                                       # every junction row opens a chain of up to four on its strand
        t, s, b, e = J[start]
        chain = [(b, e)]
        for t2, s2, b2, e2 in J[start + 1:]:
            if (t2, s2) == (t, s) and b2 > chain[-1][1] and len(chain) < 4:
                chain.append((b2, e2))
        exons = [(max(0, chain[0][0] - 40), chain[0][0])] + [(chain[k][1], chain[k + 1][0]) for k in range(len(chain) - 1)] + [(chain[-1][1], min(lens[t], chain[-1][1] + 55))]
        emit(t, chr(s) if start % 3 else ".", exons)
    iv = list(zip(rows["iv_tid"].tolist(), rows["iv_start"].tolist(), rows["iv_end"].tolist()))
    for i in rng.permutation(len(iv))[:25]:                           # single-exon transcripts on coverage rows
        t, b, e = iv[i]
        emit(t, "+-."[i % 3], [(max(0, b - i % 4), e + i % 3)], gene=bool(i % 2))
    out.append("")
    keys = {(t, b, e) for t, _, b, e in J}
    t, b, e = max(iv, key=lambda r: r[2] - r[1])                      # an intron nobody saw, inside the longest row
    assert e - b >= 30 and (t, b + 10, b + 20) not in keys
    emit(t, ".", [(b, b + 10), (b + 20, b + 30)])
    return out
