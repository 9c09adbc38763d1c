#!/usr/bin/env python3
"""tbk_tx_summary on the coverage rows of a synthetic tile (default: config 3 at full size) against a seeded annotation (default: 200 000
transcripts; most are short, a few have hundreds of exons), beside what the library could do for the same question without it — the
flat route: tbk_cov_summary over the exons and the introns as flat features, the part columns copied down, the fold on the host — and
beside the host summariser on one core.  One warm-up call, then `reps` timed calls of each route, alternated; the host clock around calls
that end in a synchronise, the kernel times from the context's events.  Every column of the three results is asserted equal (YC is
integral).  Usage: tx_prof.py [profile files reads transcripts reps out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tiebrush_amd import api, synth_dev

prof = sys.argv[1] if len(sys.argv) > 1 else "c3"
nf = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nr = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000_000
n_tx = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000
reps = max(5, int(sys.argv[5])) if len(sys.argv) > 5 else 5
out_json = sys.argv[6] if len(sys.argv) > 6 else None
kw = {"c2": {}, "c3": dict(strategy="clip"), "c5": dict(strategy="exon", max_nh=5, min_qual=1)}[prof]

dt = synth_dev.make_tile_device(nf, nr, prof, device="cuda:0")
ctx = api.Context(0)
g = ctx.collapse(dt, **kw)
dev_rows = ctx.coverage(ctx.groups_to_cov_in(g))
dev_rows = {k: v for k, v in dev_rows.items() if k[:3] == "iv_" or k[:2] == "j_"}
rows = {k: v.cpu().numpy() for k, v in dev_rows.items()}
ni, nj = len(rows["iv_tid"]), len(rows["j_tid"])

# the seeded annotation.  Exon counts: 70 % of the transcripts have 1-4 exons, 25 % 5-20, 4.5 % 21-100, 0.5 % 101-400.  A transcript
# starts at a coverage row; exons of 50-400 bases, introns of 100-5000; in three of ten transcripts with an intron the first intron is a
# junction row of the tile (so some introns are supported)
rng = np.random.RandomState(4242)
u = rng.rand(n_tx)
size = np.where(u < 0.70, rng.randint(1, 5, n_tx), np.where(u < 0.95, rng.randint(5, 21, n_tx), np.where(u < 0.995, rng.randint(21, 101, n_tx), rng.randint(101, 401, n_tx))))
off = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
n_ex = int(off[-1])
ex_tx = np.repeat(np.arange(n_tx), size)
first = np.zeros(n_ex, bool)
first[off[:-1]] = True
pick = rng.randint(0, ni, n_tx)
tid = rows["iv_tid"][pick].astype(np.int32)
start = rows["iv_start"][pick].astype(np.int64)
ex_len = rng.randint(50, 401, n_ex).astype(np.int64)
gap = rng.randint(100, 5001, n_ex).astype(np.int64)
gap[first] = 0
if nj:                                                     # the first intron of some transcripts: a junction row
    jp = rng.randint(0, nj, n_tx)
    use = (size >= 2) & (rng.rand(n_tx) < 0.3) & (rows["j_start"][jp] > 400)
    tid[use] = rows["j_tid"][jp][use]
    start[use] = rows["j_start"][jp][use].astype(np.int64) - ex_len[off[:-1]][use]
    second = off[:-1][use] + 1
    gap[second] = (rows["j_end"][jp][use].astype(np.int64) - rows["j_start"][jp][use].astype(np.int64))
step = gap + np.concatenate([[0], ex_len[:-1]])            # from an exon's begin to the next one's, within a transcript
step[first] = 0
run = np.cumsum(step)
span = (run + ex_len)[off[1:] - 1] - run[off[:-1]]
start = np.maximum(0, np.minimum(start, 2 ** 31 - 2 - span))   # (a transcript that would run off the coordinate range is moved down)
ex_beg = start[ex_tx] + run - run[off[:-1]][ex_tx]
ex_end = ex_beg + ex_len
strand = np.frombuffer(b"+-.", np.uint8)[rng.randint(0, 3, n_tx)].copy()
tx = dict(tx_off=off.astype(np.uint32), tid=tid, strand=strand, ex_beg=ex_beg, ex_end=ex_end)

# the flat route: exons and introns as features of tbk_cov_summary
has_in = ~np.concatenate([first[1:], [True]])             # exon e has an intron behind it
flat = dict(tid=np.concatenate([tid[ex_tx], tid[ex_tx][has_in]]), beg=np.concatenate([ex_beg, ex_end[has_in]]), end=np.concatenate([ex_end, ex_beg[1:][has_in[:-1]]]),
            strand=np.concatenate([np.full(n_ex, ord("."), np.uint8), strand[ex_tx][has_in]]))
with_in = np.flatnonzero(size >= 2)
in_off = np.concatenate([[0], np.cumsum(size - 1)])[:-1]


def flat_route():
    r = ctx.cov_summary(dev_rows, flat)                    # (the part columns come down inside the call)
    ec, es, em, j = r["covered"][:n_ex], r["sum"][:n_ex], r["max"][:n_ex], r["junc"][n_ex:]
    o = off[:-1]
    res = dict(covered=np.add.reduceat(ec, o), sum=np.add.reduceat(es, o), max=np.maximum.reduceat(em, o), exons_hit=np.add.reduceat((ec > 0).astype(np.uint32), o),
               introns_hit=np.zeros(n_tx, np.uint32), junc_min=np.zeros(n_tx), junc_sum=np.zeros(n_tx))
    if len(with_in):
        io = in_off[with_in]
        res["introns_hit"][with_in] = np.add.reduceat((j > 0).astype(np.uint32), io)
        res["junc_min"][with_in] = np.minimum.reduceat(j, io)
        res["junc_sum"][with_in] = np.add.reduceat(j, io)
    return res


def device_route():
    return ctx.tx_summary(dev_rows, tx)


routes = {"tx_summary": device_route, "flat": flat_route}
got = {k: f() for k, f in routes.items()}                  # warm-up: the arena and the code objects
torch.cuda.synchronize()
wall = {k: [] for k in routes}
for _ in range(reps):                                      # alternated
    for k, f in routes.items():
        t0 = time.perf_counter()
        got[k] = f()
        wall[k].append((time.perf_counter() - t0) * 1e3)
kern = {}
for k, f in routes.items():
    ctx.set_profiling(True)
    acc = {}
    for _ in range(reps):
        f()
        for name, (ms, ln) in ctx.kernel_times().items():
            a = acc.setdefault(name, [0.0, 0]); a[0] += ms; a[1] += ln
    ctx.set_profiling(False)
    kern[k] = {name: round(ms / reps, 4) for name, (ms, ln) in acc.items()}
t0 = time.perf_counter()
want = api.tx_summary_host(rows, tx)
wall_host = (time.perf_counter() - t0) * 1e3
COLS = ("covered", "sum", "max", "exons_hit", "introns_hit", "junc_min", "junc_sum")
for k in COLS:
    for r in routes:
        assert np.array_equal(got[r][k], want[k]), "%s and the host summariser disagree on %s" % (r, k)
stat = {k: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)), calls=len(v)) for k, v in wall.items()}
claim = stat["tx_summary"]["mean"] < stat["flat"]["min"]
res = dict(profile=prof, files=nf, reads=nr, interval_rows=ni, junction_rows=nj, transcripts=n_tx, exons=n_ex, introns=int(n_ex - n_tx),
           exon_count_distribution="70% 1-4, 25% 5-20, 4.5% 21-100, 0.5% 101-400", largest_transcript=int(size.max()),
           transcripts_covered=int((want["covered"] > 0).sum()), transcripts_with_a_supported_intron=int((want["introns_hit"] > 0).sum()),
           wall_ms=stat, kernel_ms=kern, host_summariser_ms=wall_host, device_fold_faster_than_flat_route=bool(claim), results_equal=True)
print("rows %d  junction rows %d  transcripts %d  exons %d (largest %d)  covered %d  with a supported intron %d" %
      (ni, nj, n_tx, n_ex, int(size.max()), res["transcripts_covered"], res["transcripts_with_a_supported_intron"]))
for k in routes:
    print("%-12s mean %.3f ms  min %.3f  max %.3f over %d calls; kernels: %s" % (k, stat[k]["mean"], stat[k]["min"], stat[k]["max"], reps,
          ", ".join("%s %.3f" % kv for kv in sorted(kern[k].items(), key=lambda kv: -kv[1]))))
print("host summariser (one core, plain loops): %.1f ms; the three results are equal in every column" % wall_host)
print("claim 'the device fold is faster than the flat route' (mean below the other's minimum): %s" % ("met" if claim else "NOT met"))
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
