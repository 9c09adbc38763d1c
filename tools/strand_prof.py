#!/usr/bin/env python3
"""tbk_cov_split_strand on the collapsed records of a synthetic tile (default: config 3 at full size): medians over `reps` calls, after
a warm-up call, of the split's kernels (profiling on), the split call, one coverage call on the whole view and the three coverage calls
on the parts (intervals only, as --strand-cov runs them); and the split's rate over its algorithmic bytes — the input columns read twice
and written once — as a fraction of HBM peak.
Usage: strand_prof.py [profile files reads reps]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from tiebrush_amd import api, synth_dev

prof = sys.argv[1] if len(sys.argv) > 1 else "c3"
nf = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nr = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000_000
reps = max(5, int(sys.argv[4])) if len(sys.argv) > 4 else 7
kw = {"c2": {}, "c3": dict(strategy="clip"), "c5": dict(strategy="exon", max_nh=5, min_qual=1)}[prof]
dt = synth_dev.make_tile_device(nf, nr, prof, device="cuda:0")
ctx = api.Context(0)
g = ctx.collapse(dt, **kw)
view = ctx.groups_to_cov_in(g)
n, nc = view.n_records, view.n_cigar_ops


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def median_of(f):
    f()                                                   # warm-up
    return statistics.median(timed(f)[0] for _ in range(reps))


parts = ctx.cov_split_strand(view)
counts = [p.n_records for p in parts]
words = [p.n_cigar_ops for p in parts]
# per record tid, pos, strand, yc, yx and one offset; a view of collapsed groups carries no flag column
rec_bytes = 4 + 4 + 1 + 8 + 8 + 4
b_alg = 2 * (n * rec_bytes + 4 * nc) + (sum(counts) * rec_bytes + 4 * sum(words))
ctx.set_profiling(True)
acc = {}
ctx.cov_split_strand(view)
for _ in range(reps):
    ctx.cov_split_strand(view)
    for k, (ms, ln) in ctx.kernel_times().items():
        acc.setdefault(k, []).append(ms)
ctx.set_profiling(False)
kern = {k: statistics.median(v) for k, v in acc.items()}
ms_split = median_of(lambda: ctx.cov_split_strand(view))
bufs, pb = {}, [{}, {}, {}]
ms_whole = median_of(lambda: ctx.coverage(view, want_junc=False, out=bufs, raw=True))
parts = ctx.cov_split_strand(view)
ms_parts = median_of(lambda: [ctx.coverage(p, want_junc=False, out=pb[k], raw=True) for k, p in enumerate(parts)])
print("records %d (+ %d, - %d, . %d)  CIGAR words %d  algorithmic bytes %.3f GB" % (n, counts[0], counts[1], counts[2], nc, b_alg / 1e9))
for k, ms in sorted(kern.items(), key=lambda kv: -kv[1]):
    print("  %-16s %8.3f ms" % (k, ms))
ks = sum(kern.values())
print("split kernels: %.3f ms -> %.1f GB/s algorithmic = %.3f of 8 TB/s" % (ks, b_alg / (ks * 1e-3) / 1e9, b_alg / (ks * 1e-3) / 8e12))
print("split call: %.3f ms" % ms_split)
print("coverage call on the whole view (intervals only): %.3f ms" % ms_whole)
print("coverage calls on the three parts: %.3f ms" % ms_parts)
print("split / whole coverage call: %.2f" % (ms_split / ms_whole))
