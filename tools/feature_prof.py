#!/usr/bin/env python3
"""tbk_cov_summary on the coverage rows of a synthetic tile (default: config 3 at full size) against seeded features (default: one
million): per-kernel times and the call's (tbk_set_profiling / kernel_times), the host summariser on the same arrays, and a check that the
two agree.  Usage: feature_prof.py [profile files reads features reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tiebrush_amd import api, synth_dev

prof = sys.argv[1] if len(sys.argv) > 1 else "c3"
nf = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nr = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000_000
n_feat = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
kw = {"c2": {}, "c3": dict(strategy="clip"), "c5": dict(strategy="exon", max_nh=5, min_qual=1)}[prof]
FS_DIRECT = 256                                   # featsum.hip

dt = synth_dev.make_tile_device(nf, nr, prof, device="cuda:0")
ctx = api.Context(0)
g = ctx.collapse(dt, **kw)
dev_rows = ctx.coverage(ctx.groups_to_cov_in(g))
dev_rows = {k: v for k, v in dev_rows.items() if k[:3] == "iv_" or k[:2] == "j_"}
rows = {k: v.cpu().numpy() for k, v in dev_rows.items()}
ni, nj = len(rows["iv_tid"]), len(rows["j_tid"])

# seeded features: exon-sized windows at rows (6 in 10), gene-sized ones (2 in 10), the junction rows themselves as introns (2 in 10),
# and a whole reference now and then
rng = np.random.RandomState(12345)
pick = rng.randint(0, ni, n_feat)
kind = rng.randint(0, 10, n_feat)
size = np.where(kind < 6, rng.randint(50, 2000, n_feat), rng.randint(5000, 200000, n_feat)).astype(np.int64)
tid = rows["iv_tid"][pick].astype(np.int32)
beg = np.maximum(0, rows["iv_start"][pick].astype(np.int64) - rng.randint(0, 200, n_feat))
end = beg + size
strand = np.frombuffer(b"+-.", np.uint8)[rng.randint(0, 3, n_feat)].copy()
if nj:
    jp = rng.randint(0, nj, n_feat)
    isj = kind >= 8
    tid[isj], beg[isj], end[isj] = rows["j_tid"][jp][isj], rows["j_start"][jp][isj], rows["j_end"][jp][isj]
whole = np.arange(0, n_feat, max(1, n_feat // 16))
beg[whole], end[whole] = 0, 2 ** 31 - 1
feats = dict(tid=tid, beg=beg, end=end, strand=strand)

# the runs, for the share of features on the aggregate path: rows whose 64-bit keys (tid << 32 | coordinate) bracket the feature
key_end = (rows["iv_tid"].astype(np.int64) << 32) | rows["iv_end"].astype(np.int64)
key_start = (rows["iv_tid"].astype(np.int64) << 32) | rows["iv_start"].astype(np.int64)
lo = np.searchsorted(key_end, (tid.astype(np.int64) << 32) | beg, side="right")
hi = np.searchsorted(key_start, (tid.astype(np.int64) << 32) | np.minimum(end, 2 ** 31 - 1), side="left")
run = np.maximum(hi - lo, 0)

def timed(rws, on):
    ctx.set_profiling(on)
    acc = {}
    got = ctx.cov_summary(rws, feats)            # warm-up: the arena and the code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        got = ctx.cov_summary(rws, feats)
        if on:
            for k, (ms, ln) in ctx.kernel_times().items():
                a = acc.setdefault(k, [0.0, 0]); a[0] += ms; a[1] += ln
    wall = (time.perf_counter() - t0) / reps
    ctx.set_profiling(False)
    return got, wall, acc

got, wall_dev, _ = timed(dev_rows, False)
_, wall_dev_prof, acc = timed(dev_rows, True)
_, wall_host_rows, _ = timed(rows, False)
t0 = time.perf_counter()
want = api.cov_summary_host(rows, feats)
wall_host = time.perf_counter() - t0
for k in ("covered", "sum", "max", "junc"):
    assert np.array_equal(got[k], want[k]), "device and host summariser disagree on " + k
print("rows %d  junction rows %d  features %d  with a row %d  aggregate path %d (%.1f %%)  longest run %d" %
      (ni, nj, n_feat, int((run > 0).sum()), int((run > FS_DIRECT).sum()), 100.0 * (run > FS_DIRECT).mean(), int(run.max())))
print("tbk_cov_summary, rows on the device, results to the host: %.3f ms a call (profiling on: %.3f ms); rows from the host: %.3f ms" %
      (wall_dev * 1e3, wall_dev_prof * 1e3, wall_host_rows * 1e3))
for k, (ms, ln) in sorted(acc.items(), key=lambda kv: -kv[1][0]):
    print("  %-20s %8.3f ms/call  %3d launches" % (k, ms / reps, ln // reps))
print("host summariser (one core, plain loops): %.1f ms; the two results are equal" % (wall_host * 1e3))
