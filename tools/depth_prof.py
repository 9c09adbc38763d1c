#!/usr/bin/env python3
"""tbk_cov_thresholds on the rows and features of tools/feature_prof.py (config 3 at full size, one million seeded features) at 1, 4 and
16 thresholds: the call's time and its two kernels' (tbk_set_profiling / kernel_times), beside tbk_cov_summary on the same inputs and
the host loop, and a check that device and host give the same counts.  One warm-up call and `reps` timed calls each.
Usage: depth_prof.py [profile files reads features reps]"""
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
THR = {1: [10.0], 4: [1.0, 10.0, 100.0, 1000.0], 16: [1.0, 2.0, 3.0, 5.0, 8.0, 10.0, 15.0, 20.0, 30.0, 50.0, 100.0, 200.0, 500.0, 1000.0, 5000.0, 30000.0]}

dt = synth_dev.make_tile_device(nf, nr, prof, device="cuda:0")
ctx = api.Context(0)
g = ctx.collapse(dt, **kw)
dev_rows = ctx.coverage(ctx.groups_to_cov_in(g))
dev_rows = {k: v for k, v in dev_rows.items() if k[:3] == "iv_" or k[:2] == "j_"}
rows = {k: v.cpu().numpy() for k, v in dev_rows.items()}
ni, nj = len(rows["iv_tid"]), len(rows["j_tid"])

# feature_prof.py's features, draw for draw: exon-sized windows at rows (6 in 10), gene-sized ones (2 in 10), the junction rows
# themselves as introns (2 in 10), and a whole reference now and then
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


def timed(call, on):
    ctx.set_profiling(on)
    acc = {}
    got = call()                                 # warm-up: the arena and the code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        got = call()
        if on:
            for k, (ms, ln) in ctx.kernel_times().items():
                a = acc.setdefault(k, [0.0, 0]); a[0] += ms; a[1] += ln
    wall = (time.perf_counter() - t0) / reps
    ctx.set_profiling(False)
    return got, wall, acc


print("rows %d  features %d  reps %d (one warm-up call before each timed series)" % (ni, n_feat, reps))
_, wall_sum, _ = timed(lambda: ctx.cov_summary(dev_rows, feats), False)
_, _, acc = timed(lambda: ctx.cov_summary(dev_rows, feats), True)
print("tbk_cov_summary, rows on the device, results to the host: %.3f ms a call" % (wall_sum * 1e3))
for k, (ms, ln) in sorted(acc.items(), key=lambda kv: -kv[1][0]):
    print("  %-20s %8.3f ms/call  %3d launches" % (k, ms / reps, ln // reps))
t0 = time.perf_counter()
api.cov_summary_host(rows, feats)
print("host summariser (one core, plain loops): %.1f ms" % ((time.perf_counter() - t0) * 1e3))
for nt in (1, 4, 16):
    thr = THR[nt]
    got, wall, _ = timed(lambda: ctx.cov_thresholds(dev_rows, feats, thr, out="host"), False)
    _, _, acc = timed(lambda: ctx.cov_thresholds(dev_rows, feats, thr, out="host"), True)
    _, wall_dd, _ = timed(lambda: ctx.cov_thresholds(dev_rows, feats, thr), False)
    t0 = time.perf_counter()
    want = api.cov_thresholds_host(rows, feats, thr)
    wall_host = time.perf_counter() - t0
    for k in ("covered", "ge"):
        assert np.array_equal(got[k], want[k]), "device and host disagree on " + k
    print("tbk_cov_thresholds, %2d thresholds, rows on the device: results to the host %.3f ms a call, results on the device %.3f ms; host loop %.1f ms; the counts are equal"
          % (nt, wall * 1e3, wall_dd * 1e3, wall_host * 1e3))
    for k, (ms, ln) in sorted(acc.items(), key=lambda kv: -kv[1][0]):
        print("  %-20s %8.3f ms/call  %3d launches" % (k, ms / reps, ln // reps))
