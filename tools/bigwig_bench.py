#!/usr/bin/env python3
"""The bigWig stage, measured.  Two parts, one JSON object on stdout:
  full   the coverage track of config 3's collapsed output as tools/cov_prof.py builds it (device rows): per-kernel times of
         tbk_bigwig_build (the library's events), its wall time with profiling off, and the size of its streams against zlib level 6
         on the same payloads (what the host producer's compress2 calls write);
  cli    `tiecov -W` with each writer on the collapsed output of `tiebrush --clip` over synthetic BAMs of the same read model, the runs
         alternated: the "bigwig phase" lines of TBK_TIMING.
Usage: bigwig_bench.py [--files 64 --reads 5000000] [--cli-files 32 --cli-reads 500000 --runs 5]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 2), mean=round(sum(xs) / len(xs), 2), max=round(xs[-1], 2), n=len(xs))


def full(files, reads, reps):
    import torch

    from tiebrush_amd import api, synth, synth_dev
    dt = synth_dev.make_tile_device(files, reads, "c3", device="cuda:0")
    ctx = api.Context(0)
    g = ctx.collapse(dt, strategy="clip")
    view = ctx.groups_to_cov_in(g)
    c = ctx.coverage(view, want_junc=False)
    n = c["n_intervals"]
    rows = [c[k][:n].clone() for k in ("iv_tid", "iv_start", "iv_end", "iv_val")]
    del dt, g, view, c
    torch.cuda.empty_cache()
    lens = synth.REF_LENS
    res = {"workload": "%d files x %d reads, config-3 read model, collapsed with --clip" % (files, reads), "rows": int(n)}
    levels = ctx.bigwig_build(*rows, lens)   # warm-up: code objects, the encoder's buffers, the pinned slices
    res["levels"] = [dict(reduction=lv["reduction"], n_items=lv["n_items"], sections=len(lv["sections"]), bytes=len(lv["bytes"])) for lv in levels]
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.bigwig_build(*rows, lens)
        walls.append((time.perf_counter() - t) * 1e3)
    res["build_wall_ms_device_rows"] = stats(walls)
    host_rows = [r.cpu().numpy() for r in rows]
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.bigwig_build(*host_rows, lens)
        walls.append((time.perf_counter() - t) * 1e3)
    res["build_wall_ms_host_rows"] = stats(walls)
    ctx.set_profiling(True)
    acc = {}
    for _ in range(reps):
        ctx.bigwig_build(*rows, lens)
        for k, (ms, ln) in ctx.kernel_times().items():
            a = acc.setdefault(k, [0.0, 0])
            a[0] += ms
            a[1] += ln
    ctx.set_profiling(False)
    res["kernel_ms_per_build"] = {k: dict(ms=round(ms / reps, 3), launches=ln // reps) for k, (ms, ln) in sorted(acc.items(), key=lambda kv: -kv[1][0])}
    # the same payloads through zlib level 6, section by section: the host producer's bytes
    dev_b = host_b = 0
    t = time.perf_counter()
    for lv in levels:
        for _c, _s, _e, off, size in lv["sections"]:
            dev_b += size
            host_b += len(zlib.compress(zlib.decompress(lv["bytes"][off:off + size]), 6))
    res["section_bytes"] = dict(device=dev_b, zlib6=host_b, ratio=round(dev_b / host_b, 4), python_zlib_round_trip_s=round(time.perf_counter() - t, 2))
    ctx.close()
    return res


def cli(files, reads, runs):
    import torch

    from tiebrush_amd import synth, synth_dev
    d = tempfile.mkdtemp(prefix="tbk_bw_", dir="/tmp")
    try:
        tile = synth_dev.tile_to_host(synth_dev.make_tile_device(files, reads, "c3", device="cuda:0"))
        torch.cuda.empty_cache()
        paths = synth.write_bams_fast(tile, os.path.join(d, "in"), seq=False)
        del tile
        out = os.path.join(d, "out.bam")
        subprocess.run([os.path.join(BIN, "tiebrush"), "--clip", "-o", out] + paths, check=True, capture_output=True, timeout=600)
        res = {"workload": "%d files x %d reads, config-3 read model, tiebrush --clip, tiecov -W on its output" % (files, reads), "runs": runs}
        phase = {"host": [], "device": []}
        wall = {"host": [], "device": []}
        for _ in range(runs):
            for w in ("host", "device"):   # alternated
                pre = os.path.join(d, "bw_" + w)
                t = time.perf_counter()
                r = subprocess.run([os.path.join(BIN, "tiecov"), "-W", "--bigwig-writer", w, "-c", pre, out], capture_output=True, text=True,
                                   timeout=600, env=dict(os.environ, TBK_TIMING="1"))
                wall[w].append(time.perf_counter() - t)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                m = re.search(r"bigwig phase ms: writer (\w+) \| (\d+) rows \| ([0-9.]+)", r.stderr)
                assert m and m.group(1) == w, r.stderr
                res["rows"] = int(m.group(2))
                phase[w].append(float(m.group(3)))
        res["bigwig_phase_ms"] = {w: dict(stats(v), all=[round(x, 1) for x in v]) for w, v in phase.items()}
        res["tiecov_wall_s"] = {w: stats(v) for w, v in wall.items()}
        res["file_bytes"] = {w: os.path.getsize(os.path.join(d, "bw_" + w + ".bigwig")) for w in phase}
        res["file_ratio_device_over_host"] = round(res["file_bytes"]["device"] / res["file_bytes"]["host"], 4)
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--cli-files", type=int, default=32)
    ap.add_argument("--cli-reads", type=int, default=500_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    res = {"tool": "tools/bigwig_bench.py", "cpu_threads": os.environ.get("OMP_NUM_THREADS")}
    if "cli" not in a.skip:
        res["cli"] = cli(a.cli_files, a.cli_reads, a.runs)
        print(json.dumps({"cli": res["cli"]}), file=sys.stderr, flush=True)
    if "full" not in a.skip:
        res["full"] = full(a.files, a.reads, a.runs)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
