#!/usr/bin/env python3
"""Wall times of the tracks: `tiebrush -o`, `tiecov -c -j -s` on its output, and `tiebrush -o --cov --junc --samp` in one run, each
as a child process; and the text of the tracks by the device formatter (tbk_format_track) against the host formatter (snprintf on every
core, TBK_TRACK_HOST_FMT=1) inside the fused run, on the same rows.  Inputs: tools/e2e_leg.py's synthetic BAMs, the SEQ / QUAL leg
(config-2 read model) and config 3's read model with --clip.  Prints ONE JSON object (committed under profiles/)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "tiebrush_amd", "_build")
T_RUN = 600


def timed(args, env=None):
    time.sleep(1.0)   # (tools/e2e_leg.py: a run of its own, after the previous process's device memory went back)
    t = time.time()
    r = subprocess.run(args, capture_output=True, text=True, timeout=T_RUN, env=dict(os.environ, TBK_TIMING="1", **(env or {})))
    dt = time.time() - t
    if r.returncode != 0:
        raise RuntimeError("%s exited with %d: %s" % (os.path.basename(args[0]), r.returncode, r.stderr[-2000:]))
    return dt, r


def median(xs):
    return sorted(xs)[len(xs) // 2]


def leg(files, reads, profile, flags, seq, runs, desc):
    import torch

    from tiebrush_amd import synth, synth_dev
    d = tempfile.mkdtemp(prefix="tbk_tracks_", dir="/tmp")
    try:
        tile = synth_dev.tile_to_host(synth_dev.make_tile_device(files, reads, profile, device="cuda:0"))
        torch.cuda.empty_cache()
        paths = synth.write_bams_fast(tile, os.path.join(d, "in"), seq=seq)
        n = tile.n_records
        del tile
        os.sync()
        out, pre = os.path.join(d, "out.bam"), os.path.join(d, "t")
        tb = [os.path.join(BIN, "tiebrush")] + flags
        tracks = ["--cov", pre + "_f", "--junc", pre + "_f", "--samp", pre + "_fs"]
        res = {"workload": desc % (files, reads), "records": n, "runs": runs}
        walls = {k: [] for k in ("tiebrush", "tiecov", "fused", "fused_host_text")}
        for _ in range(runs):
            dt, _ = timed(tb + ["-o", out] + paths)
            walls["tiebrush"].append(dt)
            dt, _ = timed([os.path.join(BIN, "tiecov"), "-c", pre + "_r", "-j", pre + "_r", "-s", pre + "_rs", out])
            walls["tiecov"].append(dt)
            dt, rf = timed(tb + tracks + ["-o", out] + paths)
            walls["fused"].append(dt)
            dt, rh = timed(tb + tracks + ["-o", out] + paths, env=dict(TBK_TRACK_HOST_FMT="1"))
            walls["fused_host_text"].append(dt)
        for k, v in walls.items():
            res[k + "_wall_s"] = round(median(v), 3)
            res[k + "_wall_s_all"] = [round(x, 3) for x in sorted(v)]
        res["fused_minus_tiebrush_s"] = round(res["fused_wall_s"] - res["tiebrush_wall_s"], 3)
        res["fused_extra_over_tiecov"] = round(res["fused_minus_tiebrush_s"] / res["tiecov_wall_s"], 3)
        # the same bytes as tiecov's
        same = all(open(pre + a, "rb").read() == open(pre + b, "rb").read()
                   for a, b in (("_f.bedgraph", "_r.bedgraph"), ("_f.bed", "_r.bed"), ("_fs.bedgraph", "_rs.bedgraph")))
        res["tracks_identical_to_tiecov"] = same
        res["track_bytes"] = {s: os.path.getsize(pre + s) for s in ("_r.bedgraph", "_r.bed", "_rs.bedgraph")}
        res["lines"] = {s: sum(1 for _ in open(pre + s, "rb")) - 1 for s in ("_r.bedgraph", "_r.bed", "_rs.bedgraph")}
        pick = lambda r: [ln for ln in r.stderr.split("\n") if ln.startswith("tracks")][-2:]
        res["fused_track_lines"], res["fused_host_text_track_lines"] = pick(rf), pick(rh)
        m = lambda r: float(re.search(r"text \+ write ([0-9.]+)", r.stderr).group(1))
        res["text_ms_device_formatter"], res["text_ms_host_formatter"] = m(rf), m(rh)
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    res = {"tool": "tools/tracks_bench.py", "cpu_threads": os.environ.get("OMP_NUM_THREADS")}
    res["seq"] = leg(a.files, a.reads, "c2", [], True, a.runs, "%d files x %d reads (config-2 read model) WITH 100-bp SEQ / QUAL, default collapse")
    res["c3"] = leg(2 * a.files, max(1, a.reads // 2), "c3", ["--clip"], False, a.runs,
                    "%d files x %d reads (config-3 read model: 10 %% soft-clipped), --clip")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
