#!/usr/bin/env python3
"""Wall times of `tiecov -c -j -s` on a collapsed BAM: plain tracks, `--tabix` (the text formatted, deflated and indexed on the GPU:
tbk_track_bgzf), and `--tabix` with TBK_TRACK_HOST_FMT=1 (snprintf, zlib level 6 and the index builder on the cores), each as a child
process, medians of --runs runs; the `tabix phase ms` lines and the .gz sizes of the two writers.  With --parent-bin DIR (the build
directory of the parent commit) the plain line is also taken with that tiecov, interleaved with this one's: --tabix must not cost the
plain tracks anything.  Inputs: the two shapes of tools/tracks_bench.py.  Prints ONE JSON object (committed as
profiles/tabix_bench.json)."""
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
SUF = {"c": ".bedgraph", "j": ".bed", "s": ".bedgraph"}


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


def leg(files, reads, profile, flags, seq, runs, desc, parent_bin):
    import torch

    from tiebrush_amd import synth, synth_dev
    d = tempfile.mkdtemp(prefix="tbk_tabix_", dir="/tmp")
    try:
        tile = synth_dev.tile_to_host(synth_dev.make_tile_device(files, reads, profile, device="cuda:0"))
        torch.cuda.empty_cache()
        paths = synth.write_bams_fast(tile, os.path.join(d, "in"), seq=seq)
        n = tile.n_records
        del tile
        os.sync()
        out = os.path.join(d, "out.bam")
        timed([os.path.join(BIN, "tiebrush")] + flags + ["-o", out] + paths)
        opts = lambda pre: [x for o in "cjs" for x in ("-" + o, os.path.join(d, pre + o))]
        lines = {"plain": ([os.path.join(BIN, "tiecov")] + opts("p") + [out], None),
                 "tabix": ([os.path.join(BIN, "tiecov"), "--tabix"] + opts("t") + [out], None),
                 "tabix_host": ([os.path.join(BIN, "tiecov"), "--tabix"] + opts("h") + [out], dict(TBK_TRACK_HOST_FMT="1"))}
        if parent_bin:
            lines["plain_parent"] = ([os.path.join(parent_bin, "tiecov")] + opts("q") + [out], None)
        res = {"workload": desc % (files, reads), "records": n, "runs": runs}
        walls = {k: [] for k in lines}
        last = {}
        for _ in range(runs):                      # the lines alternate: what drifts on a shared machine drifts for all of them
            for k, (args, env) in lines.items():
                dt, last[k] = timed(args, env)
                walls[k].append(dt)
                print("%s %s %.3f s" % (profile, k, dt), file=sys.stderr, flush=True)
        for k, v in walls.items():
            res[k + "_wall_s"] = round(median(v), 3)
            res[k + "_wall_s_all"] = [round(x, 3) for x in sorted(v)]
        if parent_bin:
            res["plain_within_parent_spread"] = min(walls["plain_parent"]) <= res["plain_wall_s"] <= max(walls["plain_parent"])
            res["parent_tracks_identical"] = all(open(os.path.join(d, "p" + o + SUF[o]), "rb").read() == open(os.path.join(d, "q" + o + SUF[o]), "rb").read()
                                                 for o in "cjs")
        res["tabix_minus_plain_s"] = round(res["tabix_wall_s"] - res["plain_wall_s"], 3)
        res["tabix_host_minus_plain_s"] = round(res["tabix_host_wall_s"] - res["plain_wall_s"], 3)
        phase = lambda r: [ln for ln in r.stderr.split("\n") if ln.startswith("tabix phase ms")]
        res["tabix_phase_lines"], res["tabix_host_phase_lines"] = phase(last["tabix"]), phase(last["tabix_host"])
        ms = lambda ls: round(sum(float(re.search(r"\| ([0-9.]+)$", ln).group(1)) for ln in ls), 1)
        res["tabix_phase_ms_device"], res["tabix_phase_ms_host"] = ms(res["tabix_phase_lines"]), ms(res["tabix_host_phase_lines"])
        res["plain_bytes"] = {o: os.path.getsize(os.path.join(d, "p" + o + SUF[o])) for o in "cjs"}
        res["lines"] = {o: sum(1 for _ in open(os.path.join(d, "p" + o + SUF[o]), "rb")) - 1 for o in "cjs"}
        res["gz_bytes_device"] = {o: os.path.getsize(os.path.join(d, "t" + o + SUF[o] + ".gz")) for o in "cjs"}
        res["gz_bytes_host"] = {o: os.path.getsize(os.path.join(d, "h" + o + SUF[o] + ".gz")) for o in "cjs"}
        ixp = lambda o: next(p for p in (os.path.join(d, "t" + o + SUF[o] + ".gz" + e) for e in (".tbi", ".csi")) if os.path.exists(p))
        res["index_bytes_device"] = {o: os.path.getsize(ixp(o)) for o in "cjs"}
        # the same text from both writers, and the plain track's
        import zlib

        def inflate(path):
            z, out_, at = open(path, "rb").read(), [], 0
            while at < len(z):
                dec = zlib.decompressobj(31)
                out_.append(dec.decompress(z[at:]))
                at = len(z) - len(dec.unused_data)
            return b"".join(out_)
        res["gz_inflates_to_plain"] = all(inflate(os.path.join(d, w + o + SUF[o] + ".gz")) == open(os.path.join(d, "p" + o + SUF[o]), "rb").read()
                                          for w in "th" for o in "cjs")
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-bin", default="", help="the parent commit's tiebrush_amd/_build: its tiecov takes the plain line too")
    ap.add_argument("--only", default="", help="seq or c3: one shape")
    a = ap.parse_args()
    res = {"tool": "tools/tabix_bench.py", "cpu_threads": os.environ.get("OMP_NUM_THREADS")}
    if a.only in ("", "seq"):
        res["seq"] = leg(a.files, a.reads, "c2", [], True, a.runs, "%d files x %d reads (config-2 read model) WITH 100-bp SEQ / QUAL, default collapse", a.parent_bin)
    if a.only in ("", "c3"):
        res["c3"] = leg(2 * a.files, max(1, a.reads // 2), "c3", ["--clip"], False, a.runs,
                        "%d files x %d reads (config-3 read model: 10 %% soft-clipped), --clip", a.parent_bin)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
