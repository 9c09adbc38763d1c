"""The route plan and the hand-over table of the collapse driver (tiebrush_amd/csrc/collapse_plan.hpp) against the model that restates
the decision flag by flag (route_model.py), without a GPU.  The header is compiled into tests/support/collapse_plan_probe.cpp, a plain
program — once as it is and once under the address and undefined-behaviour sanitizers — and both answer for the full grid of tile
shapes, options and debug keys at every threshold of the decision."""
import os
import subprocess

import numpy as np
import pytest

import route_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "support", "collapse_plan_probe.cpp")

GRID = dict(
    n=[0, 1, 32767, 32768, 65535, 65536, 2**23 - 1, 2**23, 2**30 - 1, 2**30],
    cig=[0, 2**30 - 1, 2**30],
    k=[1, 2, 64, 65, 1024, 1025, 65535],
    tbm=[rm.TBM_NONE, rm.TBM_SOME, rm.TBM_ALL],
    prio=[0, 1], carried=[0, 1],
    strategy=[0, 1, 2, 3],
    store_frac=[0, 1], collapse_same=[0, 1],
    path=[0, 1, 2], raw=[-1, 0], sort=[0, 1, 2])
assert tuple(GRID) == rm.AXES


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cp") / "collapse_plan_probe")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, PROBE], check=True)
    return exe


@pytest.fixture(scope="module")
def mesh():
    axes = np.meshgrid(*[np.asarray(GRID[a], np.int64) for a in rm.AXES], indexing="ij")   # (the probe's order: the first axis slowest)
    return {a: x.ravel() for a, x in zip(rm.AXES, axes)}


@pytest.fixture(scope="module")
def want(mesh):
    return rm.plan(**mesh)


def _grid(probe):
    r = subprocess.run([probe, "grid"] + ["%s=%s" % (a, ",".join(map(str, GRID[a]))) for a in rm.AXES], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.array(r.stdout.split(), np.int64).reshape(-1, 6)


def _after(probe, pairs):
    """pairs: (plan key, error bits) -> (action, plan key to go on with, raw_handed_back, big_bucket) each, of the header's table"""
    r = subprocess.run([probe, "after"], input="".join("%d %d %d %d %d %d\n" % (k + (eb,)) for k, eb in pairs), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array(r.stdout.split(), np.int64).reshape(-1, 8)
    assert len(got) == len(pairs)
    return [(int(g[0]), tuple(int(x) for x in g[1:6]), bool(g[6]), bool(g[7])) for g in got]


def test_plan_over_the_grid(probe, mesh, want):
    got = _grid(probe)
    assert len(got) == len(mesh["n"]) == int(np.prod([len(v) for v in GRID.values()]))
    for col, name in enumerate(("route", "part", "use_runs", "runs_min", "lean")):
        bad = np.flatnonzero(got[:, col] != want[name].astype(np.int64))
        assert bad.size == 0, (name, {a: int(mesh[a][bad[0]]) for a in rm.AXES}, int(got[bad[0], col]))
    # every route and every flag occurs, on either side of each threshold
    assert set(np.unique(got[:, 0]).tolist()) == {rm.RAW_WINDOW, rm.COMPACTED_WINDOW, rm.SORT}
    assert set(map(tuple, np.unique(got[:, 1:5], axis=0).tolist())) >= {(1, 1, 32768, 0), (0, 0, 32768, 0), (0, 1, 0, 1), (0, 1, 32768, 1)}
    assert not np.any((got[:, 1] == 1) & (got[:, 0] != rm.RAW_WINDOW))                       # the PART form exists in raw mode only


def test_hand_overs_and_termination(probe, want):
    starts = sorted(set(zip(*[want[c].astype(np.int64).tolist() for c in ("route", "part", "use_runs", "runs_min", "lean")])))
    table, todo = {}, list(starts)
    while todo:                                      # the closure of the grid's plans under the table's restarts
        pairs = [(k, eb) for k in todo for eb in rm.ERR_BITS]
        todo = []
        for (k, eb), got in zip(pairs, _after(probe, pairs)):
            action, q, handed, big = rm.after(rm.from_key(k), eb)
            assert got == (action, rm.key(q), handed, big), (k, hex(eb), got)
            table[(k, eb)] = got
            if got[0] == rm.RESTART and (got[1], 0) not in table and got[1] not in todo:
                todo.append(got[1])
    assert {a for a, _, _, _ in table.values()} == {rm.DONE, rm.RESEED, rm.RESTART, rm.ERROR}
    # the rows, one by one
    raw, rawp = (rm.RAW_WINDOW, 0, 1, 32768, 1), (rm.RAW_WINDOW, 1, 1, 32768, 0)
    comp, lean, sort = (rm.COMPACTED_WINDOW, 0, 1, 32768, 1), (rm.SORT, 0, 1, 32768, 1), (rm.SORT, 0, 1, 32768, 0)
    assert table[(raw, rm.RAWORDER)] == (rm.RESTART, comp, True, False)
    assert table[(rawp, rm.RAWORDER)] == (rm.RESTART, sort, True, False)
    assert table[(raw, rm.BIGBUCKET)] == (rm.RESTART, lean, False, True)
    assert table[(rawp, rm.FRACTIONAL)] == (rm.RESTART, sort, False, False)
    assert table[(comp, rm.BIGBUCKET)] == (rm.RESTART, lean, False, True)
    assert table[(lean, rm.BIGBUCKET)] == (rm.RESTART, (rm.SORT, 0, 0, 32768, 0), False, False)
    assert table[(sort, rm.BIGBUCKET)][0] == rm.ERROR and table[(comp, rm.RAWORDER)][0] == rm.ERROR
    for k in (raw, rawp, comp, lean, sort):
        assert table[(k, rm.COLLISION)] == (rm.RESEED, k, False, False) and table[(k, 0)] == (rm.DONE, k, False, False)
        assert table[(k, rm.UNSORTED)][0] == rm.ERROR and table[(k, rm.UNSORTED | rm.COLLISION)][0] == rm.RESEED
    # no chain of hand-overs is longer than four restarts plus four seeds: the retry loop ends
    for k in starts:
        restarts, seeds = rm.longest_chain(rm.from_key(k), after=lambda p, eb: (lambda g: (g[0], rm.from_key(g[1]), g[2], g[3]))(table[(rm.key(p), eb)]))
        assert restarts <= 4 and seeds <= rm.MAX_SEEDS, (k, restarts, seeds)
    assert max(rm.longest_chain(rm.from_key(k))[0] for k in starts) == 3               # raw -> compacted -> lean sort -> radix sort


def test_arena_hint_differs_only_where_the_old_predicate_was_wrong(probe, mesh, want):
    got = _grid(probe)[:, 5].astype(bool)
    old = rm.old_arena_lean(**mesh)
    differ = got != old
    # the old predicate said "raw form" for tiles that never take it: more files than the window path holds, and tiles the raw kernels'
    # 32-bit offsets cannot address — there the hint is the other routes' now, everywhere else it keeps its value
    named = old & ((mesh["k"] > 1024) | (mesh["n"] >= 2**30) | (mesh["cig"] >= 2**30))
    assert np.array_equal(differ, named)
    assert not got[differ].any() and np.all(want["route"][differ] != rm.RAW_WINDOW)
    assert np.any(named & (mesh["k"] > 1024) & (mesh["n"] == 65536)) and np.any(named & (mesh["n"] == 2**30)) and np.any(named & (mesh["cig"] == 2**30) & (mesh["n"] < 2**30))
    assert np.array_equal(got, old & (want["route"] == rm.RAW_WINDOW))                # where the predicate named the route taken, it stands
