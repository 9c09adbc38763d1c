"""CPU model of the collapse driver's route decision (tiebrush_amd/csrc/collapse_plan.hpp; driver: collapse.hip, tbk_collapse_device).

It restates the decision the way the driver made it before the plan existed: a handful of interleaved flags (use_runs, runs_min,
use_win, part, use_raw, lean) set one after the other, and hand-overs that assign to those flags and go round the retry loop again.
numpy only; every function takes scalars or arrays that broadcast.  tests/test_collapse_plan_cpu.py demands the same answers of the
header, tests/test_gpu_routes.py the model's first route of the device."""
import numpy as np

RAW_WINDOW, COMPACTED_WINDOW, SORT = 1, 2, 3          # TBK_ROUTE_* (include/tbk.h)
FORM = {RAW_WINDOW: "raw", COMPACTED_WINDOW: "compacted", SORT: "sort"}   # tiebrush_amd.api.Context.collapse_route()["form"]
COLLISION, FRACTIONAL, BIGBUCKET, RAWORDER = 1 << 1, 1 << 5, 1 << 8, 1 << 9   # TBK_DERR_* (tbk_internal.h)
UNSORTED = 1 << 0                                     # ... one of the bits that are the input's fault
STRAT_FULL = 1
TBM_NONE, TBM_SOME, TBM_ALL = 0, 1, 2                  # tbk_soa_in.tbmerged: no file flagged (or no array), some, every file
DONE, RESEED, RESTART, ERROR = 0, 1, 2, 3
MAX_SEEDS = 4

AXES = ("n", "cig", "k", "tbm", "prio", "carried", "strategy", "store_frac", "collapse_same", "path", "raw", "sort")


def window_supported(k):
    return (k >= 1) & (k <= 1024)


def plan(n, cig, k, tbm=TBM_NONE, prio=0, carried=0, strategy=0, store_frac=0, collapse_same=0, path=0, raw=-1, sort=0):
    """-> dict(route, part, use_runs, runs_min, lean): the flags as they stood when the retry loop was entered"""
    n, cig, k, tbm, prio, carried, strategy, store_frac, collapse_same, path, raw, sort = np.broadcast_arrays(
        *[np.asarray(x, np.int64) for x in (n, cig, k, tbm, prio, carried, strategy, store_frac, collapse_same, path, raw, sort)])
    prio, carried, store_frac, collapse_same = prio != 0, carried != 0, store_frac != 0, collapse_same != 0
    use_runs = k <= 64
    runs_min = np.full(n.shape, 32768, np.int64)
    use_runs = np.where(sort != 0, (sort != 1) & (use_runs | (sort == 2)), use_runs)
    runs_min = np.where(sort == 2, 0, runs_min)
    no_tbm = tbm == TBM_NONE
    use_win = window_supported(k) & ~store_frac & ~collapse_same & ((n >= (8 << 20)) | ((k > 64) & (n >= 65536))) & no_tbm
    use_win = np.where(path == 1, False, use_win)
    use_win = np.where(path == 2, window_supported(k) & ~store_frac & ~collapse_same & no_tbm, use_win)
    part = (tbm == TBM_ALL) & prio & carried & (k <= 64) & ~store_frac & ~collapse_same & (strategy != STRAT_FULL)
    part = part & (path != 1)
    part = part & ((n >= 65536) | (path == 2))
    use_win = use_win | part
    use_raw = use_win & (raw != 0)
    use_raw = use_raw | part
    big = (n >= (1 << 30)) | (cig >= (1 << 30))
    use_raw = use_raw & ~big
    use_win = use_win & ~(big & part)
    part = part & ~big
    lean = use_runs & ~store_frac & (tbm == TBM_NONE) & (n >= runs_min)
    route = np.where(use_raw & use_win, RAW_WINDOW, np.where(use_win, COMPACTED_WINDOW, SORT))
    return dict(route=route, part=part, use_runs=use_runs, runs_min=runs_min, lean=lean)


def old_arena_lean(n, cig, k, tbm=TBM_NONE, prio=0, carried=0, strategy=0, store_frac=0, collapse_same=0, path=0, raw=-1, sort=0):
    """the predicate tbk_collapse_tile restated for its arena hints before it read the plan (a tile on the device)"""
    n, k, tbm, prio, store_frac, collapse_same, path, raw = [np.asarray(x, np.int64) for x in (n, k, tbm, prio, store_frac, collapse_same, path, raw)]
    return ((store_frac == 0) & (collapse_same == 0) & (prio == 0) & (path == 0) & (raw < 0) &
            ((n >= (8 << 20)) | ((k > 64) & (n >= 65536))) & (tbm == TBM_NONE))


def after(p, eb):
    """one turn of the retry loop's error handling.  p: dict(route, part, use_runs, runs_min, lean) of scalars, eb: the device's error
    bits when the route came back -> (action, plan to go on with, raw_handed_back, big_bucket)"""
    use_win, use_raw, part = p["route"] != SORT, p["route"] == RAW_WINDOW, bool(p["part"])
    use_runs, lean = bool(p["use_runs"]), bool(p["lean"])
    handed = big = False
    action = None
    if use_raw and use_win:
        if eb & (RAWORDER | BIGBUCKET | FRACTIONAL):
            use_raw = False
            handed, big = bool(eb & RAWORDER), bool(eb & BIGBUCKET)
            if (eb & (BIGBUCKET | FRACTIONAL)) or part:
                use_win = False
            part = False
            action = RESTART
    elif use_win:
        if eb & BIGBUCKET:
            use_win, big, action = False, True, RESTART
    elif lean and (eb & BIGBUCKET):
        use_runs, lean, action = False, False, RESTART
    if action is None:
        action = RESEED if eb & COLLISION else ERROR if eb else DONE
    q = dict(route=RAW_WINDOW if use_raw and use_win else COMPACTED_WINDOW if use_win else SORT, part=part, use_runs=use_runs,
             runs_min=int(p["runs_min"]), lean=lean)
    return action, q, handed, big


ERR_BITS = [a | b | c | d | e for a in (0, COLLISION) for b in (0, FRACTIONAL) for c in (0, BIGBUCKET) for d in (0, RAWORDER) for e in (0, UNSORTED)]


def longest_chain(p, after=after, bits=ERR_BITS):
    """the most restarts and the most seeds any sequence of error bits can make of plan p before the loop ends -> (restarts, seeds);
    the loop itself gives up after MAX_SEEDS seeds"""
    best = (0, 1)
    stack, seen = [(p, 0, 1)], set()
    while stack:
        q, restarts, seeds = stack.pop()
        state = (key(q), restarts, seeds)
        if state in seen:
            continue
        seen.add(state)
        assert restarts < 64, "the hand-overs loop"
        best = (max(best[0], restarts), max(best[1], seeds))
        for eb in bits:
            action, nxt, _, _ = after(q, eb)
            if action == RESTART:
                stack.append((nxt, restarts + 1, seeds))
            elif action == RESEED and seeds < MAX_SEEDS:
                stack.append((q, restarts, seeds + 1))
    return best


def key(p):
    """a plan of scalars as a tuple, in the order the probe prints it"""
    return (int(p["route"]), int(bool(p["part"])), int(bool(p["use_runs"])), int(p["runs_min"]), int(bool(p["lean"])))


def from_key(t):
    return dict(zip(("route", "part", "use_runs", "runs_min", "lean"), t))
