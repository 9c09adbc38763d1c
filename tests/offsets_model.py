"""Numpy model of the offsets pass of the window path's raw form (wgroup.hip: wg_offsets_stream_k<true> / wg_offsets_wave_k, then
wg_offsets_edges_k and wg_offsets_transpose_k), and the hand-built scenes tests/test_gpu_offsets_pass.py runs through both kernels.

The matrix: off[0, f] = start of run f, off[nW + 1, f] = its end, off[r + 1, f] = the first record of run f whose key is >= W[r]
(the run's end where there is none; an empty run: its start everywhere); wbase[r] = the records of all runs before row r.
A scene is (tid, pos, run_off, W, flagged): `flagged` scenes hold a file whose raw keys decrease somewhere — the pass must raise
TBK_DERR_RAWORDER and still keep every entry inside its run."""
import numpy as np

ST = 1024            # records of a step of the wave kernel (WV_ST); the block kernel's chunk is two of them (WG_OC)
TC = 4096            # records per chunk of reference ids (WG_TC)
UNPLACED = 1 << 62


def raw_key(tid, pos):
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    return np.where(tid < 0, np.uint64(UNPLACED), (tid.astype(np.uint64) << np.uint64(31)) | (pos.astype(np.uint64) & np.uint64(0x7FFFFFFF)))


def offsets(tid, pos, run_off, W):
    """-> off [nW + 2, k] uint32, wbase [nW + 2] uint32 (sorted runs)"""
    key, W = raw_key(tid, pos), np.asarray(W, np.uint64)
    k, nW = len(run_off) - 1, len(W)
    off = np.zeros((nW + 2, k), np.uint32)
    for f in range(k):
        a, b = int(run_off[f]), int(run_off[f + 1])
        off[0, f], off[nW + 1, f] = a, b
        off[1:nW + 1, f] = a + np.searchsorted(key[a:b], W, side="left")
    wbase = (off.astype(np.int64) - np.asarray(run_off[:-1], np.int64)[None, :]).sum(axis=1).astype(np.uint32)
    return off, wbase


def runs_sorted(tid, pos, run_off):
    key = raw_key(tid, pos)
    return all(bool(np.all(key[int(a) + 1:int(b)] >= key[int(a):int(b) - 1])) for a, b in zip(run_off[:-1], run_off[1:]) if b - a > 1)


def bounds_in_step(tid, pos, run_off, W, step):
    """bounds r whose answer lies inside records [step * ST, (step + 1) * ST) of a one-file scene: key before < W[r] <= last key"""
    key, W = raw_key(tid, pos), np.asarray(W, np.uint64)
    i0, i1 = step * ST, min(len(key), (step + 1) * ST)
    below = W > key[i0 - 1] if i0 else np.ones(len(W), bool)
    return int(np.count_nonzero(below & (W <= key[i1 - 1])))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def pairs(vals, tail=True):
    """bounds around the given keys as the splitter kernel makes them: (v, v) and (v, v + 1) alternately, with one bound below every
    key and one above (tail)"""
    vals = np.unique(np.asarray(vals, np.uint64))
    second = vals + (np.arange(len(vals)) % 2).astype(np.uint64)
    W = np.concatenate([vals, second] + ([np.array([0, UNPLACED + 5], np.uint64)] if tail else []))
    return np.sort(W)


def cat(files, W=None, every=23, flagged=False):
    """files: [(tid, pos)] per run (scalars of tid are broadcast); W None: pairs around every `every`-th key in sorted order"""
    tids = [np.broadcast_to(np.asarray(t, np.int32), np.shape(p)).astype(np.int32) for t, p in files]
    poss = [np.asarray(p, np.int64).astype(np.int32) for _, p in files]
    run_off = np.concatenate([[0], np.cumsum([len(p) for p in poss])]).astype(np.uint32)
    tid, pos = np.concatenate(tids), np.concatenate(poss)
    if W is None:
        W = pairs(np.sort(raw_key(tid, pos))[::every])
    return tid, pos, run_off, np.asarray(W, np.uint64), flagged


def spos(rng, n, span=None):
    return np.sort(rng.integers(0, span if span else 5 * n + 10, n))


def deal(rng, k, n, ntid=1):
    """n sorted records dealt to k files at random, order kept"""
    tid = np.sort(rng.integers(0, ntid, n))
    pos = np.concatenate([spos(rng, int(c), 4000) for c in np.bincount(tid, minlength=ntid)])
    owner = rng.integers(0, k, n)
    return [(tid[owner == f], pos[owner == f]) for f in range(k)]


def sized(sizes, seed=5, span=9000):
    rng = np.random.default_rng(seed)
    return [(0, spos(rng, s, span)) for s in sizes]


def one_step_bounds(count):
    """3000 records 10 apart, `count` distinct bounds inside the second step and none elsewhere"""
    pos = np.arange(3000) * 10
    W = raw_key(0, pos[ST] + np.arange(count) * (10 * ST // count))
    return cat([(0, pos)], W=np.sort(W))


def inversion(at, n, k=1):
    """one file of n records (and k - 1 sorted ones behind it) whose record at - 1 lies 1 beyond record `at`"""
    pos = np.arange(n) * 3
    pos[at - 1] += 4
    rng = np.random.default_rng(at)
    return cat([(0, pos)] + [(0, spos(rng, 700, 3 * n)) for _ in range(k - 1)], every=37, flagged=True)


def _scenes():
    S = {}
    rng = np.random.default_rng(11)
    for n in (1, 15, 16, 17, 1023, 1024, 1025, 2049, 16385):   # 2049 / 16385: a wave's whole range plus one record (wg_og = 1 / 8)
        S["size-%d" % n] = cat([(0, spos(rng, n))], every=5 if n < 3000 else 61)
    for k in (1, 2, 64):
        S["runs-k%d" % k] = cat(deal(rng, k, 5000, ntid=2))
    S["boundary-at-16j"] = cat(sized([1600, 1408, 700]))
    S["boundary-at-16j-1"] = cat(sized([1599, 1409, 700]))
    S["boundary-at-16j+1"] = cat(sized([1601, 1407, 700]))
    S["files-inside-a-lane"] = cat(sized([1000, 1, 2, 1, 3, 1, 1, 2000]))
    S["run-ends-at-step-end"] = cat(sized([1024, 1024, 500]))
    S["run-ends-at-chunk-end"] = cat(sized([2048, 100, 1948, 30]))
    S["empty-runs"] = cat(sized([0, 0, 1500, 0, 700, 0, 0, 0, 900, 0]))
    S["only-empty-but-one"] = cat(sized([0, 0, 0, 1300]))
    S["second-file-below-first"] = cat([(0, 5000 + spos(rng, 1500, 900)), (0, spos(rng, 1500, 900))], every=11)
    base = [(0, spos(rng, 2600, 7000)), (0, spos(rng, 900, 7000))]
    S["bounds-none"] = cat(base, W=np.zeros(0, np.uint64))
    S["bounds-all-equal"] = cat(base, W=np.full(100, 3500, np.uint64))
    S["bounds-equal-pairs"] = cat(base, W=np.repeat(raw_key(0, base[0][1][::50]), 2))
    S["bounds-below-second-run"] = cat([(0, spos(rng, 1500, 1000)), (0, 5000 + spos(rng, 1500, 1000))], W=pairs(np.arange(5, 1000, 7), tail=False))
    S["bounds-above-first-run"] = cat([(0, spos(rng, 1500, 1000)), (0, 5000 + spos(rng, 1500, 1000))],
                                      W=pairs(np.arange(5005, 6000, 7), tail=False))
    for c in (63, 64, 65, 300):
        S["bounds-%d-in-one-step" % c] = one_step_bounds(c)
    pile = np.concatenate([np.arange(500), np.full(3 * ST + 600, 700), 800 + np.arange(500)])
    S["pile-up-three-steps"] = cat([(0, pile), (0, spos(rng, 300, 1400))], W=pairs([3, 699, 700, 701, 900]))
    t = np.repeat([0, 1], [1500, 1500])
    S["tid-change-in-step"] = cat([(t, np.concatenate([spos(rng, 1500), spos(rng, 1500)]))])
    t = np.repeat([0, 1, 2], [1501, 1, 1498])
    S["tid-change-in-lane"] = cat([(t, np.concatenate([spos(rng, 1501), [7], spos(rng, 1498)]))])
    t = np.repeat([0, 1], [3000, 2000])
    S["mixed-chunk"] = cat([(t, np.concatenate([spos(rng, 3000), spos(rng, 2000)])), (t[::2], np.concatenate([spos(rng, 1500), spos(rng, 1000)]))])
    t = np.repeat([0, 3, -1], [1200, 1000, 300])
    S["unplaced-tail"] = cat([(t, np.concatenate([spos(rng, 1200), spos(rng, 1000), np.full(300, -1)]))] * 2)
    top = np.concatenate([spos(rng, 1500, 2 ** 31 - 1), [2 ** 31 - 1] * 3])
    S["pos-2^31-1"] = cat([(5, top), (5, top[::3])], W=pairs(raw_key(5, top[::40].tolist() + [2 ** 31 - 1])))
    S["inversion-in-lane"] = inversion(1002, 3000)
    S["inversion-between-lanes"] = inversion(1004, 3000)
    S["inversion-between-quads"] = inversion(1024 + 256, 3000)
    S["inversion-between-steps"] = inversion(1024, 3000, k=2)
    S["inversion-between-chunks"] = inversion(2048, 5000)
    S["inversion-between-ranges"] = inversion(16384, 20000)
    S["inversion-last-record"] = inversion(2999, 3000, k=2)
    return S


SCENES = _scenes()
FLAGGED = [n for n, s in SCENES.items() if s[4]]
CLEAN = [n for n, s in SCENES.items() if not s[4]]
