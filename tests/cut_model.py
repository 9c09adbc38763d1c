"""CPU model of the cut search of the group-partials protocol in its "lists" form (include/tbk.h, the ABI 7 block around
TBK_PARTIAL_BUNDLES; tiebrush_amd/csrc/shard.hip: partial_keys_k .. partial_tabx_k).  numpy only: nothing here imports the library
except rounds_cut, which walks with the product's own host restatement of its probes.

Two independent statements of one contract:
  * keys / meta / targets / cands / choose / cuts_sorted / table restate the header's wording entry for entry — the device must
    produce the same arrays;
  * exact_cut is the definition itself: the smallest key at or behind the target, among the target and every group start of every
    rank, that no group of any rank that starts before it reaches (keyed end (tid + 1) << 31 | end + 1 below the key).  It knows
    nothing of bundles, heads or lists, so it also catches a model that copies a mistake of the kernels.
A cut the lists settle equals exact_cut; a cut they leave unsettled has its exact_cut at or beyond some rank's horizon (or has
none): tests/test_cut_model_cpu.py shows both on every scene of cut_scenes.py, tests/test_gpu_cut_search.py demands the model's
arrays of the device."""
import numpy as np

INF = 1 << 62
BUNDLES = 15                    # TBK_PARTIAL_BUNDLES
CAND = 2 + 2 * BUNDLES          # TBK_PARTIAL_CAND
SAMPLES = 64
META = SAMPLES + 4              # TBK_PARTIAL_META
STEP = 256                      # partial_cands_k walks a block of 256 groups at a time
LIMIT = 1 << 22                 # groups it looks at before it gives up


def K(tid, coord):
    """the 64-bit key of a coordinate: (tid + 1) << 31 | coordinate"""
    return ((int(tid) + 1) << 31) | int(coord)


def keys(groups):
    """groups: (tid, start, end) triples, 1-based inclusive, sorted by (tid, start) -> key [ng], emax [ng] (tbk_partial_keys)"""
    g = np.asarray(groups, np.int64).reshape(-1, 3)
    key = ((g[:, 0] + 1) << 31) | g[:, 1]
    endk = ((g[:, 0] + 1) << 31) | (g[:, 2] + 1)
    assert np.all(key[1:] >= key[:-1]), "groups must come in (tid, start) order"
    return key, (np.maximum.accumulate(endk) if len(g) else np.zeros(0, np.int64))


def meta(key):
    """the 64 sampled keys of a rank: key[i * ng // 64], 1 << 62 without groups"""
    ng = len(key)
    if ng == 0:
        return np.full(SAMPLES, INF, np.int64)
    return np.asarray(key, np.int64)[(np.arange(SAMPLES, dtype=np.int64) * ng) // SAMPLES]


def meta_row(key, n_files=1, first_fidx=0, bad=0, carry=0):
    """the whole row a rank gathers: samples, n_files, first_fidx, not packable, carry"""
    return np.concatenate([meta(key), np.array([n_files, first_fidx, bad, carry], np.int64)])


def targets(allmeta, world):
    """the j / world quantiles (j = 1 .. world - 1) of the valid samples of all ranks; 1 << 62 when there is none"""
    s = np.sort(np.asarray(allmeta, np.int64).reshape(world, -1)[:, :SAMPLES].reshape(-1))
    s = s[s < INF]
    nv = len(s)
    return np.array([int(s[(j * nv) // world]) if nv else INF for j in range(1, world)], np.int64)


def heads_of(key, emax):
    """a group opens a local bundle when it starts beyond everything before it"""
    h = np.ones(len(key), bool)
    h[1:] = key[1:] > emax[:-1]
    return h


def walk(key, emax, t):
    """the walk of partial_cands_k from the lower bound of t in steps of 256 groups -> (idx0, indices of the first <= 16 heads,
    where the walk stood when it ended, whether it gave up at the limit)"""
    ng = len(key)
    idx0 = int(np.searchsorted(key, t, side="left"))
    head = heads_of(key, emax)
    found, nheads, base, hit_limit = [], 0, idx0, False
    while base < ng:
        if base - idx0 >= LIMIT:
            hit_limit = True
            break
        here = np.flatnonzero(head[base:base + STEP]) + base
        found.extend(int(i) for i in here[:max(0, BUNDLES + 1 - nheads)])       # ranks beyond 15 are dropped
        nheads += len(here)
        if nheads > BUNDLES:
            break
        base += STEP
    return idx0, found[:BUNDLES + 1], base, hit_limit


def horizon_source(key, emax, t):
    """which of the three sources the horizon of this list comes from: "head16", "limit" or "none\""""
    _, hd, _, hit_limit = walk(key, emax, t)
    return "head16" if len(hd) == BUNDLES + 1 else ("limit" if hit_limit else "none")


def heads_behind(key, emax, t):
    """all local bundle heads at or behind the target (not only those the walk stores)"""
    idx0 = int(np.searchsorted(key, t, side="left"))
    return int(heads_of(key, emax)[idx0:].sum())


def cands(key, emax, t):
    """the TBK_PARTIAL_CAND words of one rank for one cut: {farthest end before the first local bundle start at or behind the
    target (-1: nothing before), horizon (1 << 62: none), 15 x (bundle start, farthest end up to its last group)}"""
    key, emax = np.asarray(key, np.int64), np.asarray(emax, np.int64)
    ng = len(key)
    _, hd, base, hit_limit = walk(key, emax, t)
    nh = len(hd)
    out = np.empty(CAND, np.int64)
    h1 = hd[0] if nh else ng
    out[0] = emax[h1 - 1] if h1 else -1
    if nh == BUNDLES + 1:
        out[1], last_known = key[hd[BUNDLES]], hd[BUNDLES]
    elif hit_limit:
        out[1], last_known = key[base], base
    else:
        out[1], last_known = INF, ng
    for b in range(BUNDLES):
        if b < nh:
            nexth = hd[b + 1] if b + 1 < nh else last_known
            out[2 + 2 * b], out[3 + 2 * b] = key[hd[b]], emax[nexth - 1]
        else:
            out[2 + 2 * b], out[3 + 2 * b] = INF, -1
    return out


def stage_cands(key, emax, allmeta, world):
    """tbk_partial_stage_cands of one rank: (targets [world - 1], cands [world - 1, CAND])"""
    tg = targets(allmeta, world)
    return tg, np.stack([cands(key, emax, int(t)) for t in tg]) if world > 1 else np.zeros((0, CAND), np.int64)


def judge(L, x):
    """one rank's list on a candidate: None = beyond what the list describes, else the farthest end of its groups before x"""
    if x > int(L[1]):
        return None
    e = int(L[0])
    for b in range(BUNDLES):
        if int(L[2 + 2 * b]) < x:
            e = int(L[3 + 2 * b])
    return e


def choose(allcands_of_cut, t):
    """allcands_of_cut [world][CAND]: every rank's list of ONE cut -> (cut, unsettled): the smallest of the target and the listed
    bundle starts that is at or behind the target, inside every horizon, and beyond every rank's reach (judge, on all candidates at
    once)"""
    L = np.asarray(allcands_of_cut, np.int64).reshape(-1, CAND)
    t = int(t)
    if t >= INF:
        return INF, False
    X = np.concatenate([[t], L[:, 2::2].reshape(-1)]).astype(np.int64)
    X = np.unique(X[(X < INF) & (X >= t)])
    clean = np.ones(len(X), bool)
    for row in L:
        before = row[2::2][None, :] < X[:, None]                                 # the listed bundles that start before the candidate
        last = BUNDLES - 1 - np.argmax(before[:, ::-1], axis=1)                  # the last of them says how far the rank reaches
        e = np.where(before.any(axis=1), row[3::2][last], row[0])
        clean &= (X <= row[1]) & (e < X)
    ok = np.flatnonzero(clean)
    return (int(X[ok[0]]), False) if len(ok) else (INF, True)


def cuts_sorted(cuts):
    """partial_cuts_sorted_k: from the back, an earlier cut that is larger than the next takes the next one's place"""
    c = [int(v) for v in cuts]
    for i in range(len(c) - 2, -1, -1):
        if c[i] > c[i + 1]:
            c[i] = c[i + 1]
    return np.array(c, np.int64)


def stage_choose(allcands, tg):
    """the cut part of tbk_partial_stage_pack: allcands [world][world - 1][CAND], targets [world - 1] -> (cuts, flag bit 1)"""
    A = np.asarray(allcands, np.int64)
    world = A.shape[0]
    A = A.reshape(world, world - 1, CAND)
    got = [choose(A[:, c, :], int(tg[c])) for c in range(world - 1)]
    return cuts_sorted([g[0] for g in got]), 2 if any(g[1] for g in got) else 0


def table(key, cuts, words_per_group):
    """tab[world][3] = {first group, rows, words} per destination d: the groups with cuts[d - 1] <= key < cuts[d]"""
    key = np.asarray(key, np.int64)
    w = np.concatenate([[0], np.cumsum(np.asarray(words_per_group, np.int64))])
    edge = np.concatenate([[0], np.searchsorted(key, np.asarray(cuts, np.int64), side="left"), [len(key)]]).astype(np.int64)
    return np.stack([edge[:-1], edge[1:] - edge[:-1], w[edge[1:]] - w[edge[:-1]]], axis=1)


def tabx(key, cuts, words_per_group, flags, n_files, first_fidx, carry):
    return np.concatenate([table(key, cuts, words_per_group).reshape(-1), np.array([flags, n_files, first_fidx, carry], np.int64)])


# ---- the definition, and the product's walk ---------------------------------------------------------------------------------------------
def exact_cut(ranks, t):
    """ranks: per rank (key [ng], endk [ng]) — start keys in order and each group's OWN keyed end (tid + 1) << 31 | end + 1.
    The smallest x >= t among t and every start of every rank such that every group of every rank with key < x has endk < x;
    1 << 62 when no such key exists."""
    t = int(t)
    if t >= INF:
        return INF
    X = np.unique(np.concatenate([[t]] + [np.asarray(k, np.int64)[np.asarray(k, np.int64) >= t] for k, _ in ranks]))
    reach = np.full(len(X), -1, np.int64)
    for k, e in ranks:
        k, e = np.asarray(k, np.int64), np.asarray(e, np.int64)
        if len(k) == 0:
            continue
        far = np.concatenate([[-1], np.maximum.accumulate(e)])      # far[n] = farthest keyed end among the first n groups
        reach = np.maximum(reach, far[np.searchsorted(k, X, side="left")])   # groups with key < x: the first searchsorted(x) ones
    ok = np.flatnonzero(reach < X)
    return int(X[ok[0]]) if len(ok) else INF


def rounds_cut(ranks, t):
    """the protocol's first form on the host (tiebrush_amd.dist._partials_rounds): ranks = per rank (key, emax); returns (cut, rounds)"""
    from tiebrush_amd import dist
    p = np.array([int(t)], np.int64)
    rounds = 0
    while True:
        rounds += 1
        m = np.array([-1], np.int64)
        for k, em in ranks:
            m = np.maximum(m, dist._probe_max_np(np.array([0, len(k)]), np.asarray(k, np.int64), np.asarray(em, np.int64), p))
        if int(m[0]) < int(p[0]) or int(p[0]) == dist.KEY_INF:
            return int(p[0]), rounds
        nxt = np.array([dist.KEY_INF], np.int64)
        for k, em in ranks:
            nxt = np.minimum(nxt, dist._probe_next_np(np.array([0, len(k)]), np.asarray(k, np.int64), m))
        p = nxt
