"""The device-wide primitives on their own (tests/support/prims_probe.hip -> libtbk_probe.so), at the sizes where each mechanism can go
wrong, against numpy on the host.  Every assertion is equality of integer arrays.

Not covered: a radix-sort tile of iter = 16 sub-tiles needs more than 125 M keys (iter = ceil(n / (2048 * 4096)), capped at 16); the
sizes here reach iter = 1, 2 and 3, which take the same loop."""
import numpy as np
import pytest
import torch

import prims_probe as pp
from tiebrush_amd import api

pytestmark = pytest.mark.gpu
U32, U64 = np.uint32, np.uint64
M32 = 0xFFFFFFFF
ALL = 2**64 - 1


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_profiling(True)       # (tbk_kernel_times then names what a probe call launched: the form that ran)
    yield c
    c.close()


def launches(ctx, name):
    return ctx.kernel_times().get(name, (0.0, 0))[1]


def same(t, ref):
    """device tensor == numpy array, compared where the tensor lives"""
    r = pp.dev(ref)
    return t.shape == r.shape and bool(torch.equal(t, r))


# ---- exclusive scans ----------------------------------------------------------------------------------------------------------
# SC_TILE = 2048; one block up to SC_SMALL = 16384, in chunks of 8192; tile sums folded inside the down-sweep up to SC_INLINE_NB = 4096
# tiles (8 388 608 elements), a spine kernel beyond, in rounds of 16 384 partials (33 554 432 elements)
EXSCAN_N = [0, 1, 2, 8191, 8192, 8193, 16383, 16384, 16385, 18431, 18432, 18433, 8388608, 8388609, 33554433]


@pytest.mark.parametrize("n", EXSCAN_N)
def test_exscan(ctx, n):
    rng = np.random.default_rng(1000 + n % 977)
    cases = [("u64 random", True, rng.integers(0, 2**32, n, dtype=U64).astype(U32)),
             ("u64 all ones", True, np.full(n, M32, U32)),                               # every carry crosses 32 bits
             ("u32 random", False, rng.integers(0, min(M32, M32 // max(n, 1)) + 1, n, dtype=U64).astype(U32))]   # total < 2^32: the callers' contract
    for what, u64, a in cases:
        inc = np.cumsum(a, dtype=U64)
        ref = np.zeros(n, U64)
        ref[1:] = inc[:-1]
        total = int(inc[-1]) if n else 0
        if not u64:
            assert total <= M32
            ref = ref.astype(U32)
        d_in = pp.dev(a)
        for with_total in (True, False):
            out, tot = pp.exscan(ctx, d_in, n, u64, with_total)
            assert same(out, ref), (what, with_total)
            if with_total:
                assert tot == total, what                                                # (n == 0: written as 0)
            if n > 16384:   # the form that ran: a spine launch only beyond SC_INLINE_NB tiles
                assert launches(ctx, "scan_spine") == (1 if -(-n // 2048) > 4096 else 0), ctx.kernel_times()


# ---- radix sorts --------------------------------------------------------------------------------------------------------------
# RX_SUB = 2048; a tile is iter = ceil(n / (2048 * 4096)) sub-tiles; rx_rowscan_k walks the tiles in rounds of 256
# 600 001: 293 tiles (second row-scan round); 8 388 609: iter = 2, a partial last tile and a sub-tile that starts past n; 16 777 217: iter = 3
RADIX_N = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 600001, 8388608, 8388609, 16777217]
RADIX_BIG = 8388608


def stable_order(*keys_major_first):
    """the stable order by the given keys (first = most significant)"""
    if len(keys_major_first) == 1:
        return np.argsort(keys_major_first[0], kind="stable")
    return np.lexsort(tuple(reversed(keys_major_first)))


def keys128(kind, n, rng):
    """-> hi, lo, and the stable order by (hi, lo)"""
    big = n >= RADIX_BIG
    c_hi, c_lo = U64(0x0123456789ABCDEF), U64(0x0FEDCBA987654321)
    if kind == "random":
        hi, lo = rng.integers(0, 2**64, n, dtype=U64), rng.integers(0, 2**64, n, dtype=U64)
        return hi, lo, stable_order(hi, lo)
    if kind == "equal":
        return np.full(n, c_hi), np.full(n, c_lo), np.arange(n)
    if kind == "few" and not big:
        pool_hi, pool_lo = rng.integers(0, 2**64, 5, dtype=U64), rng.integers(0, 2**64, 5, dtype=U64)
        pick = rng.integers(0, 5, n)
        hi, lo = pool_hi[pick], pool_lo[pick]
        return hi, lo, stable_order(hi, lo)
    if kind == "few":      # the large sizes: variation in two digits of one word, so that the reference is one sort of 16-bit keys
        small = rng.integers(0, 2**16, 5, dtype=np.uint16)[rng.integers(0, 5, n)]
        return np.full(n, c_hi), (c_lo & ~U64(0xFFFF0000)) | (small.astype(U64) << U64(16)), stable_order(small)
    small = rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "top_hi":
        return (c_hi & U64(0x00FFFFFFFFFFFFFF)) | (small.astype(U64) << U64(56)), np.full(n, c_lo), stable_order(small)
    assert kind == "bottom_lo"
    return np.full(n, c_hi), (c_lo & ~U64(0xFF)) | small.astype(U64), stable_order(small)


def check_radix128(ctx, hi, lo, order, only_hi=ALL, only_lo=ALL, exact=False):
    n = len(hi)
    d_hi0, d_lo0 = pp.dev(hi), pp.dev(lo)
    d_hi, d_lo, d_val = d_hi0.clone(), d_lo0.clone(), torch.arange(n, dtype=torch.int32, device="cuda:0")
    pp.radix128(ctx, d_hi, d_lo, d_val, n, only_hi, only_lo, exact)
    d_order = pp.dev(order.astype(np.int64))
    assert torch.equal(d_val.long(), d_order), "val = arange is the witness: equal keys keep their input order"
    assert torch.equal(d_hi, d_hi0[d_order]) and torch.equal(d_lo, d_lo0[d_order])


def radix_cases(kinds):
    """every size with every key set; fully random keys up to 600 001 (at the three largest sizes the keys vary in two digits at most)"""
    return [pytest.param(n, k, id="%d-%s" % (n, k)) for n in RADIX_N for k in kinds if not (k == "random" and n > 600001)]


@pytest.mark.parametrize("exact", [False, True], ids=["scan_bits", "exact"])
@pytest.mark.parametrize("n,kind", radix_cases(["random", "equal", "few", "top_hi", "bottom_lo"]))
def test_radix_sort128(ctx, n, kind, exact):
    rng = np.random.default_rng(n % 1009 + 7)
    hi, lo, order = keys128(kind, n, rng)
    check_radix128(ctx, hi, lo, order, exact=exact)


def keys_w64(kind, n, rng):
    """-> words, mask, the stable order by the masked bits.  Unless the whole word is the key, the bits outside the mask hold the index:
    a word is its own witness of stability"""
    idx = np.arange(n, dtype=U64)
    big = n >= RADIX_BIG
    if kind == "random":
        w = rng.integers(0, 2**64, n, dtype=U64)
        return w, ALL, stable_order(w)
    if kind == "equal":
        return (U64(0xABCD1234) << U64(32)) | idx, M32 << 32, np.arange(n)
    if kind == "few" and not big:
        k = rng.integers(0, 2**32, 5, dtype=U64)[rng.integers(0, 5, n)]
        return (k << U64(32)) | idx, M32 << 32, stable_order(k)
    if kind == "few":
        small = rng.integers(0, 2**16, 5, dtype=np.uint16)[rng.integers(0, 5, n)]
        return (U64(0x1234) << U64(48)) | (small.astype(U64) << U64(32)) | idx, M32 << 32, stable_order(small)
    small = rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "top":
        return (small.astype(U64) << U64(56)) | (U64(0x5A5A5A) << U64(32)) | idx, M32 << 32, stable_order(small)
    assert kind == "bottom"
    return (idx << U64(32)) | U64(0x00C0FF00) | small.astype(U64), M32, stable_order(small)


@pytest.mark.parametrize("exact", [False, True], ids=["scan_bits", "exact"])
@pytest.mark.parametrize("n,kind", radix_cases(["random", "equal", "few", "top", "bottom"]))
def test_radix_sort_w64(ctx, n, kind, exact):
    rng = np.random.default_rng(n % 1013 + 11)
    w, mask, order = keys_w64(kind, n, rng)
    d_w0 = pp.dev(w)
    d_w = d_w0.clone()
    pp.radix_w64(ctx, d_w, n, mask, exact)
    assert torch.equal(d_w, d_w0[pp.dev(order.astype(np.int64))])


# The contract of tbk_internal.h: the bits of only_hi / only_lo / mask take part in the ordering, "the rest are payload that must not
# reorder equal keys" — also the rest of a byte the mask ends in (collapse.hip's YD split and baix.hip's index sort pass such masks).
MASKS128 = [(0xFF00, 0), (0x00FF000000000000, 0x0000000000FF0000),                       # byte-aligned
            (0x0F00, 0), (((1 << 5) - 1) << 32, 0), (0, 0x3FF << 12), (0x7 << 30, 0x1 << 63)]   # ending inside a byte
MASK_N = [2049, 70001]


@pytest.mark.parametrize("exact", [False, True], ids=["scan_bits", "exact"])
@pytest.mark.parametrize("masks", MASKS128, ids=lambda m: "%x_%x" % m)
@pytest.mark.parametrize("n", MASK_N)
def test_radix_sort128_masked_payload_keeps_input_order(ctx, n, masks, exact):
    rng = np.random.default_rng(n + 3)
    hi, lo = rng.integers(0, 2**64, n, dtype=U64), rng.integers(0, 2**64, n, dtype=U64)    # random payload in every other bit
    order = stable_order(hi & U64(masks[0]), lo & U64(masks[1]))
    check_radix128(ctx, hi, lo, order, masks[0], masks[1], exact)


@pytest.mark.parametrize("exact", [False, True], ids=["scan_bits", "exact"])
@pytest.mark.parametrize("mask", [0xFF00, 0x00FF0000FF000000, 0x0F00, ((1 << 5) - 1) << 32, 0x3FF << 12, 0x3 << 31], ids=hex)
@pytest.mark.parametrize("n", MASK_N)
def test_radix_sort_w64_masked_payload_keeps_input_order(ctx, n, mask, exact):
    rng = np.random.default_rng(n + 5)
    w = rng.integers(0, 2**64, n, dtype=U64)
    d_w = pp.dev(w)
    calls, words = pp.radix_w64(ctx, d_w, n, mask, exact, emit=True)
    ref = w[stable_order(w & U64(mask))]
    assert same(d_w, ref)
    assert same(words, ref) and same(calls, np.r_[np.ones(n, U32), U32(0)])


@pytest.mark.parametrize("n", [1, 2, 2047, 2049, 600001])
@pytest.mark.parametrize("kind", ["few", "flat", "equal_exact"])
def test_radix_sort_w64_emit_once_per_word_with_its_final_position(ctx, n, kind):
    rng = np.random.default_rng(n)
    if kind == "few":
        w, mask, order = keys_w64("few", n, rng)
        exact = False
    else:   # no masked bit varies.  flat: the bit scan finds that, no pass runs, a flat kernel calls the functor (last < 0);
        w, mask, order = keys_w64("equal", n, rng)     # equal_exact: the passes run all the same, the last one calls it
        exact = kind == "equal_exact"
    d_w = pp.dev(w)
    calls, words = pp.radix_w64(ctx, d_w, n, mask, exact, emit=True)
    assert same(d_w, w[order])
    assert same(calls, np.r_[np.ones(n, U32), U32(0)]), "once per word, never outside the array"
    assert same(words, w[order]), "with the word's final position"
    if kind == "flat" or n == 1:
        kt = ctx.kernel_times()
        assert launches(ctx, "rx_hist") == 0 and launches(ctx, "rx_scatter") == 1, kt      # (the flat kernel runs under the scatter's name)


# ---- the run sort -------------------------------------------------------------------------------------------------------------
# MG_T = 2048 outputs per merge tile; a refine block owns RF_W = 1024 positions and a window of RF_CAP = 2048; longer buckets go to one block
# each (msort_big_k) up to MS_BIG_MAX = 2^17 records; a longer one that is also more than 1/64 of the tile raises TBK_DERR_BIGBUCKET
SENT_HI, SENT_LO, SENT_VAL = 0x7EADBEEF7EADBEEF, 0x7AFEF00D7AFEF00D, 0x7BADCAFE
PAD = 3000


def make_runs(rng, buckets, nruns, empty=(), lo_pool=16):
    """buckets: sizes of the (tid, start) buckets in position order.  The records of every bucket are spread over the runs that may hold any;
    a run is non-decreasing in hi >> 2 and otherwise in any order.  lo < 2^62 (span < 2^30), strand code <= 2; half of the records draw lo
    from a small pool so that whole keys repeat.  -> hi, lo, run_off"""
    sizes = np.asarray(buckets, np.int64)
    n = int(sizes.sum())
    P = np.repeat(np.arange(len(sizes), dtype=U64) * U64(3) + U64(5), sizes)
    live = np.array([r for r in range(nruns) if r not in empty])
    run = live[rng.integers(0, len(live), n)]
    strand = rng.integers(0, 3, n, dtype=U64)
    pool = rng.integers(0, 2**62, lo_pool, dtype=U64)
    lo = np.where(rng.integers(0, 2, n) == 0, pool[rng.integers(0, lo_pool, n)], rng.integers(0, 2**62, n, dtype=U64))
    perm = rng.permutation(n)
    perm = perm[np.lexsort((P[perm], run[perm]))]        # by (run, position), the rest shuffled
    run_off = np.zeros(nruns + 1, U32)
    run_off[1:] = np.cumsum(np.bincount(run, minlength=nruns))
    return ((P << U64(2)) | strand)[perm], lo[perm], run_off


def ordinary(rng, total):
    """buckets of 1 .. 6 records adding up to `total`"""
    out = []
    while total > 0:
        out.append(int(min(total, rng.integers(1, 7))))
        total -= out[-1]
    return out


def run_sort(ctx, hi, lo, run_off, nruns):
    """-> error bits, result side and other side as device tensors of n + PAD elements"""
    n = len(hi)
    def side(h, l, v):
        return (pp.dev(np.r_[h, np.full(PAD, SENT_HI, U64)]), pp.dev(np.r_[l, np.full(PAD, SENT_LO, U64)]), pp.dev(np.r_[v, np.full(PAD, SENT_VAL, U32)]))
    a = side(hi, lo, np.arange(n, dtype=U32))
    b = side(np.full(n, SENT_HI, U64), np.full(n, SENT_LO, U64), np.full(n, SENT_VAL, U32))
    return pp.sort_runs(ctx, a, b, n + PAD, pp.dev(run_off), nruns)


def check_sort_runs(ctx, hi, lo, run_off, nruns, order=None):
    n = len(hi)
    assert int(run_off[nruns]) == n
    if order is None:
        order = stable_order(hi, lo)       # "exactly as tbk_radix_sort128 would"
    bits, res, other = run_sort(ctx, hi, lo, run_off, nruns)
    assert bits == 0
    d_order = pp.dev(order.astype(np.int64))
    assert torch.equal(res[2][:n].long(), d_order)
    assert torch.equal(res[0][:n], pp.dev(hi)[d_order]) and torch.equal(res[1][:n], pp.dev(lo)[d_order])
    for s in (res, other):       # nothing beyond the true count is written (the grids are sized by the host's upper bound)
        assert bool((s[0][n:] == SENT_HI).all()) and bool((s[1][n:] == SENT_LO).all()) and bool((s[2][n:] == SENT_VAL).all())


@pytest.mark.parametrize("nruns,empty", [(1, ()), (2, ()), (2, (0,)), (3, ()), (3, (1,)), (5, ()), (5, (0,)), (5, (2,)), (5, (4,)), (64, ()),
                                         (64, (0, 31, 63))])
def test_sort_runs_run_counts_and_empty_runs(ctx, nruns, empty):
    rng = np.random.default_rng(nruns * 10 + len(empty))
    hi, lo, run_off = make_runs(rng, ordinary(rng, 9001), nruns, empty)
    check_sort_runs(ctx, hi, lo, run_off, nruns)


@pytest.mark.parametrize("nruns", [1, 3])
@pytest.mark.parametrize("bucket", [1023, 1024, 1025, 2047, 2048, 2049])
def test_sort_runs_bucket_at_the_refine_window_sizes(ctx, bucket, nruns):
    rng = np.random.default_rng(bucket + nruns)
    hi, lo, run_off = make_runs(rng, ordinary(rng, 700) + [bucket] + ordinary(rng, 3100), nruns)
    check_sort_runs(ctx, hi, lo, run_off, nruns)


@pytest.mark.parametrize("before,bucket", [(600, 1500), (1000, 1047), (1000, 1048), (1000, 1049), (1023, 1025), (0, 2048), (1024, 2048), (2047, 3)])
def test_sort_runs_bucket_across_a_window_boundary(ctx, before, bucket):
    """a bucket that starts `before` records into the tile: across the RF_W boundary at 1024 and inside / up to / just past the RF_CAP window"""
    rng = np.random.default_rng(before * 7 + bucket)
    hi, lo, run_off = make_runs(rng, ordinary(rng, before) + [bucket] + ordinary(rng, 2500), 3)
    check_sort_runs(ctx, hi, lo, run_off, 3)


def test_sort_runs_bucket_of_2_17_stays_in_the_block_sort(ctx):
    rng = np.random.default_rng(17)
    hi, lo, run_off = make_runs(rng, ordinary(rng, 1500) + [1 << 17] + ordinary(rng, 2500), 3)
    check_sort_runs(ctx, hi, lo, run_off, 3)


def test_sort_runs_bucket_beyond_2_17_in_a_small_tile_falls_back(ctx):
    """more than MS_BIG_MAX records and more than 1/64 of the tile: TBK_DERR_BIGBUCKET, and the other side of the buffers (what the caller gets by
    swapping back) is still a valid input of the radix sort, which then gives the order"""
    rng = np.random.default_rng(18)
    hi, lo, run_off = make_runs(rng, ordinary(rng, 1500) + [(1 << 17) + 1] + ordinary(rng, 2500), 3)
    n = len(hi)
    bits, res, other = run_sort(ctx, hi, lo, run_off, 3)
    assert bits == pp.DERR_BIGBUCKET
    pp.radix128(ctx, other[0], other[1], other[2], n)
    d_order = pp.dev(stable_order(hi, lo).astype(np.int64))
    assert torch.equal(other[2][:n].long(), d_order)
    assert torch.equal(other[0][:n], pp.dev(hi)[d_order]) and torch.equal(other[1][:n], pp.dev(lo)[d_order])
    assert bool((other[0][n:] == SENT_HI).all()) and bool((other[2][n:] == SENT_VAL).all())


def test_sort_runs_bucket_beyond_2_17_in_a_large_tile_is_sorted(ctx):
    """the same bucket is no longer more than 1/64 of a tile of 64 * (2^17 + 1) records and a few: sorted here, no flag.  The filler is 200
    buckets with keys from a small set, so that the whole order is that of one 16-bit number"""
    rng = np.random.default_rng(19)
    deep, nb, nruns = (1 << 17) + 1, 201, 2
    n = 64 * deep + 13
    fill = np.full(nb, (n - deep) // (nb - 1), np.int64)
    fill[100] = deep
    fill[-1] += n - int(fill.sum())
    assert deep * 64 <= n and np.all(np.delete(fill, 100) <= 1 << 17)
    b = np.repeat(np.arange(nb, dtype=np.uint16), fill)
    strand = rng.integers(0, 3, n, dtype=np.uint16)
    lo_i = rng.integers(0, 16, n, dtype=np.uint16)
    run = rng.integers(0, nruns, n, dtype=np.uint8)
    perm = np.argsort(run, kind="stable")                # a run: by position (b is in order already), input order otherwise
    b, strand, lo_i, run = b[perm], strand[perm], lo_i[perm], run[perm]
    hi = ((b.astype(U64) * U64(3) + U64(5)) << U64(2)) | strand.astype(U64)
    lo = (lo_i.astype(U64) << U64(36)) | U64(0x123)
    run_off = np.zeros(nruns + 1, U32)
    run_off[1:] = np.cumsum(np.bincount(run, minlength=nruns))
    check_sort_runs(ctx, hi, lo, run_off, nruns, order=stable_order((b * np.uint16(3) + strand) * np.uint16(16) + lo_i))


# ---- the scan engine ----------------------------------------------------------------------------------------------------------
# SO_TILE = 2048; the look-back reads its predecessors in windows of 64 tiles; the three-launch form folds the tile totals inside the
# down-sweep up to SO_INLINE_NB = 2048 tiles (4 194 304 elements) and runs a spine kernel beyond, in rounds of 256 partials
SCAN_N = [1, 63, 64, 65, 2047, 2048, 2049, 4096, 131071, 131072, 131073, 133121, 264197, 4194304, 4194305, 4196359]
HEADS = ["none", "first", "tile_last", "tile_first", "every_64_tiles", "third", "sparse"]
FORMS = {0: "default", 1: "lookback", 2: "3pass"}
TILES_OF_NOTE = [0, 1, 2, 63, 64, 65, 128, 129, 2047, 2048, 2049]


def head_flags(kind, n, rng, tile=2048):
    f = np.zeros(n, U32)
    if kind == "first":
        f[0] = 1
    elif kind == "tile_last":
        idx = np.array([t * tile + tile - 1 for t in TILES_OF_NOTE])
        f[idx[idx < n]] = 1
    elif kind == "tile_first":
        idx = np.array([t * tile for t in TILES_OF_NOTE[1:]])
        f[idx[idx < n]] = 1
    elif kind == "every_64_tiles":
        f[::64 * tile] = 1
    elif kind == "third":
        f[rng.integers(0, 3, n) == 0] = 1
    elif kind == "sparse":
        f[rng.integers(0, 5000, n) == 0] = 1
    else:
        assert kind == "none"       # one carry crosses every tile
    return f


def seg_scan_ref(flag, value):
    """flag [n], value [K, n] -> inclusive, exclusive as [1 + K, n] (row 0: a head at or before / before the element; row k + 1: the sum of
    value[k] since the last head, mod 2^32).  The sum since the last head is cumsum minus cumsum just before that head."""
    n = len(flag)
    idx = np.arange(n, dtype=np.int64)
    last = np.maximum.accumulate(np.where(flag != 0, idx, -1))
    inc = np.empty((1 + len(value), n), U32)
    inc[0] = last >= 0
    for k, v in enumerate(value):
        c = np.cumsum(v, dtype=U64)
        before_head = c[np.maximum(last, 0)] - v[np.maximum(last, 0)]
        inc[k + 1] = ((c - np.where(last >= 0, before_head, U64(0))) & U64(M32)).astype(U32)
    exc = np.zeros_like(inc)         # exclusive of element 0: the identity
    exc[:, 1:] = inc[:, :-1]
    return inc, exc


def scan_case(n, heads, tile=2048):
    rng = np.random.default_rng(n % 1021 + 31 * HEADS.index(heads))
    flag = head_flags(heads, n, rng, tile)
    value = rng.integers(0, 2**32, (4, n), dtype=U64).astype(U32)
    return flag, value


def check_scan(ctx, flag, value, forms, **delay):
    n = len(flag)
    inc, exc = seg_scan_ref(flag, value)
    d_flag, d_value = pp.dev(flag), pp.dev(value)
    nb = -(-n // 2048)
    d_elem, d_inc, d_exc = pp.dev(np.vstack([(flag != 0).astype(U32)[None], value])), pp.dev(inc), pp.dev(exc)
    for words in (2, 5):
        for form in forms:
            what = (words, FORMS[form])
            (elem, g_inc, g_exc), err = pp.scan(ctx, d_flag, d_value, n, words, form, **delay)
            assert err == 0, what         # (TBK_DERR_INTERNAL: a look-back gave up)
            assert torch.equal(elem, d_elem[:words]), what
            assert not bool(g_exc[:, 0].any()), what
            assert torch.equal(g_inc, d_inc[:words]), what
            assert torch.equal(g_exc, d_exc[:words]), what
            # the form that ran: one launch for a look-back over more than one tile; reduce + down-sweep, and a spine beyond SO_INLINE_NB
            want = 1 if (form == 1 and nb > 1) else (2 if nb <= 2048 else 3)
            assert launches(ctx, "probe_scan") == want, (what, ctx.kernel_times())


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_engine(ctx, n, heads):
    flag, value = scan_case(n, heads)
    check_scan(ctx, flag, value, (0, 1, 2))


@pytest.mark.parametrize("heads", ["none", "sparse"])
@pytest.mark.parametrize("delay_tile", [0, 70])
def test_scan_lookback_walks_more_than_one_window(ctx, delay_tile, heads):
    """The lane that loads the first element of one tile waits 2 ms (a bounded wait, a ten-thousandth of the look-back's own bound).  Until
    that tile has published, no later tile can publish an inclusive prefix, so every later tile finds only aggregates and walks window after
    window of 64 predecessors down to it: 300 tiles, up to four windows"""
    n = 300 * 2048 + 11
    flag, value = scan_case(n, heads)
    check_scan(ctx, flag, value, (1,), delay_index=delay_tile * 2048, delay_ticks=200000)


@pytest.mark.parametrize("heads", ["none", "third", "sparse"])
@pytest.mark.parametrize("n", [1] + [256 * 4 * m + d for m in (1, 64, 65, 129) for d in (-1, 0, 1)])
def test_scan_two_e4(ctx, n, heads):
    check_scan_two(ctx, n, heads, 4)


@pytest.mark.parametrize("heads", ["none", "third", "sparse"])
@pytest.mark.parametrize("n", [1] + [256 * 8 * m + d for m in (1, 64, 65, 129) for d in (-1, 0, 1)])
def test_scan_two_e8(ctx, n, heads):
    check_scan_two(ctx, n, heads, 8)


def check_scan_two(ctx, n, heads, E):
    flag, value = scan_case(n, heads, 256 * E)
    inc, exc = seg_scan_ref(flag, value[:2])
    term = (((exc[1].astype(U64) + np.arange(n, dtype=U64)) & U64(M32)) % U64(3) == 0).astype(U32)    # from the first scan's exclusive prefix
    before = np.zeros(n, U32)
    before[1:] = np.cumsum(term, dtype=U64)[:-1].astype(U32)
    g_inc, g_exc, g_term, g_before, err = pp.scan_two(ctx, pp.dev(flag), pp.dev(value), n, E)
    assert err == 0
    assert same(g_inc, inc) and same(g_exc, exc)
    assert same(g_term, term) and same(g_before, before)
    assert launches(ctx, "probe_scan_two") == 1
