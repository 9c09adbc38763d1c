"""Hand-built payloads for the parse of the device deflate (bgz_deflate_k, tiebrush_amd/csrc/bgzdef.hip): every scene puts ONE edge of
the three-stage parse where it can be seen in the tokens, and says what it is there for as a predicate over the tokens of the member
(deflate_tokens.decode of its deflate bytes).  The kernel's units: rounds of 512 positions (the inserting, matching and parsing waves
run a round apart), batches of 64 (the parsing wave holds 64 positions in registers), two tables of 1 << 10 entries that remember the
latest position of a 4-byte and of an 8-byte key, candidates compared over 16 bytes, a match of 16 measured in full (256 bytes a
step) when the walk takes it, the lazy look that stops at the round's edge.

tests/test_deflate_scenes_cpu.py proves every predicate on the exact host model (tests/support/deflate_model.cpp, `tokens` mode);
tests/test_gpu_deflate_edges.py holds the device's own tokens to the same predicates and its bytes to the model's.

Payloads are random bytes (no two positions share four bytes by accident) with planted copies, or zeros with random islands where a
distance must be long: zeros keep to one entry of each table, so an island's entries survive 32 KiB of them.  A planted copy is found
only while no later position has taken its table entries: a scene takes a seed, SEEDS records for every scene the first seed (from 0)
at which the model proves the predicate — `python tests/test_deflate_scenes_cpu.py` repeats that search and prints the table.

Left out, and why:
  * "both candidates give 16, the 4-byte one is kept": not reachable.  A candidate that agrees over 8 bytes has the position's 8-byte
    key AND its 4-byte key; the latest such position is then the entry of both tables, and the two candidates are the same position
    (counted once).  Two different candidates can only tie below 8 bytes, where the 8-byte table's entry is a collision of the hash:
    `tie_keeps_4` builds that (both agree over 5 bytes; the host model's older parse preferred the 8-byte one).
  * "all 29 length symbols": the parse never writes a length of 3 (its keys are four bytes); `all_symbols` uses the other 28.
  * n = 1 with a dynamic header: at n = 1 the dynamic block's bits pass 8 n + 32 and the member is stored (`one_byte_1` says so); the
    distance code's forced second symbol is shown by `one_byte_64` (a literal and one match), a distance code of two forced symbols
    by the dynamic member of `stored_dynamic_switch`, which has no match.
"""
import functools
import heapq
from collections import namedtuple

import numpy as np

ROUND, BATCH, GOOD, MAXPAY = 512, 64, 16, 0xff00

# check(members): members = [View] in the order of the cuts.  relies: {position of the first member: {"k4": the 4-byte table's
# candidate, "l4": its compared length, "k8", "l8": the 8-byte table's}} — what the scene needs the tables to hold where the tokens alone
# would not show it (NONE: no candidate); test_deflate_scenes_cpu.py asserts it on the model, and the seed search runs on it
Scene = namedtuple("Scene", "name payload cuts check relies")
NONE = 0xFFFF
View = namedtuple("View", "btype hlit hdist hclen lit_lens dist_lens cl_lens tokens at n")


def view(decoded):
    """deflate_tokens.Decoded of a member the encoder wrote (one block) -> View; at = {payload offset: token}"""
    import deflate_tokens
    assert len(decoded.blocks) == 1 and decoded.blocks[0].final
    b = decoded.blocks[0]
    return View(b.btype, b.hlit, b.hdist, b.hclen, b.lit_lens, b.dist_lens, b.cl_lens, b.tokens, dict(deflate_tokens.positions(b.tokens)), len(decoded.payload))


# the seed of every scene whose planted copies depend on the tables' entries surviving (0 where nothing does)
SEEDS = {'fibonacci_distances': 1, 'longer_8_beats_nearer_4': 4, 'tie_keeps_4': 1}

# The code-length code at its 7-bit limit: test_deflate_scenes_cpu.py's search (`--cl-limit`) ran CL_LIMIT_SEARCH[0] payloads of three
# families through the model and took the first member whose code-length code has a length of 7 where an unlimited Huffman code over
# the header's symbols would be deeper: (family, index) — the scene `cl_limit` rebuilds that payload.
CL_LIMIT_SEARCH = (3999, ("random_alpha", 123))

_SCENES = {}


def scene(fn=None, **kw):
    def reg(f):
        name = f.__name__ + "".join("_%s" % v for v in kw.values())
        _SCENES[name] = functools.partial(f, **kw)
        return f
    return reg(fn) if fn else reg


def names():
    return sorted(_SCENES)


@functools.lru_cache(maxsize=None)
def build(name, seed=None):
    seed = SEEDS.get(name, 0) if seed is None else seed
    payload, cuts, check, *relies = _SCENES[name](seed)
    payload = bytes(payload)
    cuts = [0, len(payload)] if cuts is None else list(cuts)
    assert cuts[0] == 0 and cuts[-1] == len(payload) and all(0 < b - a <= MAXPAY for a, b in zip(cuts[:-1], cuts[1:]))
    return Scene(name, payload, cuts, check, relies[0] if relies else {})


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def rnd(n, seed, alpha=None):
    """n bytes out of `alpha` values (default: 64, and 32 in a short payload): few enough for a dynamic block to beat a stored one — a
    stored member shows no tokens —, enough for four bytes not to repeat by accident"""
    alpha = (32 if n <= 400 else 64) if alpha is None else alpha
    return (np.random.default_rng([seed, n]).integers(0, alpha, n, dtype=np.uint8) * (256 // alpha) + 1).astype(np.uint8)


def zeros(n):
    return np.zeros(n, dtype=np.uint8)


def plant(a, src, dst, length, fence_after=True):
    """a[dst, dst + length) becomes a copy of a[src, src + length) (byte by byte: src + length > dst gives a periodic run), the bytes
    before and behind it made to differ from the source's so that the copy is exactly this long"""
    assert 0 <= src < dst and dst + length <= len(a)
    if src > 0 and src + length < dst:
        a[dst - 1] = a[src - 1] ^ 0xA5
    for i in range(length):
        a[dst + i] = a[src + i]
    if src > 0 and src + length >= dst:                   # (a periodic run: the byte before the copy is the run's own)
        a[src - 1] = a[dst - 1] ^ 0xA5
    if dst + length < len(a) and fence_after:
        a[dst + length] = a[src + length] ^ 0x5A


def island(a, pos, data, before=1, after=None):
    """random bytes in a field of zeros, a byte that is not zero before them (so that no match runs into the island from the zeros)"""
    a[pos - 1] = before
    a[pos:pos + len(data)] = data
    if after is not None:
        a[pos + len(data)] = after


def one(check):
    return lambda ms: check(ms[0])


def has(m, start, length, dist):
    assert m.btype == 2, "stored: no tokens to see"
    assert m.at.get(start) == (length, dist), (start, (length, dist), m.at.get(start), sorted(p for p in m.at if abs(p - start) < 20))


def is_literal(m, pos):
    assert m.btype == 2 and isinstance(m.at.get(pos), int), (pos, m.at.get(pos))


def copy_scene(n, src, dst, length, seed, want=None):
    a = rnd(n, seed)
    plant(a, src, dst, length)
    want = [(dst, min(length, 258), dst - src)] if want is None else want
    return a, None, one(lambda m: [has(m, *w) for w in want])


def unlimited_depth(freqs):
    """depth of the deepest leaf of a plain Huffman tree over the non-zero frequencies"""
    h = [(f, 0) for f in freqs if f]
    heapq.heapify(h)
    while len(h) > 1:
        (f1, d1), (f2, d2) = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (f1 + f2, max(d1, d2) + 1))
    return h[0][1]


def token_freqs(tokens):
    import deflate_tokens as dt
    lit, dist = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[257 + max(c for c in range(29) if dt.LEN_BASE[c] <= t[0] and (c == 28 or t[0] < 258))] += 1
            dist[max(c for c in range(30) if dt.DIST_BASE[c] <= t[1])] += 1
    lit[256] += 1
    return lit, dist


# ---- round and batch seams: a 40-byte copy that starts d positions before a seam ---------------------------------------------------

SEAM_D = (0, 1, 3, 4, 15, 16, 17, 39, 40)

for _k in (1, 2):
    for _d in SEAM_D:
        @scene(k=_k, d=_d)
        def round_seam(seed, k, d):
            dst = ROUND * k - d
            return copy_scene(ROUND * k + 120, dst - 70, dst, 40, seed)

for _j in (3, 11):                    # a batch seam inside round 0 and one inside round 1
    for _d in SEAM_D:
        @scene(j=_j, d=_d)
        def batch_seam(seed, j, d):
            dst = BATCH * j - d
            return copy_scene(BATCH * j + 120, dst - 70, dst, 40, seed)


@scene
def tail_covers_batches(seed):
    """a 200-byte match from lane 10 of batch 10: its tail covers batches 11 and 12 whole (carry >= cnt) and ends inside batch 13"""
    dst = BATCH * 10 + 10
    a = rnd(1100, seed)
    plant(a, 300, dst, 200)
    return a, None, one(lambda m: (has(m, dst, 200, dst - 300), is_literal(m, dst + 200)))


@scene
def tail_into_next_round(seed):
    """a match that covers the rest of round 1 and the first 10 positions of round 2: the carry crosses the round"""
    dst, length = 2 * ROUND - 100, 110
    a = rnd(1200, seed)
    plant(a, 700, dst, length)
    return a, None, one(lambda m: (has(m, dst, length, dst - 700), is_literal(m, 2 * ROUND + 10)))


@scene
def match_258_at_511(seed):
    """the last position of round 0 starts a match of 258: the measurement reads through round 1 (the parse is at round 0 then)"""
    return copy_scene(900, 100, 511, 258, seed)


@scene
def copy_300(seed):
    return copy_scene(900, 50, 400, 300, seed, want=[(400, 258, 350), (658, 42, 350)])


# ---- the lazy rule ------------------------------------------------------------------------------------------------------------------

def lazy_payload(n, p, seed, lens):
    """at p, p + 1, ... the matches of lens[0] < lens[1] < ... bytes begin, each from a source of its own (the later the nearer, so
    that the 4-byte table's entry — the latest — is the right one at every step).  -> (payload, the sources)"""
    a = rnd(n, seed)
    k = len(lens)
    x = rnd(k + lens[-1], seed + 1000)
    srcs = [p - 60 * (k - i) for i in range(k)]
    a[p:p + len(x)] = x
    a[p + len(x)] = 0xEE
    a[p - 1] = 0x77
    for i, (s, l) in enumerate(zip(srcs, lens)):
        a[s - 1] = x[i - 1] ^ 0xFF if i else 0x78
        a[s:s + l] = x[i:i + l]
        a[s + l] = (x[i + l] ^ 0xFF) if i + l < len(x) else 0x11
    return a, srcs


def rising(p, srcs, lens):
    """what a lazy scene relies on: at p + i the 4-byte table holds source i, which agrees over lens[i] bytes (16 at most are compared)"""
    return {p + i: {"k4": s, "l4": min(l, GOOD)} for i, (s, l) in enumerate(zip(srcs, lens))}


for _where in ("inside", "lane63"):
    @scene(where=_where)
    def lazy_5_then_8(seed, where):
        p = {"inside": ROUND + 20, "lane63": BATCH * 9 + 63}[where]
        a, (s1, s2) = lazy_payload(p + 200, p, seed, (5, 8))
        return a, None, one(lambda m: (is_literal(m, p), has(m, p + 1, 8, p + 1 - s2))), rising(p, (s1, s2), (5, 8))


@scene
def lazy_blind_at_round_end(seed):
    """p is the last position of round 1: the look at p + 1 sees nothing, the 5 is taken although an 8 begins behind it"""
    p = 2 * ROUND - 1
    a, (s1, s2) = lazy_payload(p + 200, p, seed, (5, 8))
    return a, None, one(lambda m: has(m, p, 5, p - s1)), rising(p, (s1, s2), (5, 8))


@scene
def lazy_chain_of_three(seed):
    p = ROUND + 100
    a, (s1, s2, s3) = lazy_payload(p + 200, p, seed, (5, 7, 9))
    return a, None, one(lambda m: (is_literal(m, p), is_literal(m, p + 1), has(m, p + 2, 9, p + 2 - s3))), rising(p, (s1, s2, s3), (5, 7, 9))


@scene
def no_lazy_from_16(seed):
    """a compared length of 16 (true length 20) is taken although 30 bytes begin at the next position.  This scene cannot tell
    whether the walk asks `L < DF_GOOD`: compared lengths stop at 16, so the next position never compares longer than a 16 and the
    condition is redundant in the kernel and in the model alike.  It shows that the measured 20 is written and the 30 is not waited for"""
    p = ROUND + 100
    a, (s1, s2) = lazy_payload(p + 200, p, seed, (20, 30))
    return a, None, one(lambda m: has(m, p, 20, p - s1)), rising(p, (s1, s2), (20, 30))


# ---- long matches: the first mismatch in every byte of a dword, in the first, the second and the last lane's dword ---------------------

for _t in sorted({16, 17, 19, 20, 271, 272, 273} | {16 + 4 * f + b for f in (0, 1, 63) for b in range(4)}):
    @scene(t=_t)
    def true_length(seed, t):
        return copy_scene(1100, 100, 601, t, seed)


# ---- the end of the member ------------------------------------------------------------------------------------------------------------

for _n in (20, 512, 513):
    @scene(n=_n)
    def ends_on_last_byte(seed, n):
        length = 8 if n == 20 else 40
        a = rnd(n, seed, 2) if n == 20 else rnd(n, seed)          # (20 bytes: only two values keep the block dynamic)
        src = 0 if n == 20 else n - 140
        plant(a, src, n - length, length)
        return a, None, one(lambda m: (has(m, n - length, length, n - length - src), ))


def end_island_scene(seed, length, n=MAXPAY):
    """zeros, an island of `length` random bytes with ZEROS behind it, and its copy as the member's last bytes: behind the copy the
    measurement reads the zero padding (and, from n - 16 - 256 on, LDS behind the payload's area): only min(..., n - p) ends it"""
    a = zeros(n)
    x = rnd(length, seed, 256) | 1                                  # (no zero byte: nothing of the island continues a run of zeros)
    src = n - 30000
    island(a, src, x, before=1)
    island(a, n - length, x, before=2)
    return a, None, one(lambda m: (has(m, n - length, length, n - length - src), is_literal(m, n - length - 1)))


@scene
def ends_on_last_byte_ff00(seed):
    return end_island_scene(seed, 40)


for _l in (258, 257, 17, 16, 5, 4):
    @scene(l=_l)
    def starts_near_the_end(seed, l):
        return end_island_scene(seed, l)


for _t in (3, 4, 5, 6, 7):
    @scene(t=_t)
    def last_bytes_repeat(seed, t):
        """the last t bytes repeat earlier ones: the last seven positions have no 8-byte key, the last three no key"""
        n = 300
        a = rnd(n, seed)
        plant(a, 100, n - t, t)

        def check(m):
            if t == 3:
                [is_literal(m, n - i) for i in (1, 2, 3)]
            else:
                has(m, n - t, t, n - t - 100)
        return a, None, one(check)


# ---- distances ------------------------------------------------------------------------------------------------------------------------

for _d in (1, 2, 3, 4, 16):
    @scene(d=_d)
    def near_distance(seed, d):
        a = rnd(400, seed)
        plant(a, 200, 200 + d, 64)
        return a, None, one(lambda m: has(m, 200 + d, 64, d))


for _d in (32767, 32768, 32769):
    @scene(d=_d)
    def far_distance(seed, d):
        a = zeros(100 + d + 64 + 50)
        x = rnd(64, seed, 256) | 1
        island(a, 100, x, before=1, after=3)
        island(a, 100 + d, x, before=2, after=4)

        def check(m):
            assert all(isinstance(t, int) or t[1] <= 32768 for t in m.tokens)
            if d <= 32768:
                has(m, 100 + d, 64, d)
            else:
                is_literal(m, 100 + d)                           # the source is out of reach; nothing else begins with these bytes
        return a, None, one(check)


for _r in (3, 4, 5, 257, 258, 259, 600):
    @scene(r=_r)
    def run_at_distance_1(seed, r):
        """r + 1 equal bytes: a literal and an overlapping copy of r from distance 1 (r = 3: four equal bytes are ONE key, no match)"""
        a = rnd(100 + r + 1 + 100, seed)
        a[100:101 + r] = 0x41
        a[99], a[101 + r] = 0x40, 0x42

        def check(m):
            is_literal(m, 100)
            if r == 3:
                [is_literal(m, 100 + i) for i in (1, 2, 3)]
                return
            p, left = 101, r
            while left >= 4:
                has(m, p, min(left, 258), 1)
                p, left = p + min(left, 258), left - min(left, 258)
            [is_literal(m, p + i) for i in range(left)]
        return a, None, one(check)


# ---- which candidate ------------------------------------------------------------------------------------------------------------------

def h8(b):
    w0, w1 = int.from_bytes(bytes(b[0:4]), "little"), int.from_bytes(bytes(b[4:8]), "little")
    return ((w0 * 0x9E3779B1 + w1 * 0x85EBCA77) & 0xFFFFFFFF) >> 22


@scene
def both_tables_one_position(seed):
    """the 12 bytes occur once before: both tables hand back that position, it is one candidate"""
    return copy_scene(700, 300, 600, 12, seed) + ({600: {"k4": 300, "l4": 12, "k8": NONE}}, )


@scene
def longer_8_beats_nearer_4(seed):
    """the nearer position agrees over 5 bytes (the 4-byte table's entry), the farther over 12 (the 8-byte table's): the farther wins"""
    p = 600
    a = rnd(800, seed)
    x = rnd(12, seed + 1000)
    far, near = 300, 450
    for s, l in ((far, 12), (near, 5)):
        a[s - 1] = 0x30 + l
        a[s:s + l] = x[:l]
        a[s + l] = x[l] ^ 0xFF if l < 12 else 0x11
    a[p - 1], a[p + 12] = 0x77, 0xEE
    a[p:p + 12] = x
    return a, None, one(lambda m: has(m, p, 12, p - far)), {p: {"k4": near, "l4": 5, "k8": far, "l8": 12}}


@scene
def tie_keeps_4(seed):
    """two different candidates that both agree over 5 bytes: the 8-byte table's entry is a position whose 8 bytes only hash like the
    position's (three bytes searched for that).  `l > best`: the 4-byte table's — the nearer one — stays"""
    p = 600
    a = rnd(800, seed)
    x = rnd(8, seed + 1000)
    far, near = 300, 450
    want = h8(x)
    z = next(z for z in range(1 << 24) if (z & 0xFF) != x[5] and h8(bytes(x[:5]) + z.to_bytes(3, "little")) == want)
    w = next(w for w in range(1 << 24) if (w & 0xFF) != x[5] and h8(bytes(x[:5]) + w.to_bytes(3, "little")) != want)
    for s, tail in ((far, z), (near, w)):
        a[s - 1] = 0x30 + (s & 7)
        a[s:s + 5] = x[:5]
        a[s + 5:s + 8] = np.frombuffer(tail.to_bytes(3, "little"), dtype=np.uint8)
    a[p - 1] = 0x77
    a[p:p + 8] = x
    return a, None, one(lambda m: has(m, p, 5, p - near)), {p: {"k4": near, "l4": 5, "k8": far, "l8": 5}}


for _period in (1, 2, 4):
    @scene(period=_period)
    def one_hash_for_64_lanes(seed, period):
        """2000 bytes of period 1, 2, 4: every lane of an inserting instruction meets the entry its neighbour wrote.  The first
        `period` bytes are literals, then matches of 258 from distance `period` to the end"""
        n = 2000
        a = np.resize(np.frombuffer(b"\x41\x42\x43\x44"[:period], dtype=np.uint8), n).copy()

        def check(m):
            want = [int(b) for b in a[:period]]
            left = n - period
            while left:
                want.append((min(left, 258), period))
                left -= min(left, 258)
            assert m.btype == 2 and m.tokens == want, m.tokens
        return a, None, one(check)


# ---- codes and header -----------------------------------------------------------------------------------------------------------------

@scene
def one_byte_1(seed):
    """n = 1: 17 header bits, the code-length code and the lengths pass 8 + 32 bits: a stored block"""
    return b"x", None, one(lambda m: (_eq(m.btype, 0), _eq(m.tokens, [0x78])))


@scene
def one_byte_64(seed):
    """64 equal bytes: a literal and one match — the distance code has one symbol and gets its forced second: the field HDIST is 1, two
    lengths of one bit are sent; the literal / length code has the byte, the end of the block and one length"""
    def check(m):
        assert m.btype == 2 and m.tokens == [0x78, (63, 1)]
        assert m.hdist == 2 and m.dist_lens == [1, 1]
        assert sorted(s for s, l in enumerate(m.lit_lens) if l) == [0x78, 256, 257 + 19]     # (63 = 59 + 4: the symbol of 59 .. 66)
    return b"x" * 64, None, one(check)


def _eq(a, b):
    assert a == b, (a, b)


def growing(k, r):
    """counts 1, r, r^2 ... rounded: like Fibonacci counts (ratio 1.618) every symbol is rarer than all the rarer ones together, so
    the Huffman tree is one chain, k - 1 deep — with a ratio above Fibonacci's the chain also survives a stray symbol or two"""
    return [max(1, int(round(r ** i))) for i in range(k)]


def tag(i):
    """two bytes that occur together once: no four bytes that hold them repeat"""
    return [40 + i % 200, 40 + i // 200]


@scene
def growing_literals(seed):
    """the end of the block once and 16 byte values with counts growing by 1.7 (Fibonacci-like, see growing()), each followed by a
    two-byte tag so that no four bytes repeat: no match, the counts reach the code as they are.  The literal / length code reaches
    its 15-bit limit where an unlimited code would go deeper"""
    s = np.repeat(np.arange(16, dtype=np.uint8), growing(17, 1.7)[1:])
    np.random.default_rng(seed).shuffle(s)
    a = np.array([b for i, v in enumerate(s) for b in [v] + tag(i)], dtype=np.uint8)

    def check(m):
        assert m.btype == 2 and all(isinstance(t, int) for t in m.tokens)
        lit, _ = token_freqs(m.tokens)
        assert unlimited_depth(lit) > 15, unlimited_depth(lit)
        assert max(m.lit_lens) == 15
    return a, None, one(check)


@scene
def fibonacci_distances(seed):
    """records of a 3-byte random tag and a 4-byte copy, the copies' distance symbols with Fibonacci counts: 1 and 1 for distances 1
    and 2 (whose copies, xxxx and xyxy, would repeat between records), then falling from symbol 2 (distance 3) to symbol 17 (385 ..
    512).  A record's distance is taken inside its symbol's range so that the source's four bytes occur nowhere nearer and the byte
    before them differs, and its tag so that no other four bytes repeat.  The distance code reaches its 15-bit limit where an
    unlimited code would go deeper"""
    import deflate_tokens as dt
    rng = np.random.default_rng(seed)
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    syms = np.repeat(np.arange(18), [1, 1] + fib[:1:-1])
    rng.shuffle(syms)
    a = [int(b) for b in rng.integers(0, 256, 600)]
    last = {tuple(a[i:i + 4]): i for i in range(len(a) - 3)}      # four bytes -> where they last began
    for s in syms:
        lo, hi = dt.DIST_BASE[s], dt.DIST_BASE[s + 1] - 1
        for attempt in range(64):
            t = a[-3:] + [int(b) for b in rng.integers(0, 256, 3)]
            p, blk = len(a) + 3, None
            for d in rng.permutation(np.arange(lo, hi + 1))[:32]:
                d = int(d)
                if d >= 7 and (last.get(tuple(a[p - d:p - d + 4])) != p - d or a[p - d - 1] == t[5]):
                    continue
                blk = list(t)
                for _ in range(4):
                    blk.append(blk[-d] if d <= len(blk) else a[len(a) - 3 + len(blk) - d])
                new = [tuple(blk[i:i + 4]) for i in range(6)]
                if len(set(new)) == 6 and not any(w in last for w in new):
                    break
                blk = None
            if blk is not None:
                break
        assert blk is not None, "no record without a stray repeat"
        base = len(a) - 3
        a += blk[3:]
        for i in range(7):
            last[tuple(blk[i:i + 4])] = base + i
    a = np.array(a, dtype=np.uint8)

    def check(m):
        assert m.btype == 2
        _, dist = token_freqs(m.tokens)
        assert unlimited_depth(dist) > 15, unlimited_depth(dist)
        assert max(m.dist_lens) == 15
    return a, None, one(check)


@scene
def all_symbols(seed):
    """every literal, the 28 length symbols the parse can write (4 .. 258) and all 30 distance symbols: HLIT = 286, HDIST = 30.
    Copies at the base distance of every symbol: the near ones (symbols 0 .. 19) one behind the other with the long lengths, the far
    ones (1025 .. 24577) short, their sources together and zeros up to the copies"""
    import deflate_tokens as dt
    rng = np.random.default_rng(seed)
    out = list(rng.permutation(256).astype(np.uint8))
    for k in range(20):
        d, length = dt.DIST_BASE[k], dt.LEN_BASE[11 + k % 18]
        out.append(0xF0 + k % 8)
        x = list(rng.integers(1, 256, d, dtype=np.uint8))
        out += x
        for _ in range(length):
            out.append(out[-d])
        out.append(out[-d] ^ 0x5A)
    a = np.array(out, dtype=np.uint8)
    base = len(a) + 8
    far = [(dt.DIST_BASE[20 + i], dt.LEN_BASE[1 + i]) for i in range(10)]
    a = np.concatenate([a, zeros(base + 400 + far[-1][0] + 64 - len(a))])
    s = base
    for i, (d, length) in enumerate(far):
        x = rng.integers(1, 256, length, dtype=np.uint8)
        island(a, s, x, before=0x80 + i, after=0xA0 + i)
        island(a, s + d, x, before=0x90 + i, after=0xB0 + i)
        s += length + 3

    def check(m):
        assert m.btype == 2 and m.hlit == 286 and m.hdist == 30
        assert all(m.lit_lens[:256]) and all(m.lit_lens[258:286]) and m.lit_lens[257] == 0 and all(m.dist_lens)
    return a, None, one(check)


def cl_freqs(lit_lens, dist_lens):
    """how often the header spells each code-length symbol (dfl_rle_lengths' spelling of the lengths, deflate_codes.h)"""
    freq, lens, j = [0] * 19, list(lit_lens) + list(dist_lens), 0
    while j < len(lens):
        v, run = lens[j], 1
        while j + run < len(lens) and lens[j + run] == v:
            run += 1
        j += run
        if v == 0:
            while run >= 11:
                freq[18] += 1
                run -= min(run, 138)
            if run >= 3:
                freq[17] += 1
                run = 0
            freq[0] += run
        else:
            freq[v] += 1
            run -= 1
            while run >= 3:
                freq[16] += 1
                run -= min(run, 6)
            freq[v] += run
    return freq


def cl_family(fam, i):
    r = np.random.default_rng([i, len(fam)])
    if fam == "skewed_lengths":
        k = int(r.integers(8, 60))
        w = 0.5 ** np.arange(k)
        return r.choice(k, size=int(r.integers(200, 3000)), p=w / w.sum()).astype(np.uint8) * 3
    if fam == "random_alpha":
        alpha = int(r.integers(2, 257))
        return r.integers(0, alpha, int(r.integers(50, 2000)), dtype=np.uint8)
    return np.repeat(r.integers(0, 256, 40, dtype=np.uint8), r.integers(1, 40, 40))


@scene
def cl_limit(seed):
    """the code-length code held by its 7-bit limit (found by search, see CL_LIMIT_SEARCH)"""
    def check(m):
        assert m.btype == 2 and max(m.cl_lens) == 7
        assert unlimited_depth(cl_freqs(m.lit_lens, m.dist_lens)) > 7
    return cl_family(*CL_LIMIT_SEARCH[1]), None, one(check)


# the stored / dynamic switch: bytes of an alphabet of SWITCH[0] values, SWITCH[1] of them; with seed SWITCH[2] the dynamic block is
# within 64 bits BELOW 8 n + 32 (BTYPE 2), with seed SWITCH[3] at or within 64 bits above (BTYPE 0).  Found by
# test_deflate_scenes_cpu.py's search over the model (`--switch`); the CPU test checks the bits the model reports.
SWITCH = (229, 2000, 39, 108)   # 16031 and 16032 bits: the last dynamic and the first stored size of the rule


def switch_member(alpha, n, seed):
    return np.random.default_rng([seed, alpha]).integers(0, alpha, n, dtype=np.uint8)


if SWITCH:
    @scene
    def stored_dynamic_switch(seed):
        alpha, n, s_dyn, s_sto = SWITCH
        a = np.concatenate([switch_member(alpha, n, s_dyn), switch_member(alpha, n, s_sto)])
        return a, [0, n, 2 * n], lambda ms: (_eq(ms[0].btype, 2), _eq(ms[1].btype, 0), _eq((ms[0].hdist, ms[0].dist_lens), (2, [1, 1])))


# ---- the size sweep: a payload, not a token scene -------------------------------------------------------------------------------------

SWEEP_CLASSES = ("random", "text", "zeros")


@functools.lru_cache(maxsize=None)
def sweep(kind):
    """members of every length 0 .. 1100, then of every length 0xff00 - 9 .. 0xff00: every member start and size on every byte alignment
    of the staging loads, the CRC chunks and the gather kernels.  -> (payload, cuts)"""
    sizes = list(range(0, 1101)) + list(range(MAXPAY - 9, MAXPAY + 1))
    cuts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(cuts[-1])
    if kind == "random":
        a = np.random.default_rng(77).integers(0, 256, n, dtype=np.uint8).tobytes()
    elif kind == "text":
        line = b"".join(b"chr%d\t%d\t%d\t%.2f\n" % (1 + i % 7, 1000 + 37 * i, 1040 + 37 * i, (i * 7919 % 1000) / 10) for i in range(4000))
        a = (line * (n // len(line) + 1))[:n]
    else:
        a = bytes(n)
    return a, cuts
