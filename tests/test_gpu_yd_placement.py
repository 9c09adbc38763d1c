"""The placement of the YD items by list (<= 64 files: yd_lcount_k / yd_lscatter_k) against the oracle, on tiles of 1024 groups
that stress it: tiles whose items overflow the LDS staging array (every group in all 128 lists: several rounds per tile), tiles
that straddle a change of reference, group counts that are not a multiple of 1024, sparse lists, and chains that do or do not
renew where a read starts at end + 1 (no head) or at end + 2 (a head) of the reads before it.  A tile of groups always holds
items (every group has a file), so the smallest cases are a single group and a tile in which nothing passes."""
import numpy as np
import pytest

from helpers import tbk_debug, tile_from_records

from test_gpu_fuzz import _cmp

pytestmark = pytest.mark.gpu

M, N = 0, 3


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def by_list(monkeypatch):
    tbk_debug(monkeypatch, path="window")


def _chain(n_groups, tids, rng, spliced=False):
    """n_groups reads in coordinate order, one per group; each starts at the end of the one before plus a step from a cycle
    that holds +1 (start == end + 1: the chain goes on) and +2 (start == end + 2: a new chain), overlaps and wider gaps"""
    steps = [1, 2, -10, 1, 0, 2, 3, -25, 1, 1, 2, 40]
    reads, pos, tid_of = [], 1000, np.repeat(np.arange(len(tids)), -(-n_groups // len(tids)))[:n_groups]
    last_tid = None
    for i in range(n_groups):
        tid = int(tids[tid_of[i]])
        if tid != last_tid:
            pos, last_tid = 1000, tid  # (the next reference starts over at the same coordinates)
        ln = int(rng.choice([30, 45, 60, 75]))
        if spliced and i % 5 == 0:
            cig = [(ln // 2, M), (int(rng.integers(20, 200)), N), (ln - ln // 2, M)]
        else:
            cig = [(ln, M)]
        reads.append((tid, pos, cig))
        end = pos + sum(l for l, _ in cig) - 1
        pos = max(pos, end + steps[i % len(steps)])
    return reads


def _files(reads, n_files, strands):
    """strands(f, i) -> strand of read i in file f, or None: file f lacks the read"""
    files = []
    for f in range(n_files):
        rows = []
        for i, (tid, pos, cig) in enumerate(reads):
            s = strands(f, i)
            if s is not None:
                rows.append((tid, pos, 0, 60, s, 1, cig))
        files.append(rows)
    return files


def test_dense_tiles_overflow_the_staging_array(ctx):
    """64 files of the same reads with '.' strands: every group feeds all 128 lists, 1024 x 128 items per full tile — more than
    the staging array holds; 2600 groups: three tiles, the last one partial, the second one across a change of reference"""
    rng = np.random.default_rng(11)
    reads = _chain(2600, [0, 1], rng)
    want = _cmp(ctx, tile_from_records(_files(reads, 64, lambda f, i: ".")))
    assert want["n_groups"] == 2600 and int(np.asarray(want["yd"]).max()) > 0


def test_sparse_lists_and_reference_changes(ctx):
    """files hold random subsets of the reads with mixed strands: cells of every fill, empty lists, tiles that straddle three
    changes of reference, spliced reads among them"""
    rng = np.random.default_rng(12)
    reads = _chain(5000, [0, 2, 3, 5], rng, spliced=True)
    keep = rng.random((64, len(reads)))
    strand = rng.choice(np.array(["+", "-", "."]), size=(64, len(reads)), p=[0.4, 0.4, 0.2])
    dens = np.linspace(0.02, 0.95, 64)
    _cmp(ctx, tile_from_records(_files(reads, 64, lambda f, i: str(strand[f, i]) if keep[f, i] < dens[f] else None)))


@pytest.mark.parametrize("n_groups", [1, 1023, 1025, 2047])
def test_group_counts_around_a_tile(ctx, n_groups):
    """one group; one group fewer or more than a tile; the last tile one group short"""
    rng = np.random.default_rng(13 + n_groups)
    reads = _chain(n_groups, [0], rng)
    strands = np.array(["+", "-", "."])
    want = _cmp(ctx, tile_from_records(_files(reads, 5, lambda f, i: str(strands[(f + i) % 3]) if (f * 7 + i) % 4 else None)))
    assert want["n_groups"] >= 1


def test_heads_at_end_plus_one_and_two(ctx):
    """two reads per list: the second starts at end + 1 of the first (one chain, distance counted) or at end + 2 (two chains);
    both across a tile boundary (groups 1023 / 1024) as well as inside a tile"""
    for gap in (1, 2):
        reads = [(0, 10 * i + 1, [(5, M)]) for i in range(1023)]  # 1023 groups that do not touch
        e = 10 * 1022 + 1 + 4
        reads += [(0, e + 1000, [(20, M)]), (0, e + 1000 + 20 - 1 + gap, [(20, M)])]  # groups 1023, 1024: the pair at the seam
        e2 = e + 1000 + 20 - 1 + gap + 19
        reads += [(0, e2 + 1000, [(30, M)]), (0, e2 + 1000 + 30 - 1 + gap, [(30, M)])]  # and a pair inside the second tile
        _cmp(ctx, tile_from_records(_files(reads, 3, lambda f, i: "." if f == 0 else "+")))


def test_nothing_passes(ctx):
    """every record filtered: no group, no tile"""
    reads = _chain(50, [0], np.random.default_rng(14))
    files = [[(t, p, 0, 0, ".", 1, c) for t, p, c in reads] for _ in range(4)]
    _cmp(ctx, tile_from_records(files), min_qual=1)
