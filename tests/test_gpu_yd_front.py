"""The front end of the YD stage where the items are placed by list (<= 64 files): the count pass (yd_lcount_k) makes the groups'
records (tid + 1, start, end, exon word) itself, and the offsets of the far groups' exon lists — groups of several exons that are
not the exact shape M N M — come from one more row of the placement's table and a prefix inside the tile (yd_lscatter_k) instead of
a device-wide scan.  Every case is compared with the oracle; the cases marked A/B also run with yd_front=split — the records by
yd_groups_k and the offsets by the scan, as on the other paths — and must give the same arrays.  Tiles hold 1024 groups, so the
shapes sit around group 1023 / 1024: far groups on both sides of a seam, a tile of nothing but far groups beside a tile without one,
groups whose exon count needs the representative's CIGAR, and tie sets, whose members the permutation reorders, across a seam."""
import numpy as np
import pytest

from helpers import tbk_debug, tile_from_records

from test_gpu_fuzz import _cmp

pytestmark = pytest.mark.gpu

M, I, D, N, S = 0, 1, 2, 3, 4
PLAIN = [(40, M)]
FAR = [(20, M), (50, N), (20, M), (60, N), (20, M)]  # three exons: the exon arrays hold them
STEP = 7  # reads overlap their neighbours: chains with distances to count


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def by_list(monkeypatch):
    tbk_debug(monkeypatch, path="window")


def _tile(cigars, n_files=3, strands="+-.", mapq=60, extra=()):
    """one read per group, group i at 1000 + STEP * i with CIGAR cigars[i], in file i % n_files with that file's strand;
    extra: (file, pos, strand, cigar) reads beside them (in coordinate order inside their file)"""
    files = [[] for _ in range(n_files)]
    for i, cig in enumerate(cigars):
        f = i % n_files
        files[f].append((0, 1000 + STEP * i, 0, mapq, strands[f % len(strands)], 1, cig))
    for f, pos, s, cig in extra:
        files[f].append((0, pos, 0, mapq, s, 1, cig))
    for rows in files:
        rows.sort(key=lambda r: r[1])
    return tile_from_records(files)


def _got(ctx, tile, **kw):
    from tiebrush_amd import api
    return api.to_numpy(ctx.collapse(tile, want_rec_group=True, **kw))


def _ab(ctx, monkeypatch, tile, **kw):
    """against the oracle, then fused against split"""
    want = _cmp(ctx, tile, **kw)
    fused = _got(ctx, tile, **kw)
    tbk_debug(monkeypatch, yd_front="split")
    split = _got(ctx, tile, **kw)
    tbk_debug(monkeypatch, yd_front=None)
    for k in ("yd", "yc", "yx", "rep"):
        assert np.array_equal(np.asarray(fused[k]), np.asarray(split[k])), k
        assert np.array_equal(np.asarray(split[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), k
    return want


def _seam_cigars():
    cigars = [PLAIN] * 2050
    for g in (0, 1022, 1023, 1024, 1025, 2049):
        cigars[g] = FAR
    return cigars


def test_far_groups_at_tile_seams(ctx, monkeypatch):
    """A/B.  2050 groups, far ones at 0, 1022 - 1025 and the last: the prefix inside a tile, the tiles' bases, and the first and the
    last entry of the table's extra row (tile 2 holds two groups, the second of them far)"""
    want = _ab(ctx, monkeypatch, _tile(_seam_cigars()))
    assert want["n_groups"] == 2050 and int(np.asarray(want["yd"]).max()) > 0


@pytest.mark.parametrize("far_first", [True, False])
def test_a_tile_of_far_groups_beside_a_tile_without(ctx, far_first):
    """1024 three-exon groups and 1024 single-exon groups, in both orders: the largest sum inside a tile (3 x 1024 exons), a base that
    follows it, and a row entry of zero"""
    cigars = [FAR] * 1024 + [PLAIN] * 1024 if far_first else [PLAIN] * 1024 + [FAR] * 1024
    want = _cmp(ctx, _tile(cigars))
    assert want["n_groups"] == 2048


WALKED = [
    [(15, M), (2, I), (15, M)],           # one exon, hashed key
    [(15, M), (3, D), (15, M)],
    [(5, S), (30, M)],                    # (one operation once clipped, strategy="clip")
    [(2000, M), (30, N), (20, M)],        # M N M with a first block >= 2^10: no X2 word
    [(20, M), (1048576, N), (20, M)],     # gap >= 2^20
    [(20, M), (40, N), (10, M), (2, I), (10, M)],
]


@pytest.mark.parametrize("strategy", ["cigar", "clip", "exon"])
def test_exon_counts_from_the_cigar_walk(ctx, strategy):
    """groups whose key word is no exact code at the first and the last lane of a wave and of a tile (groups 0, 63, 64, 1023, 1024)
    among plain reads: their exon word comes from walk_exons over the representative's CIGAR, inside the count pass"""
    for cig in WALKED:
        cigars = [PLAIN] * 1030
        for g in (0, 63, 64, 1023, 1024):
            cigars[g] = cig
        want = _cmp(ctx, _tile(cigars), strategy=strategy)
        assert want["n_groups"] == 1030, cig


TIES = [[(10, M), (2, I), (10, M)], [(12, M), (2, I), (8, M)], [(8, M), (2, I), (12, M)]]
TIE_FAR = [(6, M), (4, N), (6, M), (2, N), (2, M)]  # the same span, three exons


@pytest.mark.parametrize("with_far", [False, True])
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_tie_sets_through_the_permutation(ctx, monkeypatch, with_far, order):
    """A/B.  Groups that share (tid, start, strand, end) are ordered by the reference comparator (col_tie_sort_k): the record of
    output place o must be that of group gperm[o].  The set follows 1022 plain groups, so it covers places 1022 - 1024 (- 1025
    with the far member) across the seam; its members lie in different files, in two arrangements"""
    members = [TIES[j] for j in order] + ([TIE_FAR] if with_far else [])
    pos = 1000 + STEP * 1022
    extra = [(j % 3, pos, "+", cig) for j, cig in enumerate(members)]
    extra += [(j % 3, pos + 5 + STEP * j, "+", PLAIN if j % 4 else FAR) for j in range(8)]  # and a few groups behind the set
    want = _ab(ctx, monkeypatch, _tile([PLAIN] * 1022, strands="+", extra=extra))
    assert want["n_groups"] == 1022 + len(members) + 8


@pytest.mark.parametrize("n_groups", [1, 1023, 1025])
def test_group_counts_around_a_tile(ctx, n_groups):
    """one group (a far one); one fewer and one more than a tile, the last group far"""
    cigars = [PLAIN] * n_groups
    cigars[-1] = FAR
    cigars[n_groups // 2] = FAR
    want = _cmp(ctx, _tile(cigars))
    assert want["n_groups"] == n_groups


def test_nothing_passes(ctx):
    """every record filtered (MAPQ 0 under min_qual=1): no group, no tile, no row to scan"""
    _cmp(ctx, _tile(_seam_cigars()[:1100], mapq=0), min_qual=1)


def test_literal_machine_reads_every_far_offset(ctx, monkeypatch):
    """yd_literal=1: yd_run_k runs every chain and reads the exon offset and the exon arrays of every far item"""
    tbk_debug(monkeypatch, yd_literal=1)
    want = _cmp(ctx, _tile(_seam_cigars()))
    assert want["n_groups"] == 2050


def test_without_the_record_map(ctx):
    """no record -> group map is asked for: nothing reads the inverse of the tie permutation, and col_tie_sort_k does not write it"""
    from tiebrush_amd import api
    tile = _tile(_seam_cigars())
    want = _cmp(ctx, tile)
    got = api.to_numpy(ctx.collapse(tile))
    assert got["n_groups"] == want["n_groups"]
    for k in ("rep", "yc", "yx", "yd"):
        assert np.array_equal(np.asarray(got[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), k


def test_65_files_take_the_radix_split(ctx):
    """more than 64 files: the items go through the radix split, whose records yd_groups_k still makes"""
    cigars = [FAR if g % 9 == 0 else PLAIN for g in range(200)]
    want = _cmp(ctx, _tile(cigars, n_files=65))
    assert want["n_groups"] == 200
