"""Hand-built tiles for the items of the YD stage where they are placed by list (tiebrush_amd/csrc/collapse.hip): a far item — several
exons, not the exact shape M N M — carries the offset of its exon list in place of its end, yd_wave_k fetches its items two batches of
64 deep, no list machine looks a group up, and the item -> group word is a 16-bit index inside the tile of 1024 groups.  What can
go wrong depends on where far items fall relative to the batches of a chain, on how many exons they have, on where groups fall relative
to the tiles and on how many items a tile holds relative to the staging rounds of yd_lscatter_k.

Every read is a group of its own (no two reads share start and CIGAR), so in a scene of one file and one strand the items of the one
list are the reads in coordinate order.  A far read of variant k has exons of 10 bases; exon j >= 1 starts 100 j + shift + 3 k behind
the read's start.  A PROBE is a read of 3 bases that starts 2 + k % 5 bases inside such an exon: its distance is measured from the
exon's start as long as the exon is a node of its own, so exons read at a wrong offset change it (or zero it).

tests/test_yd_item_scenes_cpu.py proves every scene's claim with the oracle; tests/test_gpu_yd_items.py runs the scenes.  A scene and
its oracle result are built once per process."""
import functools
import heapq

import numpy as np

from helpers import tile_from_records

M, N = 0, 3
NT = 1024                     # groups of a tile (YS_NT)
CAP_OLD, CAP = 15360, 14336   # staging slots of a round of yd_lscatter_k before and since the exon offsets took 4 KB of its LDS
FILL = [(10, M)]
PROBE = [(3, M)]


BACK = 1 << 20                # a chain's first read ends in an exon this far behind its start (see chain())


def far_cigar(k, m=3, shift=0, back=False):
    cig, end = [(10, M)], 10
    for j in range(1, m):
        s = BACK if back and j == m - 1 else 100 * j + shift + 3 * k
        cig += [(s - end, N), (10, M)]
        end = s + 10
    return cig


def probe_offset(k):
    return 2 + k % 5


def rec(pos, cig, strand="+"):
    return (0, int(pos), 0, 60, strand, 1, cig)


def span(cig):
    return sum(l for l, _ in cig)


def chain(n, far_at, m=3, k_step=0):
    """one chain of n reads, far reads (m exons) at the items of far_at, item 0 among them; a far read that follows a far read starts
    where the probe of that read's exon 1 would; probes fill the items behind a far read as far as there is room, overlapping fillers
    the rest.  The LAST exon of item 0 lies 2^20 bases out and has no probe: the reference drops the exons of a read that lie behind the
    last node of a list that is not empty (mergeRead's walk runs off the list), so without a node behind everything the exons of a far
    read in mid-chain would never enter the list; it also keeps the chain in one piece whatever the gaps.
    -> (records, kinds): kinds[i] in 'far' / 'far-probe' (a far read that probes the far read before it) / 'probe' / 'fill'.
    k_step: added to the variant of every far read's exons while every read keeps its start — the CPU test's other tile, in which
    the probes meet exons that begin 3 k_step bases later"""
    far_at = sorted(far_at)
    assert far_at[0] == 0
    recs, kinds, pending = [], [], []
    pos, nfar = 1000, 0
    for i in range(n):
        while pending and pending[0] <= pos:
            heapq.heappop(pending)  # (two probes on one base: one read)
        if i in far_at:
            after_far = bool(kinds) and kinds[-1].startswith("far") and bool(pending)
            p = heapq.heappop(pending) if after_far else (pos + 3 if recs else pos)
            if not after_far:
                pending = []  # (probes that found no room)
            k = nfar % 7
            shift = 40 if after_far else 0
            recs.append(rec(p, far_cigar(k + k_step, m, shift, back=i == 0)))
            kinds.append("far-probe" if after_far else "far")
            for j in range(1, m - 1 if i == 0 else m):
                heapq.heappush(pending, p + 100 * j + shift + 3 * k + probe_offset(k))
            nfar += 1
            pos = p
        elif pending:
            pos = heapq.heappop(pending)
            recs.append(rec(pos, PROBE))
            kinds.append("probe")
        else:
            pos += 3
            recs.append(rec(pos, FILL))
            kinds.append("fill")
    assert all(a[1] < b[1] for a, b in zip(recs, recs[1:]))
    return recs, kinds


def edge_items(n):
    return sorted({0, 63, 64, n - 2, n - 1} & set(range(n)))


# ---- the scenes: name -> (function -> dict(files, ...), claim) ---------------------------------------------------------------------
# claim keys (test_yd_item_scenes_cpu.py): chains = lengths of the chains of list 0; far = items of list 0 that are far;
# probes = at least that many probing reads with a non-zero YD that another exon geometry changes; ng; tile_items = items per tile;
# peaks = groups whose YD is larger than that of both neighbours; far_groups = output places of far groups;
# probe_groups = groups whose YD is non-zero and changes with the far groups' exon geometry
SCENES = {}


def scene(name, **claim):
    def reg(fn):
        SCENES[name] = (fn, claim)
        return fn
    return reg


def _one_list(n, far_at, m=3, k_step=0):
    recs, kinds = chain(n, far_at, m, k_step)
    return dict(files=[recs], kinds=kinds)


BATCH_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 193)
for _n in BATCH_EDGES:
    # far reads at items 0, 63, 64, n - 2 and n - 1.  (The last item of a chain has no reader of its exons — the list is cleared
    # behind it — so item n - 1 is there for the loads behind a chain's end; it starts inside exon 1 of item n - 2 and probes that.)
    scene("edges-%d" % _n, chains=[_n], far=edge_items(_n), probes=min(_n - 1, 2) if _n > 1 else 0)(
        functools.partial(_one_list, _n, edge_items(_n)))

scene("batch-all-far", chains=[70], far=list(range(70)), probes=60)(functools.partial(_one_list, 70, range(70)))

for _m in (5, 9, 65):
    # 5 exons: exons 3 and 4 are loaded inside the item loop; 9 exons outgrow a lane's list, 65 the 64 lanes: yd_run_k takes the chain
    scene("exons-%d-first" % _m, chains=[_m + 30], far=[0], probes=_m - 2)(functools.partial(_one_list, _m + 30, [0], _m))
    scene("exons-%d-later" % _m, chains=[2 * _m + 30], far=[0, _m + 3], probes=2 * _m - 3)(functools.partial(_one_list, 2 * _m + 30, [0, _m + 3], _m))


PEAKS = (1, 1023, 1024, 2047, 2048, 2049)


@scene("index-2050", ng=2050, peaks=list(PEAKS), tile_items=[3 * 1024, 3 * 1024, 3 * 2])
def _index_2050(k_step=0):
    """2050 groups, each present in three files: tiles of 3072, 3072 and 6 items.  Groups 1023, 1024, 2047, 2048, 2049 and 1 hold the
    largest distance of their neighbourhood (30 and more; the others 7 at the most): a group index that lost or gained a tile's base
    moves it a multiple of 1024 groups away.  (Group 0 opens every list: nothing lies before it, its distance is zero; its neighbour,
    group 1, stands for the first entry of a tile.)"""
    recs, pos, peak = [], 1000, set(PEAKS)
    for g in range(2050):
        if g in peak:
            pos += 3 if (g - 1) in peak else 30   # inside the opener of 40 bases / the island the peak before it stretched
            recs.append(rec(pos, [(12, M)]))
        elif (g + 1) in peak:
            pos += 60
            recs.append(rec(pos, [(40, M)]))      # the opener of a peak: a chain of its own
        elif (g - 1) in peak:
            pos += 60
            recs.append(rec(pos, [(12, M)]))      # behind a peak: a chain of its own
        else:
            pos += 7 if g % 2 else 60             # pairs: an opener and a follower at distance 7
            recs.append(rec(pos, [(12, M)]))
    return dict(files=[list(recs), list(recs), list(recs)])


DENSE_FAR = (0, 500, 1017)
DENSE_PROBES = (6, 506, 1023)


def _dense(n_files, k_step=0):
    """1024 groups present in every one of n_files files with strand '.', which feeds both lists of a file: 2048 n_files items in one
    tile, list-major — group g's item of list c has index 1024 c + g, so in the larger tiles every group's items of the lists from 14
    on are staged in the second round.  A read of 10 bases every 20: every read opens a chain, except behind the far groups (0, 500,
    1017; variant 5: exon 1 begins 115 bases in), whose span holds the next ten reads in their chain; the sixth of them (groups 6, 506,
    1023) starts 5 bases inside exon 1 and reports that distance.  A group's YD is the maximum over its items, so with more than 7
    files those three groups are present only in the files from 7 on — lists 14 and up: their YD then comes from items of the second
    round alone, next to far items of the second round (lists 0 .. 13 hold 1021 items each, list 14 begins at index 14 294: the far
    items of groups 500 and 1017 in every list from 14 on, and of group 0 from list 15 on, have indices >= 14 336)."""
    recs, pos = [], 1000
    for g in range(NT):
        pos += 20
        recs.append(rec(pos, far_cigar(5 + k_step) if g in DENSE_FAR else FILL, "."))
    early = [r for g, r in enumerate(recs) if g not in DENSE_PROBES]
    return dict(files=[list(recs) if n_files <= 7 or f >= 7 else list(early) for f in range(n_files)])


# 7, 8 and 9 files: 14 336 items (one round exactly), 16 342 and 18 390 (two rounds, staged 15 360 at a time and 14 336 alike)
for _f, _items in ((7, 14336), (8, 16384 - 42), (9, 18432 - 42)):
    scene("dense-%d" % _f, ng=NT, tile_items=[_items], far_groups=list(DENSE_FAR), probe_groups=list(DENSE_PROBES),
          second_round=_items > CAP)(functools.partial(_dense, _f))


def _far_places(which, k_step=0):
    """two tiles of groups, one read each, all in one chain of one list; far groups at `which`, each followed by its probes as far as
    there is room"""
    recs, kinds = chain(2 * NT, which, 3, k_step)
    return dict(files=[recs], kinds=kinds)


scene("far-first-of-tile", far=[0, NT], far_groups=[0, NT], probes=3)(functools.partial(_far_places, [0, NT]))
scene("far-last-of-tile", far=[0, NT - 1, 2 * NT - 1], far_groups=[0, NT - 1, 2 * NT - 1], probes=3)(
    functools.partial(_far_places, [0, NT - 1, 2 * NT - 1]))
scene("tile-of-far-groups", far=[0] + list(range(NT, 2 * NT)), far_groups=[0] + list(range(NT, 2 * NT)), probes=500)(
    functools.partial(_far_places, [0] + list(range(NT, 2 * NT))))

FAR_OFFSET_SCENES = [n for n in SCENES if n.startswith(("edges-", "batch-", "exons-", "far-", "tile-of", "dense-"))]


@functools.lru_cache(maxsize=None)
def build(name, k_step=0):
    fn = SCENES[name][0]
    return fn(k_step=k_step) if k_step else fn()


@functools.lru_cache(maxsize=None)
def get(name, k_step=0):
    return tile_from_records(build(name, k_step)["files"])


@functools.lru_cache(maxsize=None)
def oracle(name, k_step=0):
    from oracle import oracle_ffi as orc
    return orc.collapse(get(name, k_step), want_rec_group=True, strategy=0)


def chains_of(recs):
    """lengths of the chains of one list: a read opens a chain when it starts beyond end + 1 of every read before it"""
    out, reach = [], None
    for r in recs:
        if reach is None or r[1] > reach + 1:
            out.append(0)
            reach = r[1] + span(r[6]) - 1
        out[-1] += 1
        reach = max(reach, r[1] + span(r[6]) - 1)
    return out
