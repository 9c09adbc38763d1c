"""The rule of `--strand-cov` without a GPU: the model (strand_model.py), api.split_strand_host (numpy) and the command
lines' host splitter (tbh::split_strand_host through libtbh.so) agree on every scene; on the goldens the three parts' oracle rows, spread
per base, add up to the whole file's; and the goldens give the cases the GPU tests lean on (all three classes, one empty, two empty)."""
import os

import numpy as np
import pytest

import strand_model as stm
import strand_scenes as sts
from helpers import GOLDEN

SCENES = sts.scenes()
GOLDENS = {"t1": ("t1/t1.bam", (2504, 58, 917)), "t12": ("t12.bam", (4405, 4169, 917)), "t2": ("t2/t2.bam", (4010, 4169, 0)),
           "t1s0": ("t1/t1s0.bam", (58411, 0, 0))}


@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_three_splitters_agree(scene):
    from tiebrush_amd import api
    want = stm.split(scene.cin)
    for name, got in (("numpy", api.split_strand_host(scene.cin)), ("libtbh", api._split_strand_libtbh(scene.cin))):
        assert len(got) == 3
        for s in range(3):
            assert stm.same(got[s], want[s]) is None, (name, s, stm.same(got[s], want[s]))
    n_mapped = int(((scene.cin.flag & 4) == 0).sum())
    assert sum(p.n_records for p in want) == n_mapped
    assert sum(len(p.cig) for p in want) == int(np.diff(scene.cin.cig_off.astype(np.int64))[(scene.cin.flag & 4) == 0].sum())
    for s, p in enumerate(want):
        assert all(stm.classify(int(b)) == s for b in p.strand) and int(p.cig_off[0]) == 0 and int(p.cig_off[-1]) == len(p.cig)


def test_the_scenes_hold_what_they_claim():
    by = sts.by_name()
    assert {s.cin.n_records for s in SCENES} >= set(sts.SIZES) | {sts.TILE - 1, sts.TILE, sts.TILE + 1}
    odd = by["pattern/odd_bytes"].cin
    others = set(int(b) for b in odd.strand) - {ord("+"), ord("-"), ord(".")}
    assert len(others) >= 4 and all(int(b) in others | {ord(".")} for b in stm.split(odd)[2].strand)
    for name, cls in (("pattern/plus_first", 0), ("pattern/minus_last", 1), ("pattern/none_first", 2), ("pattern/none_last", 2)):
        assert stm.split(by[name].cin)[cls].n_records == 1, name
    assert all(p.n_records == 0 for p in stm.split(by["unmapped/u_all"].cin))
    n = by["long/200+1000/edge"].cin
    words = np.diff(n.cig_off.astype(np.int64))
    assert words[sts.TILE - 1] == 200 and words[sts.TILE] == 1000 and not by["long/200+1000/edge"].cov_ok and by["long/200/edge"].cov_ok
    assert int(np.diff(by["long/10_words"].cin.cig_off.astype(np.int64)).max()) == sts.LANE_WORDS + 2
    w = by["weights/odd"].cin
    assert (w.yc == 0.0).any() and (w.yc == 5e-324).any() and (w.yc != np.floor(w.yc)).any() and int(w.yx.min()) >= 1 << 32
    for u in ("u_first", "u_last", "u_seventh"):
        f = by["unmapped/%s" % u].cin.flag
        assert (f & 4).any() and not (f & 4).all()


def test_strand_none_is_refused():
    from tiebrush_amd import api, soa
    c = sts.by_name()["size/2/mod3"].cin
    with pytest.raises(ValueError):
        api.split_strand_host(soa.CovInput(c.tid, c.pos, c.flag, c.cig_off, c.cig, c.yc, None, c.yx))


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_golden_parts_add_up(name, bam_loader):
    """integral YC: per base, the parts' coverage adds up to the whole file's, exactly"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import soa
    path, counts = GOLDENS[name]
    b = bam_loader(os.path.join(GOLDEN, path), keep_names=False)
    cin = soa.cov_input_from_bam(b)
    assert not (cin.flag & 4).any()                                    # (no golden holds an unmapped record: the scenes carry that case)
    parts = stm.split(cin)
    assert tuple(p.n_records for p in parts) == counts
    assert np.all(cin.yc == np.floor(cin.yc))
    whole = orc.coverage(cin, want_junc=False)
    lens = {}
    for t, e in zip(whole["iv_tid"], whole["iv_end"]):
        lens[int(t)] = max(lens.get(int(t), 0), int(e))
    total = stm.per_base(whole, lens)
    acc = {t: np.zeros(n, np.float64) for t, n in lens.items()}
    for p in parts:
        if p.n_records == 0:
            continue
        pb = stm.per_base(orc.coverage(stm.for_oracle(p), want_junc=False), lens)
        for t in acc:
            acc[t] += pb[t]
    for t in acc:
        assert np.array_equal(acc[t], total[t]), (name, t)
