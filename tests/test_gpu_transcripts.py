"""tbk_tx_summary (tiebrush_amd/csrc/txsum.hip) through Context.tx_summary against tx_model, on the hand-placed scenes of
tx_scenes and a seeded random case; rows from host and from device memory.

The numeric contract: covered, max, exons_hit, introns_hit and junc_min are exact; sum and junc_sum are exact where every row value on
the transcript is a multiple of 2^-3 and the sums stay below 2^50 (tx_model.exact / jexact), else within gamma(pieces + 1) x the sum of
the absolute terms (tx_model.check).  The per-exon columns are, bit for bit, Context.cov_summary's for the exons given as features, and
in_junc its junc for the introns given as features — for any values."""
import numpy as np
import pytest

import tx_model as tm
import tx_scenes as ts

pytestmark = pytest.mark.gpu

COLS = ("covered", "sum", "max", "exons_hit", "introns_hit", "junc_min", "junc_sum")
PARTS = ("ex_covered", "ex_sum", "ex_max", "in_junc")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    out = {name: f() for name, f in ts.SCENES.items()}
    return {name: (rows, tx, tm.per_row(rows, tx)) for name, (rows, tx, _) in out.items()}


def _device(rows):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in rows.items()}


def _check(got, model):
    assert got["covered"].dtype == np.uint64 and got["exons_hit"].dtype == np.uint32 and got["introns_hit"].dtype == np.uint32
    assert all(got[k].dtype == np.float64 for k in ("sum", "max", "junc_min", "junc_sum")) and len(got["sum"]) == len(model)
    for k in range(len(model)):
        tm.check(got, model, k)


def _check_parts(ctx, got, rows, tx):
    """the per-exon columns against cov_summary of the exons / the introns as features, bit for bit"""
    ex, (inf, at) = ctx.cov_summary(rows, tm.exon_feats(tx)), tm.intron_feats(tx)
    for k in ("covered", "sum", "max"):
        assert got["ex_" + k].tobytes() == ex[k].tobytes(), k
    want = np.zeros(len(tx["ex_beg"]))
    if len(at):
        want[at] = ctx.cov_summary(rows, inf)["junc"]
    assert got["in_junc"].tobytes() == want.tobytes()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", sorted(ts.SCENES))
def test_scenes(ctx, scenes, name, mem):
    rows, tx, model = scenes[name]
    given = _device(rows) if mem == "device" else rows
    got = ctx.tx_summary(given, tx, parts=True)
    _check(got, model)
    if name == "thirds":
        assert not any(tm.exact(m) for m in model)                  # this scene is the one held to the bound
    _check_parts(ctx, got, given, tx)
    again = ctx.tx_summary(given, tx, parts=True)
    for k in COLS + PARTS:
        assert got[k].tobytes() == again[k].tobytes(), k            # the same inputs, the same bits
    plain = ctx.tx_summary(given, tx)                               # the parts in arena scratch: the same transcripts
    assert sorted(plain) == sorted(COLS)
    for k in COLS:
        assert got[k].tobytes() == plain[k].tobytes(), k


def test_random_case(ctx):
    rows, tx = ts.random_case()
    model = tm.per_row(rows, tx)
    got = ctx.tx_summary(rows, tx, parts=True)
    _check(got, model)
    assert all(tm.exact(m) and tm.jexact(m) for m in model)
    _check_parts(ctx, got, rows, tx)
    dev = ctx.tx_summary(_device(rows), tx, parts=True)
    for k in COLS + PARTS:
        assert got[k].tobytes() == dev[k].tobytes(), k


def test_missing_tracks_and_no_rows(ctx, scenes):
    """rows without the interval or the junction columns leave those out; no row at all gives zeros; a table without strands is all '.'"""
    import feature_scenes as fs
    rows, tx, model = scenes["list65"]
    full = ctx.tx_summary(rows, tx, parts=True)
    only_c = ctx.tx_summary({k: v for k, v in rows.items() if k[:3] == "iv_"}, tx, parts=True)
    assert sorted(only_c) == sorted(COLS[:4] + PARTS[:3])
    only_j = ctx.tx_summary({k: v for k, v in rows.items() if k[:2] == "j_"}, tx, parts=True)
    assert sorted(only_j) == sorted(COLS[4:] + PARTS[3:])
    for k, v in list(only_c.items()) + list(only_j.items()):
        assert v.tobytes() == full[k].tobytes(), k
    empty = ctx.tx_summary(fs.rows_of(), tx, parts=True)
    assert sorted(empty) == sorted(COLS + PARTS) and all(not empty[k].any() for k in empty)
    dots = dict(tx, strand=np.full(len(tx["tid"]), ord("."), np.uint8))
    a, b = ctx.tx_summary(rows, dots), ctx.tx_summary(rows, {k: v for k, v in tx.items() if k != "strand"})
    for k in COLS:
        assert a[k].tobytes() == b[k].tobytes(), k
    _check(a, tm.per_row(rows, dots))


def _good(ctx, scenes):
    rows, tx, model = scenes["isoforms"]
    _check(ctx.tx_summary(rows, tx), model)


def _tx(**kw):
    base = ts.table([(1, "+", [(100, 200), (300, 400)]), (1, "-", [(50, 60)])])
    base.update({k: np.array(v, base[k].dtype) for k, v in kw.items()})
    return base


REFUSED = {"no transcript": dict(tx_off=[0], tid=[], strand=[]), "tx_off[0] != 0": dict(tx_off=[1, 2, 3]), "an empty transcript": dict(tx_off=[0, 3, 3]),
           "last offset != n_exon": dict(tx_off=[0, 2, 2]), "offsets descend": dict(tx_off=[0, 4, 3]), "tid < 0": dict(tid=[1, -1]), "ex_beg < 0": dict(ex_beg=[-1, 300, 50]),
           "ex_end == ex_beg": dict(ex_end=[200, 400, 50]), "ex_end < ex_beg": dict(ex_end=[200, 400, 40]), "exons out of order": dict(ex_beg=[300, 100, 50], ex_end=[400, 200, 60]),
           "exons overlap": dict(ex_end=[301, 400, 60]), "exons abut": dict(ex_end=[300, 400, 60]), "strand": dict(strand=[ord("+"), ord("*")])}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_tables(ctx, scenes, what):
    from tiebrush_amd._lib import TbkError
    rows = scenes["isoforms"][0]
    with pytest.raises(TbkError) as e:
        ctx.tx_summary(rows, _tx(**REFUSED[what]))
    assert e.value.status == -1
    _good(ctx, scenes)


@pytest.mark.parametrize("asked", [("ex_covered",), ("ex_sum", "ex_max"), ("ex_covered", "ex_max", "in_junc")])
def test_refused_part_columns(ctx, scenes, asked):
    from tiebrush_amd._lib import TbkError
    rows = scenes["isoforms"][0]
    with pytest.raises(TbkError) as e:
        ctx.tx_summary(rows, _tx(), parts=asked)
    assert e.value.status == -1 and "together" in str(e.value)
    ok = ctx.tx_summary(rows, _tx(), parts=("in_junc",))            # in_junc alone is its own option
    assert sorted(ok) == sorted(COLS + ("in_junc",))
    _good(ctx, scenes)


def _swap(rows, key, i, j):
    out = {k: v.copy() for k, v in rows.items()}
    for k in out:
        if k.startswith(key):
            out[k][[i, j]] = out[k][[j, i]]
    return out


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("what", ["iv order", "iv overlap", "j order", "j strand"])
def test_refused_rows(ctx, scenes, what, mem):
    from tiebrush_amd._lib import TbkError
    rows, tx, model = scenes["list65"]
    n = len(rows["iv_tid"])
    if what == "iv order":
        bad = _swap(rows, "iv_", 600, 601)
    elif what == "iv overlap":
        bad = {k: v.copy() for k, v in rows.items()}
        bad["iv_end"][n - 3] += 5
    elif what == "j order":
        bad = _swap(rows, "j_", 3, 9)
    else:
        bad = {k: v.copy() for k, v in rows.items()}
        bad["j_start"][1], bad["j_end"][1] = bad["j_start"][0], bad["j_end"][0]      # the same triple with a smaller strand byte behind it
        bad["j_strand"][0], bad["j_strand"][1] = ord("-"), ord("+")
    with pytest.raises(TbkError) as e:
        ctx.tx_summary(_device(bad) if mem == "device" else bad, tx)
    assert e.value.status == -1 and "sorted" in str(e.value)
    _check(ctx.tx_summary(_device(rows) if mem == "device" else rows, tx), model)
