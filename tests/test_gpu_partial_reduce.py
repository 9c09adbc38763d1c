"""The owner's merge-reduce (tbk_partial_reduce: pr_sample_rank_k, wg_split_k, the offsets build, pr_merge_k, pr_compact_k) on the
hand-built scenes of partial_scenes.py, against the CPU oracle's collapse of the received rows under the priority rule — array for
array, no tolerance: integers and exactly representable doubles.

Per scene and order of the ranks: every rank's ctx.collapse, partial_keys and partial_pack (the sender's side as the multi-rank
driver runs it), the rows end to end, the scene's edits, ctx.partial_reduce.  tests/test_partial_scenes_cpu.py has proved that the
scene sits on its edge and that no window of a scene expected to be accepted exceeds PR_CAP: a refusal there is a failure here, not a
fallback.  A scene that must be refused is refused with the status its edge names, and the same context then reduces a good scene."""
import numpy as np
import pytest

from helpers import tbk_debug

from dist_helpers import STRAT, check_against_flat
import partial_scenes as ps

pytestmark = pytest.mark.gpu

COV_KEYS = ("iv_tid", "iv_start", "iv_end", "iv_val", "j_tid", "j_start", "j_end", "j_strand", "j_val")


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def received(ctx, name, reverse, monkeypatch):
    """the sender's side of every rank -> (rows [n2, 12] int32 on the host, unedited; CIGAR words, device; run_off)"""
    import torch
    from tiebrush_amd import api
    sc = ps.SCENES[name]
    tiles, first = ps.tiles_of(name, reverse)
    rows_all, cig_all, cnt = [torch.zeros((0, 12), dtype=torch.int32, device="cuda:0")], [torch.zeros(0, dtype=torch.int32, device="cuda:0")], []
    for t, f in zip(tiles, first):
        if t is None:                    # a rank without records sends nothing
            cnt.append(0)
            continue
        dt = api.to_device(t, "cuda:0")
        fin = ctx.collapse(dt, strategy=sc.strategy, want_coords=True, want_effend=True)
        key, _, bad = ctx.partial_keys(dt, fin)
        assert bad == 0
        if sc.mask is not None:          # (the hash word masked away at the pack only: the local collapse keeps its keys)
            tbk_debug(monkeypatch, hash_mask=sc.mask)
        rows, cigw, tab = ctx.partial_pack(dt, fin, key, None, 1, f, strategy=sc.strategy)
        if sc.mask is not None:
            tbk_debug(monkeypatch, hash_mask=None)
        th = tab.cpu().numpy()
        rows_all.append(rows.clone())
        cig_all.append(cigw[:int(th[0, 2])].clone())
        cnt.append(int(th[0, 1]))
    run_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    return torch.cat(rows_all).cpu().numpy(), torch.cat(cig_all), run_off


def reduce_scene(ctx, name, reverse, monkeypatch):
    """-> (status, result dict on the host or None, coverage of the view or None, rows as reduced (host), run_off, CIGAR words (host))"""
    import torch
    from tiebrush_amd import api
    from tiebrush_amd._lib import TbkError
    sc = ps.SCENES[name]
    rows_h, cig, run_off = received(ctx, name, reverse, monkeypatch)
    rows_h = ps.apply_edits(name, rows_h, run_off, reverse)
    cig_h = cig.cpu().numpy().view(np.uint32)
    # what the device packed is what the CPU test reasoned about (word 10, the key word, exists only here).  Under clip the device
    # packs a group whose clipped alignment is a single M or M N M from its key, without the soft clips (partial_rows_k, shard.hip:
    # "soft clips do not travel then"): the CIGAR words and their count in word 2 may differ there, nothing else
    prow, pro, pcig = ps.packed(name, reverse)
    assert np.array_equal(run_off, pro)
    a, b = rows_h[:, :10].copy(), prow[:, :10].copy()
    if sc.strategy == "clip":
        a[:, 2] &= 0xFF
        b[:, 2] &= 0xFF
    else:
        assert np.array_equal(cig_h, pcig)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert not len(bad), "rows %s: device %s, host %s" % (bad.tolist(), a[bad].tolist(), b[bad].tolist())
    assert not rows_h[:, 11].any()
    rows = torch.from_numpy(np.ascontiguousarray(rows_h)).to("cuda:0")
    try:
        got = ctx.partial_reduce(rows, run_off, cig, strategy=sc.strategy)
    except TbkError as e:
        return e.status, None, None, rows_h, run_off, cig_h
    cov = api.to_numpy(ctx.coverage(got.pop("view"))) if got["n_groups"] else None      # (the view lives until the next call)
    return 0, api.to_numpy(got), cov, rows_h, run_off, cig_h


def check_scene(ctx, name, reverse, monkeypatch):
    from oracle import oracle_ffi as orc
    from tiebrush_amd import synth
    sc = ps.SCENES[name]
    status, got, cov, rows, run_off, cig = reduce_scene(ctx, name, reverse, monkeypatch)
    assert status == sc.expect, "status %d, expected %d" % (status, sc.expect)
    if status != 0:
        return
    t2, want = ps.expected(rows, run_off, cig, sc.strategy)      # the oracle on the rows as received
    cpu = ps.expected_of(name, reverse)[1]                        # ... is the result the CPU test proved the scene's claims on
    for k in ("n_groups", "rep", "yc", "yx", "yd", "g_start", "g_end"):
        assert np.array_equal(np.asarray(want[k]), np.asarray(cpu[k])), "oracle " + k
    assert got["n_groups"] == want["n_groups"]
    if not want["n_groups"]:
        return
    assert np.array_equal(np.asarray(got["rep"]).astype(np.int64), np.asarray(want["rep"]).astype(np.int64)), "rep"
    assert np.asarray(got["yc"]).dtype == np.float64
    for k in ("yc", "yx", "yd", "g_start", "g_end"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    if not sc.edits and sc.mask is None:       # the flat run over all records as one tile: same groups, sums and representative
        tile = ps.flat_tile(name, reverse)
        flat = orc.collapse(tile, strategy=STRAT[sc.strategy])
        assert got["n_groups"] == flat["n_groups"]
        for k in ("yc", "yx", "yd", "g_start", "g_end"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(flat[k])), "flat " + k
        rep, frep = np.asarray(got["rep"]).astype(np.int64), flat["rep"].astype(np.int64)
        fo = tile.file_of().astype(np.int64)
        assert np.array_equal(rows[rep, 4], fo[frep]) and np.array_equal(rows[rep, 5], frep - tile.file_off[fo[frep]].astype(np.int64))
    cw = orc.coverage(synth.collapsed_to_cov_input(t2, want))
    for k in COV_KEYS:
        assert np.array_equal(cov[k], cw[k]), k


ACCEPTED = [(n, rev) for n, s in ps.SCENES.items() if s.expect == 0 for rev in ((False, True) if s.reverse else (False,))]
REFUSED = [n for n, s in ps.SCENES.items() if s.expect != 0]


@pytest.mark.parametrize("name,reverse", ACCEPTED)
def test_scene_equals_oracle(ctx, name, reverse, monkeypatch):
    """n_groups, rep (the row index), yc, yx, yd, g_start, g_end and tiecov's tracks of the view against the oracle; scenes without row
    edits also against the flat collapse of all records; again with the ranks in reversed order (the groups and sums are the same, the
    representative follows (effective end, run))"""
    check_scene(ctx, name, reverse, monkeypatch)


@pytest.mark.parametrize("name", REFUSED)
def test_refusal_and_the_context_after_it(ctx, name, monkeypatch):
    """PR_CAP + 1 rows on one base and a YX sum of 2^32: TBK_E2BIG; 65 runs: TBK_EUNSUPPORTED; a hashed key word shared by two
    alignments, the odd one the group's last member: TBK_ECOLLISION — and the context reduces a good scene afterwards"""
    check_scene(ctx, name, False, monkeypatch)
    check_scene(ctx, "seam_257", False, monkeypatch)
    check_scene(ctx, "odd_last", False, monkeypatch)


class DeviceCompute:
    """tiles resident in HBM, results stay torch tensors; records what the owner's merge-reduce refused, and masks the hash word at the
    pack when asked to"""

    def __init__(self, monkeypatch, pack_mask=None):
        from tiebrush_amd import api
        self.ctx = api.Context(0)
        self.refused = []
        self.mp, self.pack_mask = monkeypatch, pack_mask

    def collapse(self, tile, **kw):
        return self.ctx.collapse(tile, **kw)

    def groups_to_cov_in(self, fin):
        return self.ctx.groups_to_cov_in(fin)

    def _packing(self, fn, *a, **k):
        if self.pack_mask is None:
            return fn(*a, **k)
        tbk_debug(self.mp, hash_mask=self.pack_mask)
        try:
            return fn(*a, **k)
        finally:
            tbk_debug(self.mp, hash_mask=None)

    def partial_pack(self, *a, **k):
        return self._packing(self.ctx.partial_pack, *a, **k)

    def partial_stage_pack(self, *a, **k):
        return self._packing(self.ctx.partial_stage_pack, *a, **k)

    def partial_reduce(self, *a, **k):
        from tiebrush_amd._lib import TbkError
        try:
            return self.ctx.partial_reduce(*a, **k)
        except TbkError as e:
            self.refused.append(e.status)
            raise

    def __getattr__(self, name):          # tbk_shard_* / tbk_partial_*
        if name.startswith("shard_") or name.startswith("partial_"):
            return getattr(self.ctx, name)
        raise AttributeError(name)

    def finish_yd(self):
        self.ctx.finish_yd()

    def coverage(self, view):
        from tiebrush_amd import api
        return api.to_numpy(self.ctx.coverage(view))


@pytest.mark.parametrize("name", ps.LOOPBACK)
def test_driver_gives_the_flat_result(name, monkeypatch):
    """the multi-rank driver on a pile-up the merge-reduce refuses (TBK_E2BIG), on a shared hashed key word (TBK_ECOLLISION) and on a
    heavy window it takes: one virtual rank per run, the result of the flat oracle run either way — through the general path after a
    refusal"""
    import torch
    from oracle import oracle_ffi as orc
    from tiebrush_amd import api, dist, synth
    sc = ps.SCENES[name]
    assert not sc.edits
    tile = ps.flat_tile(name)
    flat = orc.collapse(tile, strategy=STRAT[sc.strategy])
    flat_cov = orc.coverage(synth.collapsed_to_cov_input(tile, flat))
    tiles, first = ps.tiles_of(name)
    comp = DeviceCompute(monkeypatch, sc.mask)
    res = dist.run_loopback(comp, [api.to_device(t, "cuda:0") for t in tiles], first, strategy=sc.strategy, want_coverage=True,
                            device_chain=True)
    for r in res:
        for f in ("tid", "start", "end", "rep_fidx", "rep_idx", "yc", "yx", "yd"):
            v = getattr(r, f)
            setattr(r, f, v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
    check_against_flat(res, tile, flat, flat_cov)
    assert comp.refused == ([sc.expect] if sc.expect else [])
    comp.ctx.close()
