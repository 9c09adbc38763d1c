"""`tiebrush -r REGION`: one locus of indexed inputs collapsed on the device.  The contract: the output is what the same
command line without -r makes of inputs in which every file is replaced by its records that overlap the region.  The expected values
never come from the code under test: the inputs are parsed by tiebrush_amd.bamio / soa.tile_from_bams, filtered in numpy by the overlap
rule restated here, and collapsed by the oracle (oracle_ffi.collapse, tb_cpu_e2e on filtered files written with bamio.write_bam).
Every test fails on a build without the feature: tbk_bam_decode_file_spans / tbk_tile_region are missing, -r is an unknown option."""
import os
import subprocess

import numpy as np
import pytest

import bai_reader as br
import csi_reader as cr
import region_fixtures as rf
from helpers import GOLDEN, sample_paths, read_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = rf.BIN
CPU_E2E = os.path.join(ROOT, "oracle", "_build", "tb_cpu_e2e")
W = rf.W
REF_OPS = (0, 2, 3, 7, 8)                                           # M D N = X consume the reference


# ---- the contract restated in numpy ---------------------------------------------------------------------------------------------------
def overlap_mask(t, tid, beg, end):
    """record i is the region's when tid[i] == tid, pos < end and rec_end > beg, rec_end = pos + the reference length of its CIGAR over
    M D N = X, or pos + 1 when that length is 0"""
    n = t.n_records
    w = np.where(np.isin(t.cig & 15, REF_OPS), t.cig >> 4, 0).astype(np.int64)
    rec = np.repeat(np.arange(n), np.diff(t.cig_off.astype(np.int64)))
    rl = np.bincount(rec, weights=w, minlength=n).astype(np.int64)
    pos = t.pos.astype(np.int64)
    return (t.tid == tid) & (pos < end) & (pos + np.where(rl > 0, rl, 1) > beg)


def _csr_select(off, payload, mask):
    lens = np.diff(off.astype(np.int64))[mask]
    new = np.zeros(len(lens) + 1, dtype=np.uint32)
    new[1:] = np.cumsum(lens)
    src = np.repeat(off[:-1].astype(np.int64)[mask] - new[:-1].astype(np.int64), lens) + np.arange(int(new[-1]))
    return new, payload[src]


def select(t, mask):
    """the tile of the records under mask, file order kept"""
    from tiebrush_amd import soa
    fo = np.concatenate([[0], np.cumsum(mask)])[t.file_off.astype(np.int64)].astype(np.uint32)
    co, cg = _csr_select(t.cig_off, t.cig, mask)
    o = soa.SoATile(n_files=t.n_files, file_off=fo, tbmerged=t.tbmerged, tid=t.tid[mask], pos=t.pos[mask], flag=t.flag[mask], mapq=t.mapq[mask],
                    strand=t.strand[mask], nh=t.nh[mask], cig_off=co, cig=cg)
    if t.yc_in is not None:
        o.yc_in, o.yx_in, o.yd_in = t.yc_in[mask], t.yx_in[mask], t.yd_in[mask]
    if t.md_off is not None:
        o.md_off, o.md = _csr_select(t.md_off, t.md, mask)
        o.md_has = t.md_has[mask]
    if t.qn_off is not None:
        o.qn_off, o.qn = _csr_select(t.qn_off, t.qn, mask)
        o.qname_hash = t.qname_hash[mask] if t.qname_hash is not None else None
    return o


class Inputs:
    """input files parsed once by bamio: .fx (region_fixtures.Fixture each), .bams, .tile (names and MD included)"""

    def __init__(self, paths, hashes=True):
        from tiebrush_amd import bamio
        self.fx = [rf.Fixture(p) for p in paths]
        self.bams = [bamio.read_bam(p, keep_md=True) for p in paths]
        self.hashes = hashes
        self._sub = {}
        self.tile = self.sub(range(len(paths)))
        self.n_ref = len(self.fx[0].lens)

    def sub(self, order):
        """the tile of the files `order`, names and MD included (qname_hash only with `hashes`: the oracle compares the names)"""
        from tiebrush_amd import soa
        key = tuple(order)
        if key not in self._sub:
            bams = [self.bams[f] for f in key]
            t = soa.tile_from_bams(bams, with_names=self.hashes, with_md=True)
            if not self.hashes:
                names = [q for b in bams for q in b.qname]
                t.qn_off = np.zeros(len(names) + 1, dtype=np.uint32)
                t.qn_off[1:] = np.cumsum(np.fromiter((len(q) for q in names), dtype=np.int64, count=len(names)))
                t.qn = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
            self._sub[key] = t
        return self._sub[key]

    def raw_records(self, idx):
        """the framed records (block_size first) behind tile indices, back to back"""
        import struct
        fo = self.tile.file_of()
        out = []
        for i in idx:
            b = self.bams[int(fo[i])]
            o = int(b.rec_off[int(i) - int(self.tile.file_off[int(fo[i])])])
            out.append(bytes(b.raw[o:o + 4 + struct.unpack_from("<I", b.raw, o)[0]]))
        return b"".join(out)


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _subset_files(d, tag, aligned):
    """four synthetic inputs that cover different ranges: everything; every other record; the first reference up to window 31; the last
    reference only (for most regions: a file without a chunk)"""
    recs = br.synthetic_records()
    allr = br.read_bam(cr.write_bam(str(d / "tmp.bam"), br.SYN_NAMES, br.SYN_LENS, recs))[2]
    parts = [recs, recs[::2], [r for r, m in zip(recs, allr) if m[0] == 0 and m[1] < 31 * W], [r for r, m in zip(recs, allr) if m[0] == 2]]
    return [rf.write_syn(str(d / ("%s%d.bam" % (tag, i))), br.SYN_NAMES, br.SYN_LENS, p, aligned) for i, p in enumerate(parts)]


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb_region_syn")
    return {al: Inputs(_subset_files(d, "syn%d_" % al, al)) for al in (0, 1)}


@pytest.fixture(scope="module")
def merged(tmp_path_factory):
    """t1.bam and t2.bam are TieBrush outputs (YC / YX / YD, MD, names); t2s0.bam between them is a plain input"""
    d = tmp_path_factory.mktemp("tb_region_merged")
    return Inputs([rf.golden_copy(d, "t1/t1.bam"), rf.golden_copy(d, "t2/t2s0.bam"), rf.golden_copy(d, "t2/t2.bam")])


COLS = ("tid", "pos", "flag", "mapq", "strand", "nh", "cig_off", "cig")


def _region_tile(ctx, inp, order, kind, region, want_md=False, want_names=False):
    """the library's region tile of the inputs `order` (indices into inp) -> (decoded records, out struct, file_off, numpy columns)"""
    from tiebrush_amd import api
    tid, beg, end = region
    fspans = []
    for f in order:
        fx = inp.fx[f]
        fspans.append(fx.spans(api.index_query(fx.path, tid, beg, end, fx.indexes[kind])) if beg < end else [])
    tb = np.array([inp.tile.tbmerged[f] for f in order], dtype=np.uint8)
    tile, fo = ctx.bam_decode_file_spans(fspans, inp.n_ref, tb, want_md, want_names)
    decoded = int(tile.n_records)
    assert int(fo[-1]) == decoded and int(tile.n_files) == len(order)
    out, fo2 = ctx.tile_region(tile, tid, beg, end)
    fields = list(COLS)
    if out.yc_in:
        fields += ["yc_in", "yx_in", "yd_in"]
    if out.md_off:
        fields += ["md_off", "md_has"]
    if out.qname_off:
        fields += ["qname_off", "qname_hash"]
    got = ctx.soa_to_numpy(out, fields=tuple(fields)) if int(out.n_records) else {}
    return decoded, out, fo2, got


def _want_tile(inp, order, region):
    """the numpy filter of the parsed files `order` -> (filtered tile, tile indices of the kept records in inp.tile)"""
    sub = inp.sub(order)
    m = overlap_mask(sub, *region)
    base = np.concatenate([np.arange(int(inp.tile.file_off[f]), int(inp.tile.file_off[f + 1])) for f in order]) if order else np.zeros(0, int)
    return select(sub, m), base[m]


def _assert_tile(got, out, fo, want, what, md=False, names=False):
    assert int(out.n_records) == want.n_records, what
    assert list(fo) == list(want.file_off), what                      # per file
    if want.n_records == 0:
        return
    assert int(out.n_cigar_ops) == len(want.cig), what
    for k in COLS:
        assert np.array_equal(got[k], getattr(want, k)), (what, k)
    if want.tbmerged.any():
        for k in ("yc_in", "yx_in", "yd_in"):
            tbrec = want.tbmerged[want.file_of()] != 0                # (the carried tags are read only for records of merged files)
            assert np.array_equal(got[k][tbrec], getattr(want, k)[tbrec]), (what, k)
    else:
        assert not out.yc_in and not out.yx_in and not out.yd_in, what
    if md:
        assert np.array_equal(got["md_off"], want.md_off) and np.array_equal(got["md_has"], want.md_has) and np.array_equal(got["md"], want.md), what
    else:
        assert not out.md_off and not out.md and not out.md_has, what
    if names:
        assert np.array_equal(got["qname_off"], want.qn_off) and np.array_equal(got["qname"], want.qn), what
        assert np.array_equal(got["qname_hash"], want.qname_hash), what
    else:
        assert not out.qname_off and not out.qname and not out.qname_hash, what


def _check(ctx, inp, order, kind, region, md=False, names=False, records=False):
    decoded, out, fo, got = _region_tile(ctx, inp, order, kind, region, md, names)
    want, idx = _want_tile(inp, order, region)
    _assert_tile(got, out, fo, want, (order, kind, region), md, names)
    if records and want.n_records:
        blob, off = ctx.bam_records(np.arange(want.n_records))
        assert blob == inp.raw_records(idx), (order, kind, region)
        pick = np.array([want.n_records - 1, 0, want.n_records // 2])
        blob, off = ctx.bam_records(pick)
        assert blob == inp.raw_records(idx[pick])
    return decoded, want.n_records


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bai", "csi"])
@pytest.mark.parametrize("al", [0, 1])
def test_region_tile_equals_the_numpy_filter(ctx, syn, al, kind):
    """the hand-picked edges (a record ending at beg / starting at end: out; the reference-length-0 record: in) and 20 random regions, on
    four files through both index kinds, members that records straddle (0) and record-aligned members (1)"""
    inp = syn[al]
    filtered = 0
    for k, region in enumerate(rf.syn_regions() + rf.random_regions(inp.fx[0], 5 + al, 20)):
        decoded, kept = _check(ctx, inp, [0, 1, 2, 3], kind, region, records=k % 7 == 0)
        filtered += kept < decoded
    assert filtered > 10                                              # the filter is exercised, not merely the index


def test_the_edges_are_in_the_regions(ctx, syn):
    """what the edge regions are there for, told from the parsed files alone, and the library's tile of each of them: a record ending
    exactly at beg and one starting at end are out, the record of reference length 0 at beg is in, one base further it is out"""
    inp = syn[1]
    iso = 50 * W - 20
    t = inp.tile
    zero = overlap_mask(t, 0, 60 * W + 5, 60 * W + 6)
    assert zero.sum() >= 1 and all(int(c) & 15 in (1, 4) for i in np.flatnonzero(zero) for c in t.cig[t.cig_off[i]:t.cig_off[i + 1]])
    for region, some in (((0, iso, iso + 50), True), ((0, iso + 50, iso + 120), False), ((0, iso - 100, iso), False),
                         ((0, 60 * W + 5, 60 * W + 6), True), ((0, 60 * W + 6, 60 * W + 7), False)):
        n = int(overlap_mask(t, *region).sum())
        assert (n >= 1) == some, region
        for kind in ("bai", "csi"):
            decoded, kept = _check(ctx, inp, [0, 1, 2, 3], kind, region)
            assert kept == n and decoded >= kept, (region, kind)


@pytest.mark.parametrize("order", [[3, 0, 1], [0, 3, 1], [0, 1, 3], [3, 3, 3], [3]])
def test_files_without_a_chunk(ctx, syn, order):
    """file 3 holds the last reference only: first, in the middle, last, and every file without a chunk"""
    from tiebrush_amd import api
    inp = syn[1]
    region = (0, 30 * W + 500, 30 * W + 5003)
    assert api.index_query(inp.fx[3].path, *region, inp.fx[3].indexes["bai"]) == []
    decoded, kept = _check(ctx, inp, order, "bai", region, records=True)
    assert (kept == 0) == (order.count(3) == len(order)) and (decoded == 0) == (kept == 0)
    _check(ctx, inp, order, "csi", (1, 0, 100000))                    # chrEmpty: no file has a chunk


def test_nothing_kept_and_everything_kept(ctx, syn):
    inp = syn[1]
    decoded, kept = _check(ctx, inp, [0, 1, 2], "bai", (0, 50 * W + 30, 50 * W + 100))    # chunks decoded, no record overlaps
    assert decoded > 0 and kept == 0
    blob, off = ctx.bam_records(np.zeros(0, np.uint32))
    assert blob == b""
    decoded, kept = _check(ctx, inp, [3, 3], "bai", (2, 0, 1000000), records=True)       # files of one record each, on their own reference
    assert decoded == kept == 2


def _count_files(d, tag, counts, pad):
    """files of counts[f] records inside (0, 1000, 2000) each, and beside them in the same members: `pad` records before the region, one that
    ends exactly at beg, one that starts at end — none of them the region's"""
    from tiebrush_amd import bamio
    paths = []
    for f, c in enumerate(counts):
        rows = sorted((100 + i % 50, 30) for i in range(pad)) + [(970, 30)] + [(1000 + (i * 950) // max(c, 1), 40) for i in range(c)] + [(2000, 30)]
        recs = [bamio.encode_record(0, p, 0, 60, [l << 4], b"c%d_%d" % (f, i), aux=b"NHC\x01") for i, (p, l) in enumerate(rows)]
        paths.append(str(d / ("%s_%d.bam" % (tag, f))))
        cr.write_bam(paths[-1], ["chrC"], [100000], recs)
    return Inputs(paths)


@pytest.mark.parametrize("counts", [(0, 1, 0), (100, 155, 0), (256, 0, 0), (1, 255, 1)], ids=["1", "255", "256", "257"])
def test_kept_counts_at_wave_and_block_edges(ctx, tmp_path, counts):
    inp = _count_files(tmp_path, "k", counts, pad=3)
    decoded, kept = _check(ctx, inp, [0, 1, 2], "bai", (0, 1000, 2000), names=True, records=True)
    assert kept == sum(counts) and decoded == kept + 5 * 3


@pytest.mark.parametrize("n", [16382, 16383, 16384, 16385])
def test_tile_lengths_around_the_scan_tile(ctx, tmp_path, n):
    """the scans run over n + 1 elements: 16384 is the last length the one-block scan takes, 16385 = 8 * 2048 + 1 the first of the tiled
    scan and one element into its ninth tile"""
    a = 9000
    inp = _count_files(tmp_path, "s", (a - 2 - 7, n - a - 2 - 7), pad=7)
    decoded, kept = _check(ctx, inp, [0, 1], "csi", (0, 1000, 2000), records=False)
    assert decoded == n and kept == n - 18


@pytest.mark.parametrize("kind", ["bai", "csi"])
def test_merged_inputs_carry_yd_md_and_names(ctx, merged, kind):
    """t1.bam + t2.bam are flagged tbmerged: yc / yx / yd_in come through, with the MD and QNAME CSRs and qname_hash; the plain file between
    them reads none of its tags"""
    inp = merged
    assert list(inp.tile.tbmerged) == [1, 0, 1]
    t = inp.fx[2].recs[len(inp.fx[2].recs) // 3]
    regions = [(t[0], max(0, t[1] - 3000), t[1] + 3000), (t[0], 0, inp.fx[2].lens[t[0]]), (57, 0, inp.fx[2].lens[57])] + rf.random_regions(inp.fx[2], 9, 6)
    yd_seen = 0
    for k, region in enumerate(regions):
        decoded, out, fo, got = _region_tile(ctx, inp, [0, 1, 2], kind, region, True, True)
        want, idx = _want_tile(inp, [0, 1, 2], region)
        if want.n_records:
            yd_seen += int((want.yd_in > 0).sum())
        _assert_tile(got, out, fo, want, (kind, region), md=True, names=True)
        if k < 2 and want.n_records:
            blob, _ = ctx.bam_records(np.arange(want.n_records))
            assert blob == inp.raw_records(idx)
    assert yd_seen > 0
    decoded, out, fo, got = _region_tile(ctx, inp, [1], kind, regions[0], False, False)   # no merged file, no MD, no names: the columns stay NULL
    _assert_tile(got, out, fo, _want_tile(inp, [1], regions[0])[0], "plain")


@pytest.mark.parametrize("flags,okw", [([], {}), (["L"], dict(strategy=1)), (["A"], dict(collapse_same=True))])
def test_collapse_of_the_region_tile_equals_the_oracle_on_the_filtered_tile(ctx, merged, flags, okw):
    from oracle import oracle_ffi as orc
    inp = merged
    t = inp.fx[2].recs[len(inp.fx[2].recs) // 3]
    region = (t[0], max(0, t[1] - 3000), t[1] + 3000)
    decoded, out, fo, _ = _region_tile(ctx, inp, [0, 1, 2], "bai", region, "L" in flags, "A" in flags)
    want_tile, _ = _want_tile(inp, [0, 1, 2], region)
    assert 0 < want_tile.n_records < decoded
    want = orc.collapse(want_tile, **okw)
    from tiebrush_amd import api
    got = api.to_numpy(ctx.collapse_struct(out, 3, **okw))
    assert got["n_groups"] == want["n_groups"] and got["n_passed"] == want["n_passed"]
    for k in ("rep", "yc", "yx", "yd"):
        assert np.array_equal(np.asarray(got[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), k
    blob, _ = ctx.bam_records(np.asarray(got["rep"]).astype(np.uint32))                   # the writers' fetch, by compacted index
    sub_idx = _want_tile(inp, [0, 1, 2], region)[1]
    assert blob == inp.raw_records(sub_idx[np.asarray(want["rep"]).astype(int)])


def test_a_foreign_or_joined_tile_is_refused_and_the_context_goes_on(ctx, syn):
    from tiebrush_amd import api, _lib
    inp = syn[1]
    region = (0, 30 * W + 500, 30 * W + 5003)
    other = api.Context(0)
    try:
        fx = inp.fx[0]
        spans = fx.spans(api.index_query(fx.path, *region, fx.indexes["bai"]))
        theirs, _ = other.bam_decode_file_spans([spans], inp.n_ref)
        mine, _ = ctx.bam_decode_file_spans([spans], inp.n_ref)
        with pytest.raises(_lib.TbkError) as e:                        # another context's tile
            ctx.tile_region(theirs, *region)
        assert e.value.status == -1
        whole, _ = ctx.bam_decode([open(inp.fx[3].path, "rb").read()])
        host = select(inp.tile, np.arange(inp.tile.n_records) < 5)
        host.qn_off = host.qn = host.qname_hash = host.md_off = host.md = host.md_has = None
        joined, _ = ctx.tile_join(whole, host)
        with pytest.raises(_lib.TbkError) as e:                        # a joined tile
            ctx.tile_region(joined, 2, 0, 1000000)
        assert e.value.status == -1
        out, fo = ctx.tile_region(whole, 2, 0, 1000000)                # ... and the decoded tile itself is still taken
        assert int(out.n_records) == 1 and list(fo) == [0, 1]
    finally:
        other.close()
    _check(ctx, inp, [0, 1, 2, 3], "bai", region, records=True)        # the context takes the next call


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _tiebrush(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(BIN, "tiebrush")] + [str(a) for a in args], capture_output=True, text=True, env=e)


def _linked(d, inp, kind, tag):
    """the inputs under new names with the index of one kind only beside each"""
    out = []
    for i, fx in enumerate(inp.fx):
        p = str(d / ("%s%d.bam" % (tag, i)))
        if not os.path.exists(p):
            os.symlink(fx.path, p)
            os.symlink(fx.indexes[kind], p + "." + kind)
        out.append(p)
    return out


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb_region_t1s")
    return Inputs([rf.golden_copy(d, "t1/t1s%d.bam" % i) for i in range(10)], hashes=False)


@pytest.fixture(scope="module")
def recollapse(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb_region_t12")
    return Inputs([rf.golden_copy(d, "t1/t1.bam"), rf.golden_copy(d, "t2/t2.bam")], hashes=False)


OPTION_SETS = [([], {}), (["-L"], dict(strategy=1)), (["-P"], dict(strategy=2)), (["-E"], dict(strategy=3)), (["-A"], dict(collapse_same=True)),
               (["--keep-secondary", "-S", "--store-frac"], dict(keep_secondary=True, keep_supplementary=True, store_frac=True)),
               (["-N", "5", "-Q", "1"], dict(max_nh=5, min_qual=1))]


def _region_text(inp, region, commas=False):
    tid, beg, end = region
    return "%s:%s-%d" % (inp.fx[0].names[tid], format(beg + 1, ",") if commas else str(beg + 1), end)


def _assert_output(inp, region, okw, out_path, stderr):
    """the record stream and YC / YX / YD of out_path equal the oracle's collapse of the filtered inputs"""
    from oracle import oracle_ffi as orc
    from tiebrush_amd import bamio
    m = overlap_mask(inp.tile, *region)
    idx = np.flatnonzero(m)
    want = orc.collapse(select(inp.tile, m), **okw)
    o = bamio.read_bam(out_path)
    assert o.n == want["n_groups"]
    assert "%d input records written as %d" % (want["n_passed"], want["n_groups"]) in stderr
    fo = inp.tile.file_of()
    for g in range(o.n):
        gi = int(idx[int(want["rep"][g])])
        f = int(fo[gi])
        i = gi - int(inp.tile.file_off[f])
        assert bamio.record_identity(o, g) == bamio.record_identity(inp.bams[f], i), g
        assert o.yx[g] == want["yx"][g] and o.yd[g] == want["yd"][g], g
        if not inp.bams[f].has_yc[i]:       # (a carried integer YC is not replaced by the float update: test_tiebrush_cli_recollapse_and_listfile)
            assert o.has_yc[g] and np.float32(o.yc[g]) == np.float32(want["yc"][g]), g
    return o.n, int(m.sum())


def _locus(inp):
    r = inp.fx[0].recs[len(inp.fx[0].recs) // 2]
    return (r[0], r[1] - 150, r[1] + 150)


@pytest.mark.parametrize("flags,okw", OPTION_SETS, ids=["default", "L", "P", "E", "A", "secondary_frac", "N5_Q1"])
def test_cli_locus_of_ten_inputs(samples, tmp_path, flags, okw):
    """a locus inside the ten samples' 8 kb: --writer device through the .bai, --writer host through the .csi"""
    region = _locus(samples)
    for writer, kind, opt in (("device", "bai", "-r"), ("host", "csi", "--region")):
        paths = _linked(tmp_path, samples, kind, kind)
        out = str(tmp_path / (writer + ".bam"))
        r = _tiebrush([opt, _region_text(samples, region, commas=writer == "host"), "--writer", writer, "-o", out] + flags + paths, env=dict(TBK_TIMING="1"))
        assert r.returncode == 0, r.stderr
        n_out, n_in = _assert_output(samples, region, okw, out, r.stderr)
        assert 0 < n_out and 0 < n_in < samples.tile.n_records // 4
        assert "region path ms: index queries" in r.stderr and "chunks of 10 inputs" in r.stderr


def test_cli_whole_reference_and_empty_region(samples, tmp_path):
    paths = _linked(tmp_path, samples, "bai", "w")
    out = str(tmp_path / "whole.bam")
    r = _tiebrush(["-r", "chr12", "-o", out] + paths)
    assert r.returncode == 0, r.stderr
    n_out, n_in = _assert_output(samples, (4, 0, samples.fx[0].lens[4]), {}, out, r.stderr)
    assert n_in == int((samples.tile.tid == 4).sum()) > samples.tile.n_records - 1000      # (a few records lie on another reference)
    for writer in ("device", "host"):
        out = str(tmp_path / ("empty_%s.bam" % writer))
        r = _tiebrush(["-r", "chr1:1000-2000", "--writer", writer, "--index", "-o", out] + paths)
        assert r.returncode == 0, r.stderr
        assert "0 input records written as 0 (0.00% reduction)" in r.stderr and "nan" not in r.stderr
        data = open(out, "rb").read()
        names, lens, recs, _ = br.read_bam(data)                      # a valid BAM: header + EOF member
        assert recs == [] and names == samples.fx[0].names and data.endswith(cr.EOF_MEMBER)
        assert open(out + ".bai", "rb").read() == br.expected_bai(data)


@pytest.mark.parametrize("flags,okw", [OPTION_SETS[i] for i in (0, 1, 4, 5, 6)], ids=["default", "L", "A", "secondary_frac", "N5_Q1"])
def test_cli_merged_inputs(recollapse, tmp_path, flags, okw):
    """t1.bam t2.bam are TieBrush outputs: their YC / YX / YD are carried into the region's groups"""
    inp = recollapse
    t = inp.fx[1].recs[len(inp.fx[1].recs) // 3]
    for k, (region, writer, kind) in enumerate([((t[0], max(0, t[1] - 2000), t[1] + 2000), "device", "csi"), ((57, 0, inp.fx[1].lens[57]), "host", "bai")]):
        paths = _linked(tmp_path, inp, kind, kind)
        out = str(tmp_path / ("m%d.bam" % k))
        r = _tiebrush(["-r", _region_text(inp, region), "--writer", writer, "-o", out] + flags + paths)
        assert r.returncode == 0, r.stderr
        n_out, n_in = _assert_output(inp, region, okw, out, r.stderr)
        assert 0 < n_out <= n_in < inp.tile.n_records


def test_cli_merged_inputs_equal_the_cpu_tool_on_filtered_files(recollapse, tmp_path):
    """whole files: every input replaced by its records that overlap the region (bamio.write_bam under its own header), run through
    tb_cpu_e2e — records and all three tags, the carried YC text included"""
    from tiebrush_amd import bamio
    inp = recollapse
    t = inp.fx[1].recs[len(inp.fx[1].recs) // 3]
    region = (t[0], max(0, t[1] - 2000), t[1] + 2000)
    m = overlap_mask(inp.tile, *region)
    filt = []
    for f, b in enumerate(inp.bams):
        keep = np.flatnonzero(m[int(inp.tile.file_off[f]):int(inp.tile.file_off[f + 1])])
        raw = inp.raw_records(keep + int(inp.tile.file_off[f]))
        filt.append(str(tmp_path / ("f%d.bam" % f)))
        bamio.write_bam(filt[-1], b.header.text, inp.fx[f].names, inp.fx[f].lens, raw)
    ref = str(tmp_path / "ref.bam")
    subprocess.run([CPU_E2E, "-o", ref] + filt, check=True, capture_output=True)
    out = str(tmp_path / "o.bam")
    r = _tiebrush(["-r", _region_text(inp, region), "-o", out] + _linked(tmp_path, inp, "bai", "e"))
    assert r.returncode == 0, r.stderr
    o, g = bamio.read_bam(out), bamio.read_bam(ref)
    assert o.n == g.n > 0
    for i in range(g.n):
        assert bamio.record_identity(o, i) == bamio.record_identity(g, i), i
        assert o.has_yc[i] == g.has_yc[i] and o.yc[i] == g.yc[i] and o.yx[i] == g.yx[i] and o.yd[i] == g.yd[i], i


def test_cli_index_and_tracks_are_those_of_the_output(samples, tmp_path):
    """--index: OUT.bam.bai is bai_reader's index of OUT.bam and tiecov -r runs on it; --cov --junc --samp: tiecov -c -j -s OUT.bam's files"""
    region = _locus(samples)
    paths = _linked(tmp_path, samples, "csi", "i")
    out = str(tmp_path / "o.bam")
    pre = str(tmp_path / "t")
    r = _tiebrush(["-r", _region_text(samples, region), "--index", "--cov", pre + ".c", "--junc", pre + ".j", "--samp", pre + ".s", "-o", out] + paths)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    bai = open(out + ".bai", "rb").read()
    assert bai == br.expected_bai(data)
    br.validate(data, bai)
    ref = str(tmp_path / "ref")
    tc = os.path.join(BIN, "tiecov")
    subprocess.run([tc, "-c", ref + ".c", "-j", ref + ".j", "-s", ref + ".s", out], check=True, capture_output=True)
    for ext in (".c.bedgraph", ".j.bed", ".s.bedgraph"):
        assert open(pre + ext, "rb").read() == open(ref + ext, "rb").read(), ext      # the tracks of OUT.bam, not clipped
    assert len(read_lines(pre + ".c.bedgraph")) > 2
    sub = str(tmp_path / "sub")
    r2 = subprocess.run([tc, "-r", _region_text(samples, (region[0], region[1] + 100, region[1] + 140)), "-c", sub, out], capture_output=True, text=True)
    assert r2.returncode == 0 and len(read_lines(sub + ".bedgraph")) > 1, r2.stderr
    out2 = str(tmp_path / "o2.bam")
    r = _tiebrush(["-r", _region_text(samples, region), "--csi", "--writer", "host", "-o", out2] + paths)
    assert r.returncode == 0 and os.path.exists(out2 + ".csi"), r.stderr


def test_without_region_nothing_changes(tmp_path):
    """the default route on a golden case never enters the region code (its phase line is absent) and writes the golden records and tags.
    The comparison with the golden file is by record identity and tags, not by bytes: the golden file was written by the reference
    program, and the header's @PG line carries the program, its version and the command line, so no two programs' files are equal
    byte for byte.  The byte-for-byte comparison that can be made is made: the same command line run again, which does not enter the
    region code either, writes the same file.  The existing suite is the real check that the routes without -r are unchanged."""
    from tiebrush_amd import bamio
    out = str(tmp_path / "o.bam")
    r = _tiebrush(["-A", "-o", out] + sample_paths("t2"), env=dict(TBK_TIMING="1"))
    assert r.returncode == 0 and "region path" not in r.stderr and "242910 input records written as 8179" in r.stderr, r.stderr
    first = open(out, "rb").read()
    o, g = bamio.read_bam(out), bamio.read_bam(os.path.join(GOLDEN, "t2", "t2.bam"))
    assert o.n == g.n
    for i in range(g.n):
        assert bamio.record_identity(o, i) == bamio.record_identity(g, i), i
        assert o.yc[i] == (g.yc[i] if g.has_yc[i] else 1.0) and o.yx[i] == g.yx[i] and o.yd[i] == g.yd[i], i
    r = _tiebrush(["-A", "-o", out] + sample_paths("t2"))
    assert r.returncode == 0 and open(out, "rb").read() == first
    r = _tiebrush(["-o", out] + sample_paths("t2")[:1] + ["-r"])        # (-r takes a value)
    assert r.returncode == 1 and "value required" in r.stderr
