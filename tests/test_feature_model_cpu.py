"""CPU side of `--features BED --summary OUT`: the two forms of the model agree on every scene and prove the scenes'
claims; the BED feature parser of libtbh; `tbh_tool summary` (the host summariser and the TSV writer) on the golden tracks."""
import os
from fractions import Fraction

import numpy as np
import pytest

import feature_model as fm
import feature_scenes as fs
import region_fixtures as rf
from helpers import GOLDEN


@pytest.mark.parametrize("name", sorted(fs.SCENES))
def test_model_forms_agree_and_prove_the_claims(name):
    rows, feats, claims = fs.SCENES[name]()
    n = len(feats["tid"])
    assert n == len(claims) and n >= 1
    # the rows are what the entry takes: sorted by (tid, start) and disjoint; junction rows sorted by (tid, start, end, strand)
    t, s, e = rows["iv_tid"].astype(np.int64), rows["iv_start"].astype(np.int64), rows["iv_end"].astype(np.int64)
    assert np.all(e > s) and np.all((t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (s[1:] >= e[:-1])))
    jk = list(zip(rows["j_tid"].tolist(), rows["j_start"].tolist(), rows["j_end"].tolist(), rows["j_strand"].tolist()))
    assert jk == sorted(jk) and len(set(jk)) == len(jk)
    a = fm.mark_dyadic(rows, fm.per_row(rows, feats))
    b = fm.per_base(rows, feats)
    for k in range(n):
        if b[k] is not None:
            assert b[k]["covered"] == a[k]["covered"] and b[k]["max"] == a[k]["max"], k
            assert b[k]["sum"] == float(a[k]["S"]), k            # both are the exact sum rounded once
        for key, want in claims[k].items():
            got = a[k]["S"] if key == "sum" else a[k][key]
            assert got == (Fraction(want) if key == "sum" else want), (name, k, key, got, want)
    if name == "thirds":
        assert not any(fm.exact(m) for m in a if m["m"])
    elif name == "top":
        assert not fm.exact(a[0]) and fm.exact(a[2])
    else:
        assert all(fm.exact(m) for m in a)


def test_the_scenes_cover_both_paths_and_every_tile_count():
    _, _, claims = fs.runs()
    assert {c["path"] for c in claims} == {"direct", "agg"}
    assert {c["tiles"] for c in claims if c["path"] == "agg"} >= {0, 1, 2, 3}
    assert {c["hi"] - c["lo"] for c in claims} >= {63, 64, 65, fs.D - 1, fs.D, fs.D + 1}
    assert any(c["lo"] % fs.T == 0 for c in claims if c["path"] == "agg") and any(c["hi"] % fs.T == 0 for c in claims if c["path"] == "agg")
    for n in fs.LIST_N:
        rows, feats, _ = fs.feature_list(n)
        assert len(feats["tid"]) == n
        if n >= 64:
            m = fm.per_row(rows, feats)
            assert {x["path"] for x in m} == {"direct", "agg"}
            keys = list(zip(feats["beg"].tolist(), feats["end"].tolist()))
            assert len(set(keys)) < n and keys != sorted(keys)                                  # duplicates, not in order
            assert any(a[0] < b[0] and b[1] < a[1] for a in keys[:40] for b in keys[:40])       # nested


def test_random_case_meets_its_conditions():
    rows, feats = fs.random_case()
    assert len(rows["iv_tid"]) <= 4000 and len(feats["tid"]) <= 2000
    m = fm.mark_dyadic(rows, fm.per_row(rows, feats))
    n = len(m)
    assert 2 * sum(x["m"] > 0 for x in m) >= n and 10 * sum(x["path"] == "agg" for x in m) >= n
    assert all(fm.exact(x) for x in m) and sum(x["junc"] > 0 for x in m) > 50


# ---- the BED feature parser (tbh_features_from_bed) -----------------------------------------------------------------------------------
T2 = os.path.join(GOLDEN, "t2", "t2.bam")


def _header(bam_loader, path):
    h = bam_loader(path).header
    return list(h.ref_names), list(h.ref_lens)


def test_feature_parser_accepts(tmp_path, bam_loader):
    from tiebrush_amd import api
    names, lens = _header(bam_loader, T2)
    a, L = names[0], lens[0]
    bed = tmp_path / "f.bed"
    bed.write_text("# comment\ntrack name=x\nbrowser position\n\n"
                   "%s\t10\t20\n" % a +                                     # line 5: three columns
                   "%s 30 40 geneA\r\n" % a +                               # spaces, a name, CR
                   "%s\t30\t40\tgeneA\t0\t-\n" % a +                        # a duplicate interval, with a strand
                   "%s\t5\t%d\tlong\t900\t+\textra\n" % (a, L + 500) +      # cut to the reference; further columns ignored
                   "%s\t0\t1\t.\t0\t.\n" % names[-1] +                      # out of order
                   "%s\t12\t18\tnested" % a)                                # no newline at the end
    f = api.features_from_bed(T2, str(bed))
    assert f["line"].tolist() == [5, 6, 7, 8, 9, 10]
    assert f["tid"].tolist() == [0, 0, 0, 0, len(names) - 1, 0]
    assert f["beg"].tolist() == [10, 30, 30, 5, 0, 12] and f["end"].tolist() == [20, 40, 40, L, 1, 18]
    assert bytes(f["strand"]) == b"..-+.." and f["name"] == [".", "geneA", "geneA", "long", ".", "nested"]
    assert f["tid"].dtype == np.int32 and f["beg"].dtype == np.int64 and f["strand"].dtype == np.uint8
    many = tmp_path / "many.bed"                                            # more features and name bytes than the first buffers hold
    many.write_text("".join("%s\t%d\t%d\tfeature_number_%06d\n" % (a, i, i + 1, i) for i in range(300)))
    g = api.features_from_bed(T2, str(many))
    assert len(g["tid"]) == 300 and g["name"][299] == "feature_number_000299" and g["beg"].tolist() == list(range(300))


@pytest.mark.parametrize("line,msg", [("{a}\t10", "fewer than three"), ("{a}\tten\t20", "start"), ("{a}\t10\t-5", "end"), ("{a}\t20\t10", "start > end"),
                                      ("nochrom\t1\t2", "unknown reference"), ("{a}\t1\t2\tn\t0\t*", "strand"), ("{a}\t1\t2\tn\t0\t+-", "strand"),
                                      ("{a}\t7\t7", "empty"), ("{a}\t{L}\t{L1}", "empty")])
def test_feature_parser_refuses_with_the_line_number(tmp_path, bam_loader, line, msg):
    from tiebrush_amd import api
    names, lens = _header(bam_loader, T2)
    bed = tmp_path / "bad.bed"
    bed.write_text("#h\n%s\t1\t2\n" % names[0] + line.format(a=names[0], L=lens[0], L1=lens[0] + 10) + "\n%s\t3\t4\n" % names[0])
    with pytest.raises(RuntimeError) as e:
        api.features_from_bed(T2, str(bed))
    assert "bad.bed line 3" in str(e.value) and msg in str(e.value), str(e.value)


def test_feature_parser_refuses_a_file_without_features(tmp_path):
    from tiebrush_amd import api
    bed = tmp_path / "none.bed"
    bed.write_text("# nothing\n\ntrack x\n")
    with pytest.raises(RuntimeError, match="no feature"):
        api.features_from_bed(T2, str(bed))
    with pytest.raises(RuntimeError, match="cannot read"):
        api.features_from_bed(T2, str(tmp_path / "missing.bed"))


# ---- tbh_tool summary: the host summariser and the writer on the golden tracks ----------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tool_summary_on_the_golden_tracks(tmp_path, bam_loader, name):
    from tiebrush_amd import api
    bam = os.path.join(GOLDEN, name, name + ".bam")
    cov, junc = os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed")
    names, lens = _header(bam_loader, bam)
    rows = fs.read_tracks(cov, junc, names)
    assert len(rows["iv_tid"]) > 100 and len(rows["j_tid"]) >= 1
    bed = tmp_path / "g.bed"
    bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
    feats = api.features_from_bed(bam, str(bed))
    model = fm.mark_dyadic(rows, fm.per_row(rows, feats))
    assert all(fm.exact(m) for m in model)                        # YC is integral in the goldens
    assert sum(m["covered"] > 0 for m in model) >= 10 and sum(m["junc"] > 0 for m in model) >= 1 and any(m["covered"] == 0 for m in model)
    out = tmp_path / "o.tsv"
    r = rf.tool("summary", bam, cov, junc, bed, out)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == fm.tsv(names, feats, model)
    # a track that is not there leaves its columns zero
    r = rf.tool("summary", bam, "-", junc, bed, out)
    assert r.returncode == 0, r.stderr
    zero = [dict(m, covered=0, S=Fraction(0), max=0.0) for m in model]
    assert out.read_bytes() == fm.tsv(names, feats, zero)
    # a refused BED leaves no file
    bad = tmp_path / "bad.bed"
    bad.write_text("%s\t5\t1\n" % names[0])
    r = rf.tool("summary", bam, cov, junc, bad, tmp_path / "no.tsv")
    assert r.returncode == 1 and "bad.bed line 1" in r.stderr and not (tmp_path / "no.tsv").exists()


# ---- the host summariser on the scenes (tbh_cov_summary_host) ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fs.SCENES) + ["random"])
def test_host_summariser_on_the_scenes(name):
    from tiebrush_amd import api
    rows, feats = fs.random_case() if name == "random" else fs.SCENES[name]()[:2]
    got = api.cov_summary_host(rows, feats)
    for k, m in enumerate(fm.mark_dyadic(rows, fm.per_row(rows, feats))):
        assert int(got["covered"][k]) == m["covered"] and float(got["max"][k]) == m["max"] and float(got["junc"][k]) == m["junc"], (k, m)
        fm.check_sum(got["sum"][k], m)


def test_mirrored_constants_are_the_kernels():
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiebrush_amd", "csrc", "featsum.hip")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (FS_TILE|FS_DIRECT) = (\d+);", src)}
    assert got == {"FS_TILE": fs.FS_TILE, "FS_DIRECT": fs.FS_DIRECT} == {"FS_TILE": fm.FS_TILE, "FS_DIRECT": fm.FS_DIRECT}
    assert "FS_DIRECT = %d" % fm.FS_DIRECT in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "feature_prof.py")).read()
