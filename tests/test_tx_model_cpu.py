"""CPU side of `--gtf FILE --transcripts OUT`: the two forms of the model agree on every scene and prove the scenes'
claims; the GTF parser of libtbh; the host summariser on the scenes; `tbh_tool transcripts` on the golden tracks; the option rules that
are refused before a device is touched."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import feature_model as fm
import feature_scenes as fs
import region_fixtures as rf
import tx_model as tm
import tx_scenes as ts
from helpers import GOLDEN, sample_paths

GTF = os.path.join(GOLDEN, "sashimi", "example.gtf")


@pytest.fixture(scope="module")
def scenes():
    return {name: f() for name, f in ts.SCENES.items()}


@pytest.fixture(scope="module")
def models(scenes):
    return {name: tm.per_row(rows, tx) for name, (rows, tx, _) in scenes.items()}


def _table_is_valid(tx):
    off = tx["tx_off"].astype(np.int64)
    assert off[0] == 0 and off[-1] == len(tx["ex_beg"]) and np.all(np.diff(off) >= 1) and len(tx["tid"]) == len(off) - 1
    assert np.all(tx["ex_end"] > tx["ex_beg"]) and np.all(tx["ex_beg"] >= 0)
    for k in range(len(off) - 1):
        assert np.all(tx["ex_beg"][off[k] + 1:off[k + 1]] > tx["ex_end"][off[k]:off[k + 1] - 1]), k     # ascending, an intron has a base


@pytest.mark.parametrize("name", sorted(ts.SCENES))
def test_model_forms_agree_and_prove_the_claims(scenes, models, name):
    rows, tx, claims = scenes[name]
    _table_is_valid(tx)
    a, b = models[name], tm.per_base(rows, tx)
    assert len(a) == len(b) == len(claims) == len(tx["tid"]) >= 1
    for k, (m, d) in enumerate(zip(a, b)):
        if d["covered"] is not None:
            assert (d["covered"], d["max"], d["exons_hit"]) == (m["covered"], m["max"], m["exons_hit"]), (name, k)
            assert d["sum"] == float(m["S"]), (name, k)                  # both are the exact sum rounded once
        assert (d["introns_hit"], d["junc_min"]) == (m["introns_hit"], m["junc_min"]) and d["junc_sum"] == float(m["JS"]), (name, k)
        for key, want in claims[k].items():
            if key == "parts":
                assert len(want) == len(m["parts"])
                for p, w in zip(m["parts"], want):
                    for pk, pv in w.items():
                        assert (p["hi"] - p["lo"] if pk == "hi_lo" else p[pk]) == pv, (name, k, pk)
            else:
                assert m[key] == want, (name, k, key, m[key], want)
    if name == "thirds":
        assert not any(tm.exact(m) for m in a) and not any(tm.jexact(m) for m in a if m["jm"])
    elif name == "top":
        assert not tm.exact(a[1]) and tm.exact(a[2])
    else:
        assert all(tm.exact(m) and tm.jexact(m) for m in a)


def test_the_scenes_reach_their_edges(scenes, models):
    assert {m["exons"] for m in models["sizes"]} == {1, 2, 63, 64, 65, 129}
    for m in models["sizes"]:                                             # a true minimum: neither the first nor the last intron's value
        if m["introns"] >= 3:
            assert m["junc_min"] < min(m["junc"][0], m["junc"][-1]) and m["junc"].count(m["junc_min"]) == 1
    for n in ts.LIST_N:
        rows, tx, _ = scenes["list%d" % n]
        assert len(tx["tid"]) == n
        if n >= 64:
            sizes = np.diff(tx["tx_off"].astype(np.int64))
            assert len(set(sizes.tolist())) >= 5 and sizes.max() > 64
            starts = tx["ex_beg"][tx["tx_off"][:-1]]
            assert np.all(np.diff(starts) <= 0) and np.any(np.diff(starts) == 0)        # descending, with duplicates
            assert {m["introns_hit"] > 0 for m in models["list%d" % n]} == {True, False}
    runs = [p["hi"] - p["lo"] for m in models["run_exons"] for p in m["parts"]]
    assert {ts.D - 1, ts.D, ts.D + 1} <= set(runs)
    assert any(p["path"] == "agg" and p["tiles"] == 2 for m in models["run_exons"] for p in m["parts"])
    for name in ("last_exon_same_ref", "last_exon_next_ref"):            # the row between A's last exon and B's first is there, and is nobody's
        rows, tx, _ = scenes[name]
        key = (int(tx["ex_end"][1]), int(tx["ex_beg"][2]))
        assert key in set(zip(rows["j_start"].tolist(), rows["j_end"].tolist())) and int(tx["tx_off"][1]) == 2
        assert (tx["tid"][1] != tx["tid"][0]) == (name == "last_exon_next_ref")
        assert int(tx["ex_end"][-1]) in rows["j_start"].tolist()
        assert sum(m["JS"] for m in models[name]) == 5
    m = models["introns"]
    assert any(0 < x["introns_hit"] < x["introns"] and x["junc_min"] == 0 for x in m)
    assert any(x["introns_hit"] == x["introns"] == 3 and x["junc_min"] not in (x["junc"][0], x["junc"][-1]) for x in m)


def test_random_case_meets_its_conditions():
    rows, tx = ts.random_case()
    _table_is_valid(tx)
    assert len(rows["iv_tid"]) <= 4000 and len(tx["tid"]) <= 300
    m = tm.per_row(rows, tx)
    assert any(x["exons"] == 1 for x in m)
    assert any(x["introns"] >= 1 and x["introns_hit"] == x["introns"] for x in m)
    assert any(0 < x["introns_hit"] < x["introns"] for x in m)
    assert any(x["covered"] == 0 for x in m) and any(x["covered"] > 0 for x in m)
    assert any(p["path"] == "agg" for x in m for p in x["parts"])
    assert all(tm.exact(x) and tm.jexact(x) for x in m)


# ---- the host summariser (tbh_tx_summary_host) -----------------------------------------------------------------------------------------
def _check_parts(got, rows, tx, ref):
    """the per-exon columns against `ref`, a cov_summary of the exons / the introns as features, bit for bit"""
    ex, (inf, at) = ref(rows, tm.exon_feats(tx)), tm.intron_feats(tx)
    for k in ("covered", "sum", "max"):
        assert got["ex_" + k].tobytes() == ex[k].tobytes(), k
    want = np.zeros(len(tx["ex_beg"]))
    if len(at):
        want[at] = ref(rows, inf)["junc"]
    assert got["in_junc"].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sorted(ts.SCENES) + ["random"])
def test_host_summariser_on_the_scenes(scenes, models, name):
    from tiebrush_amd import api
    rows, tx = ts.random_case() if name == "random" else scenes[name][:2]
    model = tm.per_row(rows, tx) if name == "random" else models[name]
    got = api.tx_summary_host(rows, tx)
    assert got["covered"].dtype == np.uint64 and got["exons_hit"].dtype == np.uint32 and got["junc_min"].dtype == np.float64
    for k in range(len(model)):
        tm.check(got, model, k)
    _check_parts(got, rows, tx, api.cov_summary_host)
    only_c = api.tx_summary_host({k: v for k, v in rows.items() if k[:3] == "iv_"}, tx)
    assert sorted(only_c) == ["covered", "ex_covered", "ex_max", "ex_sum", "exons_hit", "max", "sum"] and only_c["sum"].tobytes() == got["sum"].tobytes()
    only_j = api.tx_summary_host({k: v for k, v in rows.items() if k[:2] == "j_"}, tx)
    assert sorted(only_j) == ["in_junc", "introns_hit", "junc_min", "junc_sum"] and only_j["junc_sum"].tobytes() == got["junc_sum"].tobytes()


def test_host_summariser_refuses_a_broken_table(scenes):
    from tiebrush_amd import api
    rows, tx, _ = scenes["isoforms"]
    for bad in (dict(tx, tx_off=np.array([1, 2, 5, 7, 10, 11], np.uint32)), dict(tx, ex_beg=tx["ex_beg"][::-1].copy()), dict(tx, strand=np.full(6, ord("*"), np.uint8))):
        with pytest.raises(RuntimeError):
            api.tx_summary_host(rows, bad)


# ---- the GTF parser (tbh_transcripts_from_gtf) -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chr19(tmp_path_factory):
    """a header-only input: @SQ chr19 and a short second reference"""
    from tiebrush_amd import bamio
    names, lens = ["chr19", "chrS"], [58617616, 1000]
    path = str(tmp_path_factory.mktemp("gtf") / "header.bam")
    bamio.write_bam(path, "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lens)), names, lens, b"", level=6)
    return path


def test_the_reference_example_parses_to_the_pinned_table(chr19):
    from tiebrush_amd import api
    text = open(GTF).read().split("\n")
    kinds = [ln.split("\t")[2] for ln in text if ln]
    assert (len(kinds), kinds.count("transcript"), kinds.count("CDS"), kinds.count("exon")) == (30, 3, 12, 15) and os.path.getsize(GTF) == 3839
    x = api.transcripts_from_gtf(chr19, GTF)
    assert x["id"] == ["ENST00000592529.6", "ORFanage:ENST00000590088.5", "ENST00000590088.5"]
    assert x["gene"] == ["ENSG00000167384.11", ".", "ENSG00000167384.11"]                       # (the second transcript's lines carry no gene_id)
    assert x["tx_off"].tolist() == [0, 5, 10, 15] and x["tid"].tolist() == [0, 0, 0] and bytes(x["strand"]) == b"---"
    for k in range(3):                                                   # the exons of every transcript, from the file itself
        ex = sorted((int(f[3]) - 1, int(f[4])) for f in (ln.split("\t") for ln in text if ln) if f[2] == "exon" and f[8].startswith('transcript_id "%s"' % x["id"][k]))
        a, b = int(x["tx_off"][k]), int(x["tx_off"][k + 1])
        assert list(zip(x["ex_beg"][a:b].tolist(), x["ex_end"][a:b].tolist())) == ex and len(ex) == 5
    first = [(int(x["ex_beg"][o]), int(x["ex_end"][o])) for o in x["tx_off"][:-1]]
    last = [(int(x["ex_beg"][o - 1]), int(x["ex_end"][o - 1])) for o in x["tx_off"][1:]]
    assert first == [(44474442, 44478146), (44475638, 44478146), (44475638, 44478146)]
    assert last == [(44500274, 44500522), (44500197, 44500524), (44500197, 44500524)]
    assert x["line"].tolist() == [2, 12, 23]
    assert x["tx_off"].dtype == np.uint32 and x["tid"].dtype == np.int32 and x["ex_beg"].dtype == np.int64 and x["strand"].dtype == np.uint8


def test_parser_accepts(tmp_path, chr19):
    from tiebrush_amd import api
    g = tmp_path / "a.gtf"
    A = 'transcript_id "A"; gene_id "g;1"; note "x";'
    g.write_text("# comment\n\n   \t\n"
                 "chr19\ts\ttranscript\tnot\tread\n" +                                           # line 4: not an exon line, never looked at
                 "chr19\ts\texon\t301\t400\t.\t-\t.\t%s\r\n" % A +                               # 5: minus strand, listed descending, CR
                 "chr19\ts\tCDS\t0\t0\t.\t*\t.\tnothing\n" +
                 "chr19\ts\texon\t101\t200\t.\t-\t.\t%s\n" % A +                                 # 7
                 "chrS\ts\texon\t1\t1000\t.\t.\t.\tgene_name q; transcript_id B\n" +             # 8: bare values, no gene_id, the whole reference
                 "chr19\ts\texon\t1\t50\t.\t-\t.\t%s\n" % A +                                    # 9
                 "chr19\ts\texon\t10\t20\t.\t+\t.\tgene_id G2; transcript_id \"C D\" ; x 1")     # 10: no newline at the end
    x = api.transcripts_from_gtf(chr19, str(g))
    assert x["id"] == ["A", "B", "C D"] and x["gene"] == ["g;1", ".", "G2"] and x["line"].tolist() == [5, 8, 10]
    assert x["tx_off"].tolist() == [0, 3, 4, 5] and x["tid"].tolist() == [0, 1, 0] and bytes(x["strand"]) == b"-.+"
    assert x["ex_beg"].tolist() == [0, 100, 300, 0, 9] and x["ex_end"].tolist() == [50, 200, 400, 1000, 20]
    many = tmp_path / "many.gtf"                                                                  # more than the first buffers hold
    many.write_text("".join("chr19\ts\texon\t%d\t%d\t.\t+\t.\ttranscript_id \"transcript_number_%05d\"; gene_id \"gene_%05d\";\n" % (100 * e + 1, 100 * e + 50, t, t)
                            for t in range(200) for e in range(1 + t % 4)))
    y = api.transcripts_from_gtf(chr19, str(many))
    assert len(y["tid"]) == 200 and y["id"][199] == "transcript_number_00199" and y["gene"][7] == "gene_00007"
    assert np.diff(y["tx_off"].astype(np.int64)).tolist() == [1 + t % 4 for t in range(200)] and len(y["ex_beg"]) == 500


GOOD = 'chr19\ts\texon\t101\t200\t.\t+\t.\ttranscript_id "T";'


@pytest.mark.parametrize("line,msg", [("chr19\ts\texon\t1\t2\t.\t+\t.", "fewer than nine"), ("chr19\ts\texon\tone\t2\t.\t+\t.\ttranscript_id \"U\";", "start"),
                                      ("chr19\ts\texon\t1\t2.5\t.\t+\t.\ttranscript_id \"U\";", "end"), ("chr19\ts\texon\t0\t5\t.\t+\t.\ttranscript_id \"U\";", "start < 1"),
                                      ("chr19\ts\texon\t9\t5\t.\t+\t.\ttranscript_id \"U\";", "end < start"), ("chrS\ts\texon\t900\t1001\t.\t+\t.\ttranscript_id \"U\";", "beyond"),
                                      ("chr20\ts\texon\t1\t5\t.\t+\t.\ttranscript_id \"U\";", "unknown reference"), ("chr19\ts\texon\t1\t5\t.\t*\t.\ttranscript_id \"U\";", "strand"),
                                      ("chr19\ts\texon\t1\t5\t.\t+\t.\tgene_id \"G\";", "transcript_id"), ("chrS\ts\texon\t1\t5\t.\t+\t.\ttranscript_id \"T\";", "two references"),
                                      ("chr19\ts\texon\t1\t5\t.\t-\t.\ttranscript_id \"T\";", "two strands"), ("chr19\ts\texon\t150\t300\t.\t+\t.\ttranscript_id \"T\";", "overlap or abut"),
                                      ("chr19\ts\texon\t201\t300\t.\t+\t.\ttranscript_id \"T\";", "overlap or abut"), ("chr19\ts\texon\t51\t100\t.\t+\t.\ttranscript_id \"T\";", "overlap or abut")])
def test_parser_refuses_with_the_line_number(tmp_path, chr19, line, msg):
    from tiebrush_amd import api
    g = tmp_path / "bad.gtf"
    g.write_text("#h\n" + GOOD + "\n" + line + "\n" + GOOD.replace("101\t200", "1001\t1100") + "\n")
    with pytest.raises(RuntimeError) as e:
        api.transcripts_from_gtf(chr19, str(g))
    assert "bad.gtf line 3" in str(e.value) and msg in str(e.value), str(e.value)


def test_parser_refuses_a_file_without_exons(tmp_path, chr19):
    from tiebrush_amd import api
    g = tmp_path / "none.gtf"
    g.write_text("# nothing\n\nchr19\ts\ttranscript\t1\t5\t.\t+\t.\ttranscript_id \"T\";\nchr19\ts\tCDS\t1\t5\t.\t+\t0\ttranscript_id \"T\";\n")
    with pytest.raises(RuntimeError, match="no exon line"):
        api.transcripts_from_gtf(chr19, str(g))
    with pytest.raises(RuntimeError, match="cannot read"):
        api.transcripts_from_gtf(chr19, str(tmp_path / "missing.gtf"))


# ---- tbh_tool transcripts: the host summariser and the writer on the golden tracks -------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tool_transcripts_on_the_golden_tracks(tmp_path, bam_loader, name):
    from tiebrush_amd import api
    bam = os.path.join(GOLDEN, name, name + ".bam")
    cov, junc = os.path.join(GOLDEN, name, name + ".coverage.bedgraph"), os.path.join(GOLDEN, name, name + ".junctions.bed")
    h = bam_loader(bam).header
    names, lens = list(h.ref_names), list(h.ref_lens)
    rows = fs.read_tracks(cov, junc, names)
    gtf = tmp_path / "g.gtf"
    gtf.write_text("\n".join(ts.golden_gtf(rows, names, lens)) + "\n")
    tx = api.transcripts_from_gtf(bam, str(gtf))
    model = tm.per_row(rows, tx)
    assert all(tm.exact(m) and tm.jexact(m) for m in model)               # YC is integral in the goldens
    assert any(m["introns"] >= 2 and m["introns_hit"] == m["introns"] for m in model) and any(m["exons"] == 1 and m["covered"] > 0 for m in model)
    assert model[-1]["introns"] == 1 and model[-1]["introns_hit"] == 0 and model[-1]["covered"] == 20      # the invented intron
    out = tmp_path / "o.tsv"
    r = rf.tool("transcripts", bam, cov, junc, gtf, out)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == tm.tsv(names, tx, model)
    # a track that is not there leaves its columns zero
    r = rf.tool("transcripts", bam, cov, "-", gtf, out)
    assert r.returncode == 0, r.stderr
    zero = [dict(m, introns_hit=0, junc_min=0.0, JS=Fraction(0)) for m in model]
    assert out.read_bytes() == tm.tsv(names, tx, zero)
    # a refused GTF leaves no file
    bad = tmp_path / "bad.gtf"
    bad.write_text("%s\ts\texon\t5\t1\t.\t+\t.\ttranscript_id \"T\";\n" % names[0])
    r = rf.tool("transcripts", bam, cov, junc, bad, tmp_path / "no.tsv")
    assert r.returncode == 1 and "bad.gtf line 1" in r.stderr and not (tmp_path / "no.tsv").exists()


# ---- option rules that are refused before a device is touched ----------------------------------------------------------------------------
def test_option_rules_without_a_device(tmp_path):
    bam = os.path.join(GOLDEN, "t1", "t1.bam")
    out = tmp_path / "out"
    out.mkdir()
    tsv, pre = out / "x.tsv", out / "c"
    cases = [("tiecov", ["--transcripts", tsv, "-c", pre, bam], "--gtf"),
             ("tiecov", ["--gtf", GTF, "-c", pre, bam], "--transcripts"),
             ("tiecov", ["--gtf", GTF, bam], "--transcripts"),
             ("tiecov", ["--stream", "--gtf", GTF, "--transcripts", tsv, "-c", pre, bam], "--stream"),
             ("tiebrush", ["-o", out / "o.bam", "--transcripts", tsv] + sample_paths("t1"), "--gtf"),
             ("tiebrush", ["-o", out / "o.bam", "--gtf", GTF] + sample_paths("t1"), "--transcripts"),
             ("tiebrush", ["-o", out / "o.bam", "--ranks", "2", "--gtf", GTF, "--transcripts", tsv] + sample_paths("t1"), "--ranks"),
             ("tiebrush", ["-o", out / "o.bam", "--ranks=2", "--transcripts=%s" % tsv, "--gtf=%s" % GTF] + sample_paths("t1"), "--ranks")]
    for tool, args, msg in cases:
        r = subprocess.run([os.path.join(rf.BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and msg in r.stderr and "Error" in r.stderr, (tool, args, r.stderr)
        assert os.listdir(str(out)) == [], (tool, args)
    for tool in ("tiecov", "tiebrush"):
        r = subprocess.run([os.path.join(rf.BIN, tool), "--help"], capture_output=True, text=True, timeout=60)
        assert "--gtf FILE --transcripts OUT.tsv" in r.stderr + r.stdout
