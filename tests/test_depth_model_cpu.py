"""CPU side of `--thresholds / --depth-summary / --feature-depth`: the two forms of the model agree on every scene and
prove the scenes' claims; the threshold parser of libtbh; the host loop on the scenes; `tbh_tool depth` (the host loops and the table
writers) on the golden coverage tracks, in the plain build and in the sanitizer build of the stand-alone tool."""
import os
import subprocess

import numpy as np
import pytest

import depth_model as dm
import depth_scenes as ds
import feature_scenes as fs
import region_fixtures as rf
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR_TEXT = ["2", "5", "10", "50", "1000", "30000"]
THR_ARG = ",".join(THR_TEXT)


@pytest.fixture(scope="module")
def scenes():
    return {name: f() for name, f in ds.SCENES.items()}


@pytest.mark.parametrize("name", sorted(ds.SCENES))
def test_model_forms_agree_and_prove_the_claims(scenes, name):
    rows, feats, thr, claims = scenes[name]
    n = len(feats["tid"])
    assert n >= 1 and 1 <= len(thr) <= dm.MAX_THRESHOLDS and all(a < b for a, b in zip(thr, thr[1:])) and thr[0] > 0
    cov, ge = dm.per_row(rows, feats, thr)
    base = dm.per_base(rows, feats, thr)
    for f in range(n):
        if base[f] is not None:
            assert base[f][0] == int(cov[f]) and base[f][1] == [int(x) for x in ge[f]], f
        assert all(int(ge[f, k]) >= int(ge[f, k + 1]) for k in range(len(thr) - 1)) and int(ge[f, 0]) <= int(cov[f])
    if claims.get("zero"):
        assert not ge.any() and cov.any()
    if claims.get("all"):
        assert np.array_equal(ge[:, 0], cov) and cov.any()
    for (f, k), want in claims.get("cells", {}).items():
        assert int(ge[f, k]) == want, (f, k, int(ge[f, k]), want)


def test_the_scenes_cover_the_list_sizes_and_both_paths():
    import feature_model as fm
    assert {len(ds.SCENES[n]()[2]) for n in ds.SCENES} >= {1, 16}
    assert {len(ds.SCENES["list%d" % n]()[1]["tid"]) for n in fs.LIST_N} == {1, 64, 65, 257}
    rows, feats, _, _ = ds.runs13()
    m = fm.per_row(rows, feats)
    assert {x["path"] for x in m} == {"direct", "agg"} and {x["tiles"] for x in m if x["path"] == "agg"} >= {0, 1, 2, 3}


# ---- the threshold parser (tbh_parse_thresholds: what both command lines and tbh_tool depth run) ----------------------------------------
@pytest.mark.parametrize("text,want", [("1", [1.0]), ("2,5,10,50,1000,30000", [2, 5, 10, 50, 1000, 30000]), ("0.5,1.5", [0.5, 1.5]), ("1e3", [1000.0]),
                                       ("+2,2.5e0,.75e1", [2.0, 2.5, 7.5]), (",".join(str(k) for k in range(1, 17)), list(range(1, 17))),
                                       ("1e-300,1e300", [1e-300, 1e300]), ("0.1,0.30000000000000004", [0.1, 0.30000000000000004])])
def test_threshold_parser_accepts(text, want):
    from tiebrush_amd import api
    got = api.parse_thresholds(text)
    assert got.dtype == np.float64 and got.tolist() == [float(w) for w in want]


@pytest.mark.parametrize("text,item", [("", ""), ("1,,2", ""), ("1,2,", ""), ("abc", "abc"), ("1,2x", "2x"), ("1, 2", " 2"), ("0", "0"), ("-1", "-1"), ("1,0.5", "0.5"),
                                       ("1,1", "1"), ("2,1e0", "1e0"), ("nan", "nan"), ("1,inf", "inf"), ("1,1e999", "1e999"), ("0x10", "0x10"), ("1;2", "1;2"),
                                       (",".join(str(k) for k in range(1, 18)), "17"), ("1e-999", "1e-999")])
def test_threshold_parser_refuses_with_the_item(text, item):
    from tiebrush_amd import api
    with pytest.raises(RuntimeError) as e:
        api.parse_thresholds(text)
    assert "--thresholds" in str(e.value) and "'%s'" % item in str(e.value), str(e.value)


# ---- the host loop on the scenes (tbh_cov_thresholds_host) -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ds.SCENES))
def test_host_loop_on_the_scenes(scenes, name):
    from tiebrush_amd import api
    rows, feats, thr, _ = scenes[name]
    got = api.cov_thresholds_host(rows, feats, thr)
    cov, ge = dm.per_row(rows, feats, thr)
    assert got["covered"].dtype == np.uint64 and got["ge"].dtype == np.uint64 and got["ge"].shape == (len(feats["tid"]), len(thr))
    assert np.array_equal(got["covered"], cov) and np.array_equal(got["ge"], ge)


@pytest.mark.parametrize("thr", [[], list(range(1, 18)), [2.0, 1.0], [1.0, 1.0], [float("nan")], [1.0, float("inf")], [0.0], [-1.0, 1.0]])
def test_host_loop_refuses_the_thresholds(scenes, thr):
    from tiebrush_amd import api
    rows, feats = scenes["equal"][:2]
    with pytest.raises(RuntimeError):
        api.cov_thresholds_host(rows, feats, thr)


# ---- tbh_tool depth: the host loops and the writers on the golden tracks ------------------------------------------------------------------
def _golden(name, bam_loader):
    bam = os.path.join(GOLDEN, name, name + ".bam")
    cov = os.path.join(GOLDEN, name, name + ".coverage.bedgraph")
    h = bam_loader(bam).header
    names, lens = list(h.ref_names), list(h.ref_lens)
    rows = fs.read_tracks(cov, os.path.join(GOLDEN, name, name + ".junctions.bed"), names)
    return bam, cov, names, lens, rows


@pytest.fixture(scope="module")
def golden_tables(bam_loader, tmp_path_factory):
    """per golden: the model's two texts, computed once"""
    from tiebrush_amd import api
    out = {}
    for name in ("t1", "t2"):
        bam, cov, names, lens, rows = _golden(name, bam_loader)
        thr = [float(t) for t in THR_TEXT]
        text, tot = dm.depth_tsv(names, lens, THR_TEXT, dm.per_ref(rows, lens, thr))
        bed = tmp_path_factory.mktemp("depth_" + name) / "g.bed"
        bed.write_text("\n".join(fs.golden_bed(rows, names, lens)) + "\n")
        feats = api.features_from_bed(bam, str(bed))
        fcov, fge = dm.per_row(rows, feats, thr)
        out[name] = dict(bam=bam, cov=cov, names=names, lens=lens, text=text, total=tot, bed=str(bed), ftext=dm.feature_tsv(names, feats, THR_TEXT, fcov, fge),
                         plain=dm.depth_tsv(names, lens, [], dm.per_ref(rows, lens, []))[0], fge=fge, fcov=fcov)
    return out


@pytest.mark.parametrize("name", ["t1", "t2"])
def test_tool_depth_on_the_golden_tracks(tmp_path, golden_tables, name):
    g = golden_tables[name]
    out = tmp_path / "o.tsv"
    r = rf.tool("depth", g["bam"], g["cov"], THR_ARG, out)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == g["text"]
    assert g["text"].split(b"\n")[0] == b"#chrom\tlength\tcovered\tsum\tmean0\tmean\tmax\tge_2\tge_5\tge_10\tge_50\tge_1000\tge_30000"
    assert len(g["text"].split(b"\n")) == len(g["names"]) + 3 and g["text"].split(b"\n")[-2].startswith(b"total\t")
    if name == "t1":                                       # computed from the golden file; its max is 26843
        t = g["total"]
        assert t["covered"] == 9417 and t["ge"] == [7862, 6263, 6151, 2206, t["ge"][4], 0] and t["max"] == 26843.0
    # no thresholds: no ge_ columns
    r = rf.tool("depth", g["bam"], g["cov"], "-", out)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == g["plain"] and b"ge_" not in g["plain"]
    # the per-feature table of golden_bed's features
    r = rf.tool("depth", g["bam"], g["cov"], THR_ARG, out, g["bed"])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == g["ftext"]
    assert g["fcov"].any() and g["fge"][:, 0].any() and (g["fcov"] == 0).any()
    # the names are the text as given
    r = rf.tool("depth", g["bam"], g["cov"], "2.0,5e0,+10", out)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes().split(b"\n")[0].endswith(b"\tmax\tge_2.0\tge_5e0\tge_+10")
    assert [ln.split(b"\t")[7:] for ln in out.read_bytes().split(b"\n")[1:-1]] == [ln.split(b"\t")[7:10] for ln in g["text"].split(b"\n")[1:-1]]
    # refusals leave no file
    for args, msg in ((("2,1",), "'1'"), (("0",), "'0'"), ((THR_ARG, os.path.join(str(tmp_path), "missing.bed")), "cannot read")):
        no = tmp_path / "no.tsv"
        r = rf.tool("depth", g["bam"], g["cov"], args[0], no, *args[1:])
        assert r.returncode == 1 and msg in r.stderr and not no.exists(), r.stderr


def test_tool_depth_under_the_sanitizers(tmp_path, golden_tables):
    """the stand-alone tool built with SAN=address,undefined gives the same bytes and no report"""
    host = os.path.join(ROOT, "tiebrush_amd", "csrc", "host")
    tool = os.path.join(ROOT, "tiebrush_amd", "_build_san_address_undefined", "tbh_tool")
    r = subprocess.run(["make", "-C", host, "SAN=address,undefined", "../../_build_san_address_undefined/tbh_tool"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in ("t1", "t2"):
        g = golden_tables[name]
        for extra, want in (((), g["text"]), ((g["bed"],), g["ftext"])):
            out = tmp_path / "san.tsv"
            r = subprocess.run([tool, "depth", g["bam"], g["cov"], THR_ARG, str(out)] + list(extra), capture_output=True, text=True, env=env)
            assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
            assert out.read_bytes() == want
    r = subprocess.run([tool, "depth", golden_tables["t1"]["bam"], golden_tables["t1"]["cov"], "1,x", str(tmp_path / "no.tsv")], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "'x'" in r.stderr and "ERROR" not in r.stderr and "runtime error" not in r.stderr
