"""The bigWig scenes and their numpy model against the host writer (no GPU): the model is what tests/test_gpu_bigwig.py's expectations
rest on, so it is pinned here to `tbh_tool bedgraph2bw` payload for payload, each scene to the edge it claims, and the new entry
points to their declarations."""
import os
import re

import pytest

import bigwig_model
import bigwig_payloads as bp
import bigwig_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bw_host")


@pytest.mark.parametrize("name", bigwig_scenes.names())
def test_model_equals_host_writer(name, host_dir):
    scene = bigwig_scenes.by_name(name)
    want = bp.host_file(scene, host_dir)
    m = bigwig_model.model(scene)
    bp.same_levels(m["levels"], want["levels"])
    assert want["summary"][0] == m["covered"]
    assert want["ubuf"] == max([len(s[3]) for lv in m["levels"] for s in lv["sections"]], default=0)
    assert {k: v[0] for k, v in want["chroms"].items()} == {i: c[0] for i, c in enumerate(scene.chroms)}


@pytest.mark.parametrize("name", bigwig_scenes.names())
def test_scene_sits_on_its_edge(name):
    scene = bigwig_scenes.by_name(name)
    assert scene.check(bigwig_model.model(scene)), scene.edge


def test_scenes_cover_the_issue_list():
    m = {s.name: bigwig_model.model(s) for s in bigwig_scenes.scenes()}
    assert len(m["dense_40k"]["levels"]) >= 4                      # at least three zoom levels
    assert len(m["chroms_700"]["levels"][0]["sections"]) > 256     # a two-level R-tree
    assert max(m["item_across_90_bins"]["opens"][0]) >= 90


def test_two_level_rtree_in_the_host_file(host_dir):
    v = bp.host_file(bigwig_scenes.by_name("chroms_700"), host_dir)
    hdr, nodes = v["levels"][0]["rtree"]
    assert hdr[1] == 700 and nodes[0][0] == 0 and len(nodes) == 1 + 3   # a root above three leaves


def test_new_symbols_declared_and_bound():
    from tiebrush_amd import _lib
    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    dl = open(os.path.join(ROOT, "tiebrush_amd", "csrc", "host", "tbk_dl.h")).read()
    for sym in ("tbk_zlib_deflate", "tbk_bigwig_build"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.SYMBOLS, sym
    assert "tbk_bigwig_build" in dl
    assert re.search(r"#define TBK_ABI_VERSION 9\b", header)
    L = _lib.load()
    assert L.tbk_abi_version() == 9
    assert L.tbk_zlib_deflate.restype is not None and L.tbk_bigwig_build.restype is not None
    assert _lib.BW_MAX_ZOOM == int(re.search(r"#define TBK_BW_MAX_ZOOM (\d+)", header).group(1))
    import ctypes as C
    assert C.sizeof(_lib.BwSection) == 32 and C.sizeof(_lib.BwLevel) == 40 and C.sizeof(_lib.BwOut) == 8 + 40 * 11
