"""A payload-level view of bigWig files and of tbk_bigwig_build's output, on top of bigwig_reader.BigWig: what the contract between the
two section producers speaks about — levels, reductions, sections in order with their inflated payloads, R-tree keys,
chromosome tree, summary, section count, uncompressBufSize — and nothing of what may differ (compressed bytes, offsets, sizes)."""
import os
import struct
import subprocess
import zlib

from bigwig_reader import BigWig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("TBK_TEST_TBH_TOOL") or os.path.join(ROOT, "tiebrush_amd", "_build", "tbh_tool")


def _rtree(bw, index_off):
    """-> (header keys, [node keys in file order]): every bounding range the index holds, without offsets and sizes"""
    d = bw.d
    magic, block, count, c0, s0, c1, e1, _end_off, per_slot, _ = struct.unpack_from("<IIQIIIIQII", d, index_off)
    assert magic == 0x2468ACE0
    nodes = []

    def walk(off):
        leaf, _, n = struct.unpack_from("<BBH", d, off)
        p = off + 4
        keys, kids = [], []
        for _ in range(n):
            a, b, c, e, o = struct.unpack_from("<IIIIQ", d, p)
            keys.append((a, b, c, e))
            if not leaf:
                kids.append(o)
            p += 32 if leaf else 24
        nodes.append((leaf, tuple(keys)))
        for o in kids:
            walk(o)
    walk(index_off + 48)
    return (block, count, c0, s0, c1, e1, per_slot), nodes


def file_view(path):
    """everything the contract pins, of one file"""
    bw = BigWig(path)
    levels = []
    n_sections = struct.unpack_from("<Q", bw.d, bw.data_off)[0]
    heads = [(0, bw.data_off, bw.index_off)] + [(red, doff, ioff) for red, _, doff, ioff in bw.zoom_headers]
    for k, (red, doff, ioff) in enumerate(heads):
        blocks = bw._blocks(ioff)
        secs = []
        for a, b, c, e, o, sz in blocks:
            assert a == c
            secs.append((a, b, e, zlib.decompress(bw.d[o:o + sz])))   # (plain zlib.decompress: it checks the Adler-32)
        n_items = sum((len(p) - 24) // 12 for *_k, p in secs) if k == 0 else struct.unpack_from("<I", bw.d, doff)[0]
        levels.append(dict(reduction=red, n_items=n_items, sections=secs, rtree=_rtree(bw, ioff)))
    assert n_sections == len(levels[0]["sections"])
    return dict(levels=levels, chroms=bw.chroms, summary=bw.summary, n_sections=n_sections, ubuf=bw.ubuf, version=bw.version)


def build_view(levels):
    """Context.bigwig_build's result in the same terms (sections inflated with plain zlib.decompress)"""
    out = []
    for lv in levels:
        secs = []
        pos = 0
        for chrom, start, end, off, size in lv["sections"]:
            assert off == pos, "the streams lie back to back in section order"
            secs.append((chrom, start, end, zlib.decompress(lv["bytes"][off:off + size])))
            pos = off + size
        assert pos == len(lv["bytes"])
        assert lv["max_payload"] == max([len(p) for *_k, p in secs], default=0)
        out.append(dict(reduction=lv["reduction"], n_items=lv["n_items"], sections=secs))
    return out


def same_levels(got, want):
    """levels, reductions, item counts, sections in order with identical payload bytes; raises with the first difference"""
    assert [lv["reduction"] for lv in got] == [lv["reduction"] for lv in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["n_items"] == w["n_items"], (k, g["n_items"], w["n_items"])
        assert len(g["sections"]) == len(w["sections"]), (k, len(g["sections"]), len(w["sections"]))
        for i, (a, b) in enumerate(zip(g["sections"], w["sections"])):
            assert a[:3] == b[:3], (k, i, a[:3], b[:3])
            if a[3] != b[3]:
                j = next((x for x in range(min(len(a[3]), len(b[3]))) if a[3][x] != b[3][x]), min(len(a[3]), len(b[3])))
                raise AssertionError("level %d section %d: payloads differ at byte %d (lengths %d / %d)" % (k, i, j, len(a[3]), len(b[3])))


def same_files(got, want):
    """the whole contract between two files (file_view of each)"""
    same_levels(got["levels"], want["levels"])
    for k, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        assert g["rtree"] == w["rtree"], "R-tree keys of level %d" % k
    for key in ("chroms", "summary", "n_sections", "ubuf", "version"):
        assert got[key] == want[key], key


_HOST = {}


def host_file(scene, tmpdir):
    """the host writer's file of a scene (tbh_tool bedgraph2bw with a SAM header as the chromosome list), written once per directory"""
    key = (scene.name, str(tmpdir))
    if key not in _HOST:
        sam, bg, out = (os.path.join(str(tmpdir), scene.name + ext) for ext in (".sam", ".bedgraph", ".bigwig"))
        open(sam, "w").write(scene.sam_header())
        open(bg, "w").write(scene.bedgraph())
        r = subprocess.run([TOOL, "bedgraph2bw", sam, bg, out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _HOST[key] = file_view(out)
    return _HOST[key]
