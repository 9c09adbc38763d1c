"""Hand-placed thresholds on feature_scenes' rows for tbk_cov_thresholds (tiebrush_amd/csrc/depththr.hip).  numpy only;
importable without a GPU.  A scene is (rows, feats, thr, claims): `claims` are facts about the input that tests/test_depth_model_cpu.py
proves through depth_model before the GPU is asked (tests/test_gpu_depth.py):
  zero=True          every count is 0 (a threshold above every value)
  all=True           ge == covered for every threshold (a threshold below every value)
  cells={(f, k): n}  single counts"""
import numpy as np

import feature_scenes as fs

T, D = fs.T, fs.D
UP, DOWN = np.inf, -np.inf


def _strip(rows):
    return {k: v for k, v in rows.items() if k[:3] == "iv_"}


def equal():
    """every threshold is a row's value: the comparison is inclusive"""
    rows, feats, _ = fs.edges()
    thr = [2.0, 3.0, 5.0, 7.0, 11.0, 13.0]
    # feature 1 is (1, 100, 200), the row of value 3; feature 11 is (1, 90, 100): no row
    return _strip(rows), feats, thr, dict(cells={(1, 0): 100, (1, 1): 100, (1, 2): 0, (11, 0): 0})


def nextafter():
    """one step below and one above a row's value, on the doubles"""
    rows, feats, _ = fs.edges()
    thr = [np.nextafter(3.0, DOWN), np.nextafter(3.0, UP), np.nextafter(13.0, DOWN), np.nextafter(13.0, UP)]
    # feature 1: the row of value 3; feature 21 is (2, 150, 230): 50 bases at 11, 30 at 13
    return _strip(rows), feats, thr, dict(cells={(1, 0): 100, (1, 1): 0, (21, 0): 80, (21, 1): 80, (21, 2): 30, (21, 3): 0})


def above_all():
    rows, feats, _ = fs.runs()
    return _strip(rows), feats, [1e9], dict(zero=True)


def below_all():
    rows, feats, _ = fs.runs()
    return _strip(rows), feats, [0.5], dict(all=True)


def thirds():
    """the rows' values are k x (1 / 3), none representable as a decimal: the thresholds are the same doubles, so each is met inclusively"""
    rows, feats, _ = fs.thirds()
    thr = [k * (1.0 / 3.0) for k in range(1, 14)]
    assert all(a < b for a, b in zip(thr, thr[1:])) and set(thr) == set(rows["iv_val"].tolist())
    return _strip(rows), feats, thr, dict()


RUNS13_THR = [float(k) for k in range(1, 14)] + [13.5, 14.0, 100.0]       # sixteen of them


def runs13_rows():
    rows = _strip(fs.runs()[0])
    i = np.arange(len(rows["iv_tid"]))
    rows["iv_val"] = (1 + (7 * i) % 13).astype(np.float64)
    return rows


def tile_aggregates(rows, thr):
    """what dt_tile_k writes: per tile of T rows and threshold the bases with val >= thr"""
    ln = rows["iv_end"].astype(np.int64) - rows["iv_start"]
    n = len(ln)
    return np.array([[int(ln[a:a + T][rows["iv_val"][a:a + T] >= t].sum()) for t in thr] for a in range(0, n, T)])


def runs13():
    """the runs with row i at value 1 + (7 i mod 13): a tile of 256 rows ends 9 rows into the cycle of 13, so every whole tile's
    aggregate differs per threshold and from every other tile's — a tile range that is off by one, or shifted, changes a count"""
    rows = runs13_rows()
    feats = fs.runs()[1]
    agg = tile_aggregates(rows, RUNS13_THR)
    whole = agg[:len(rows["iv_tid"]) // T]
    assert len(whole) >= 4
    for a in whole:
        assert all(x > y for x, y in zip(a[:13], a[1:14])) and a[13] == 0 and a[12] > 0          # differs per threshold
    assert len({tuple(a) for a in whole}) == len(whole)                                           # and from its neighbours
    for a, b in zip(whole, whole[1:]):
        assert sum(x != y for x, y in zip(a[:13], b[:13])) >= 6
    return rows, feats, RUNS13_THR, dict()


def search_edges():
    rows, feats, _ = fs.search_edges()
    return _strip(rows), feats, [1.0, 2.5, 5.0], dict(cells={(4, 0): 7, (4, 1): 7, (4, 2): 0})    # feature 4: the last row, value 3


def top():
    rows, feats, _ = fs.top()
    return _strip(rows), feats, [1.0, float(fs.TOP), float(fs.TOP) + 1.0], dict(cells={(0, 0): fs.TOP - 1, (0, 1): fs.TOP - 1, (0, 2): 0})


def _list(n):
    rows, feats, _ = fs.feature_list(n)
    return _strip(rows), feats, [2.0, 5.0, 9.5], dict()


SCENES = {"equal": equal, "nextafter": nextafter, "above_all": above_all, "below_all": below_all, "thirds": thirds, "runs13": runs13,
          "search_edges": search_edges, "top": top}
SCENES.update({"list%d" % n: (lambda n=n: _list(n)) for n in fs.LIST_N})
