"""A numpy float32 model of what the bigWig builders make of coverage rows: the data sections, the zoom plan and the zoom records,
written from the format and the rules of BigWigWriter::close (host/bigwig.cpp) rather than from its code's shape: plain loops over
(row, bin) pairs.  Every float operation is one correctly rounded float32 operation, in row order, as the writers do them.

model(scene) -> dict:
  levels   [{reduction (0: the data), n_items, sections [(chrom, start, end, payload bytes)]}], data first
  opens    per planned level (kept or dropped): the zoom records every row opens
  records  per kept level: [(chrom, start, end, valid, min, max, sum, sumsq)]
  per_bin  per kept level: the rows that feed each record
  dropped  levels the shrink rule discarded (0 or 1)
  covered  the bases the rows cover"""
import functools
import struct

import numpy as np

ITEMS = 1024
MAX_ZOOM = 10


def data_sections(tid, start, end, val):
    out, i, n = [], 0, len(tid)
    while i < n:
        j = i
        while j < n and j - i < ITEMS and tid[j] == tid[i]:
            j += 1
        p = struct.pack("<IIIIIBBH", int(tid[i]), int(start[i]), int(end[j - 1]), 0, 0, 1, 0, j - i)
        body = np.empty(j - i, dtype=[("s", "<u4"), ("e", "<u4"), ("v", "<f4")])
        body["s"], body["e"], body["v"] = start[i:j], end[i:j], val[i:j]
        out.append((int(tid[i]), int(start[i]), int(end[j - 1]), p + body.tobytes()))
        i = j
    return out


def zoom_level(tid, start, end, val, lens, red):
    """-> (records, opens per row, rows per record) at one reduction"""
    recs, opens, per_bin = [], [], []
    f32 = np.float32
    for t, s, e, v in zip(tid.tolist(), start.tolist(), end.tolist(), val):
        opened = 0
        b = s // red
        while b * red < e:
            bs, be = b * red, min((b + 1) * red, 0xFFFFFFFF)
            lo, hi = max(bs, s), min(be, e)
            if not recs or recs[-1][0] != t or recs[-1][1] != bs:
                recs.append([t, bs, min(be, max(int(lens[t]), hi)), 0, v, v, f32(0), f32(0)])
                per_bin.append(0)
                opened += 1
            r = recs[-1]
            w = f32(hi - lo)
            r[3] += hi - lo
            r[4] = v if v < r[4] else r[4]
            r[5] = v if r[5] < v else r[5]
            r[6] = f32(r[6] + f32(v * w))
            r[7] = f32(r[7] + f32(f32(v * v) * w))
            per_bin[-1] += 1
            b += 1
        opens.append(opened)
    return [tuple(r) for r in recs], opens, per_bin


def zoom_sections(recs):
    out, i, n = [], 0, len(recs)
    while i < n:
        j = i
        while j < n and j - i < ITEMS and recs[j][0] == recs[i][0]:
            j += 1
        p = b"".join(struct.pack("<IIIIffff", *r) for r in recs[i:j])
        out.append((recs[i][0], recs[i][1], recs[j - 1][2], p))
        i = j
    return out


def build(tid, start, end, val, lens):
    val = np.asarray(val, dtype=np.float32)
    n = len(tid)
    covered = int((end.astype(np.int64) - start.astype(np.int64)).sum())
    m = dict(levels=[dict(reduction=0, n_items=n, sections=data_sections(tid, start, end, val))], opens=[], records=[], per_bin=[], dropped=0,
             covered=covered)
    if n == 0:
        return m
    red = max(32, 4 * (covered // n + 1))
    z = 0
    while z < MAX_ZOOM and red < (1 << 31):
        recs, opens, per_bin = zoom_level(tid, start, end, val, lens, red)
        m["opens"].append(opens)
        if z > 0 and len(recs) * 2 > len(m["records"][-1]):
            m["dropped"] = 1
            break
        m["records"].append(recs)
        m["per_bin"].append(per_bin)
        m["levels"].append(dict(reduction=red, n_items=len(recs), sections=zoom_sections(recs)))
        if len(recs) < 1000:
            break
        z += 1
        red *= 4
    return m


@functools.lru_cache(maxsize=None)
def _model_of(name):
    from bigwig_scenes import by_name
    s = by_name(name)
    return build(s.tid, s.start, s.end, s.val, s.ref_len())


def model(scene):
    """the model of a scene, computed once and shared (treat it as read-only)"""
    return _model_of(scene.name)
