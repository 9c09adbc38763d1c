"""A plain model of tbk_cov_stream_push (include/tbk.h): the ends of a tile's records, the bundle heads of carry ++ tile,
the last head, the view and the new carry.  Python lists and numpy only; importable without a GPU.  Written from the header's contract
and tiecov's bundle rule, one record at a time; it shares no code with the kernels (tiebrush_amd/csrc/stream.hip).

A record is the tuple cov_scenes.mk() takes — (tid, pos, flag, [(len, op) ...], yc, strand) — plus its YX; a tile is a soa.CovInput."""
import numpy as np

import cov_scenes as cs

REF_OPS = (0, 2, 3, 7, 8)     # M D N = X take reference bases (GSamRecord::setupCoordinates)


def end_of(rec):
    """1-based inclusive end by the coverage path's rule: pos + the reference length of the CIGAR (pos itself for a CIGAR without one)"""
    return rec[1] + sum(ln for ln, op in rec[3] if op in REF_OPS)


def heads(recs):
    """head flag of every record of a list of MAPPED records: the first of a tid run, or start > the running maximum of end over the
    records of the run before it (tiecov.cpp:443)"""
    out, tid, mx = [], None, None
    for r in recs:
        start = r[1] + 1
        h = tid is None or r[0] != tid or start > mx
        if tid is None or r[0] != tid:
            tid, mx = r[0], end_of(r)
        else:
            mx = max(mx, end_of(r))
        out.append(h)
    return out


def tile_records(cin, seen=None):
    """the records of a tile with the weights the view gives them: YC / YX where `seen` (bit 0 / bit 1 per record; None: everywhere) says
    the tag is present, 1.0 / 1 where not (tbk_region_view's rule)"""
    out = []
    for i, r in enumerate(cs.records(cin)):
        sn = 3 if seen is None else int(seen[i])
        yc = r[4] if (sn & 1) else 1.0
        yx = (int(cin.yx[i]) if cin.yx is not None else 1) if (sn & 2) else 1
        out.append(((r[0], r[1], r[2], r[3], yc, r[5]), yx))
    return out


def to_cin(recs_yx):
    return cs.mk([r for r, _ in recs_yx], [y for _, y in recs_yx])


class Stream:
    """the carry between pushes"""

    def __init__(self):
        self.carry = []       # [(record, yx)]: the open bundle

    def reset(self):
        self.carry = []

    def push(self, cin, final, seen=None):
        """-> (view as [(record, yx)], info dict) and the new self.carry"""
        recs = tile_records(cin, seen)
        n = len(recs)
        mapped = [(i, r) for i, r in enumerate(recs) if not (r[0][2] & 4)]
        seq = self.carry + [r for _, r in mapped]
        nc = len(self.carry)
        hd = heads([r for r, _ in seq])
        last = max((j for j, h in enumerate(hd) if h), default=None)
        if final:
            view, carry, cut = seq, [], n
        elif last is None or last < nc:
            view, carry, cut = [], seq, 0
        else:
            view, carry, cut = seq[:last], seq[last:], mapped[last - nc][0]
        self.carry = carry
        n_taken = max(len(view) - nc, 0)
        return view, dict(n_view=len(view), n_carry=len(carry), n_taken=n_taken, cut=cut)


def run(pushes):
    """[(tile, final, seen)] -> [(view, info)] of one stream from an empty carry, and the carry that is left"""
    s = Stream()
    out = [s.push(cin, final, seen) for cin, final, seen in pushes]
    return out, s.carry


def uncut(pushes):
    """the mapped records of the whole stream as one input: what the views must add up to"""
    recs = []
    for cin, _, seen in pushes:
        recs += [r for r in tile_records(cin, seen) if not (r[0][2] & 4)]
    return to_cin(recs)
