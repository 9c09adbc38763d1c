"""The rule of tbk_cov_split_strand (include/tbk.h) as a plain loop, and the text of a part's coverage track.  numpy only;
importable without a GPU.

split(cin) -> [part of '+', part of '-', part of every other strand byte]: the mapped records (flag bit 0x4 clear; flag None: all) of
each class in the input's order, every column copied bit for bit, the CIGAR CSR rebuilt from 0, flag None.  It shares no code with
api.split_strand_host (vectorised) or tbh::split_strand_host (C++); tests/test_strand_model_cpu.py holds the three against each other."""
import numpy as np

from tiebrush_amd import soa

CLASSES = ("plus", "minus", "none")
COLS = (("tid", np.int32), ("pos", np.int32), ("cig_off", np.uint32), ("cig", np.uint32), ("yc", np.float64), ("strand", np.uint8), ("yx", np.int64))
HEADER = b"track type=bedGraph\n"


def classify(strand_byte):
    return 0 if strand_byte == ord("+") else (1 if strand_byte == ord("-") else 2)


def split(cin):
    n = cin.n_records
    rec = [[], [], []]
    for i in range(n):
        if cin.flag is not None and (int(cin.flag[i]) & 4):
            continue
        rec[classify(int(cin.strand[i]))].append(i)
    out = []
    for idx in rec:
        off, words = [0], []
        for i in idx:
            w = cin.cig[int(cin.cig_off[i]):int(cin.cig_off[i + 1])]
            words.extend(int(x) for x in w)
            off.append(len(words))
        idx = np.asarray(idx, np.int64)
        out.append(soa.CovInput(tid=np.asarray(cin.tid, np.int32)[idx], pos=np.asarray(cin.pos, np.int32)[idx], flag=None,
                                cig_off=np.asarray(off, np.uint32), cig=np.asarray(words, np.uint32),
                                yc=None if cin.yc is None else np.asarray(cin.yc, np.float64)[idx], strand=np.asarray(cin.strand, np.uint8)[idx],
                                yx=None if cin.yx is None else np.asarray(cin.yx, np.int64)[idx]))
    return out


def for_oracle(part):
    """a part as the oracle reads it: the oracle wants a flag column (the views carry none: every record is mapped)"""
    return soa.CovInput(part.tid, part.pos, np.zeros(part.n_records, np.uint16), part.cig_off, part.cig, part.yc, part.strand, part.yx)


def same(a, b):
    """None when two CovInput hold the same bytes in every column (yc compared as raw 64 bits), else the first column that differs"""
    for k, dt in COLS + (("flag", np.uint16),):
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None):
            return k
        if x is not None and np.ascontiguousarray(x, dtype=dt).tobytes() != np.ascontiguousarray(y, dtype=dt).tobytes():
            return k
    return None


def cov_text(rows, names, header=True):
    """the bytes of `tiecov -c` for the interval rows of a coverage call (tiecov.cpp:91-95)"""
    out = [HEADER] if header else []
    for t, s, e, v in zip(rows["iv_tid"], rows["iv_start"], rows["iv_end"], rows["iv_val"]):
        out.append(b"%s\t%d\t%d\t%.3f\n" % (names[int(t)].encode() if isinstance(names[int(t)], str) else names[int(t)], int(s), int(e), float(v)))
    return b"".join(out)


def per_base(rows, tid_len):
    """interval rows spread per base: {tid: float64 array}"""
    out = {t: np.zeros(ln, np.float64) for t, ln in tid_len.items()}
    for t, s, e, v in zip(rows["iv_tid"], rows["iv_start"], rows["iv_end"], rows["iv_val"]):
        out[int(t)][int(s):int(e)] += float(v)
    return out
