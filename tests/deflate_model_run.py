"""tests/support/deflate_model.cpp's exact mode from python (test infrastructure): the model is compiled once per process with the host
compiler (`g++ ... -lz`, as test_deflate_model.py does) and run on a payload and its cuts; what comes back is, per member, the
kernel's parse as the model holds it — tokens, block type, deflate bytes, the bits the choice of block was made on and, when asked
for, every position's two candidates with their compared lengths."""
import atexit
import functools
import os
import shutil
import struct
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tokens: int = literal, (length, distance) = match; cand: None, or an (n, 4) array: the 4-byte table's candidate, the 8-byte table's
# (0xFFFF: none), their compared lengths
ModelMember = namedtuple("ModelMember", "n btype tokens deflate bits cand")


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="deflate_model_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "deflate_model")
    subprocess.run(["g++", "-O2", "-o", exe, os.path.join(ROOT, "tests", "support", "deflate_model.cpp"), "-lz"], check=True)
    return exe


def run(payload, cuts=None, want_tokens=True, want_candidates=False):
    """-> [ModelMember] (a member of no bytes: n = 0, nothing else).  The model itself inflates every member with zlib and fails
    when the payload does not come back."""
    payload = bytes(payload)
    if cuts is None:
        cuts = list(range(0, len(payload), 0xff00)) + [len(payload)]
    with tempfile.TemporaryDirectory(prefix="deflate_model_io_") as d:
        pp, cp, op = (os.path.join(d, x) for x in ("payload", "cuts", "out"))
        with open(pp, "wb") as f:
            f.write(payload)
        np.ascontiguousarray(cuts, dtype="<u8").tofile(cp)
        r = subprocess.run([_exe(), "candidates" if want_candidates else "tokens", pp, cp, op], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        with open(op, "rb") as f:
            raw = f.read()
    assert raw[:4] == b"DFTK"
    nmem, o = struct.unpack_from("<I", raw, 4)[0], 8
    assert nmem == len(cuts) - 1
    out = []
    for _ in range(nmem):
        n, btype, ntok, nbytes, bits = struct.unpack_from("<5I", raw, o)
        o += 20
        toks = None
        if want_tokens:
            t = np.frombuffer(raw, dtype="<u4", count=ntok, offset=o)
            toks = [(int(v >> 16 & 0x1FF), int(v & 0xFFFF) + 1) if v & 0x80000000 else int(v) for v in t]
        o += 4 * ntok
        z = raw[o:o + nbytes]
        o += nbytes
        cand = None
        if want_candidates:
            cand = np.frombuffer(raw, dtype="<u2", count=4 * n, offset=o).reshape(n, 4)
            o += 8 * n
        out.append(ModelMember(n, btype, toks, z, bits, cand))
    assert o == len(raw)
    return out
