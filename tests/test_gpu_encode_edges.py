"""The record layer of the device writer (bgzdef.hip: enc_plan_k, enc_emit_k, enc_maxlen_k, enc_strip_k, enc_cuts_k, enc_members_k)
and the index front end that bisects its member cuts (baix.hip: ix_rec_k) on the hand-built scenes of enc_scenes.py, against the
plain model of enc_model.py and the restatements of the index contract (bai_reader.py, csi_reader.py).  Every comparison is exact.
test_enc_scenes_cpu.py holds the scenes to their claims, and the model to the host writer, before the GPU is asked."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bai_reader as br
import bam_craft as bc
import enc_model as em
import enc_scenes as es
from test_gpu_csi import check_part as check_csi_part
from test_gpu_deflate import check_run, members
from test_gpu_encode import members_begin_with_records
from test_gpu_index import BIN, _split_header, check_part

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tiebrush_amd import api
    c = api.Context(0)
    yield c
    c.close()


def member_sizes(run):
    return [isize for _, _, isize in members(run)]


def _host(recs):
    return dict(enumerate(recs))


@pytest.mark.parametrize("name", list(es.SCENES))
def test_scene_by_the_host_hand_over(ctx, name):
    recs, yc, yx, yd, ref_len, _ = es.get(name)
    n = len(recs)
    rep = np.arange(n, dtype=np.uint32)
    want = em.stream(recs, yc, yx, yd)
    run, pay = ctx.bam_encode(rep, yc, yx, yd, n_dev=0, host_records=_host(recs))
    got = gzip.decompress(run)
    if got != want:                                                    # say which record differs
        o = 0
        for i, ln in enumerate(es.lengths(es.get(name))):
            assert got[o:o + ln] == want[o:o + ln], (i, yc[i], yx[i], yd[i], recs[i][em.aux_start(recs[i]):])
            o += ln
    assert got == want and pay == len(want)
    check_run(run, want)
    members_begin_with_records(run)
    assert member_sizes(run) == em.cuts(es.lengths(es.get(name)))[2]
    # the same call with the run's index part: the same bytes, and every record's virtual offset in the member that holds it
    run_i, pay_i, part = ctx.bam_encode_indexed(rep, yc, yx, yd, ref_len, n_dev=0, host_records=_host(recs))
    assert run_i == run and pay_i == pay
    check_part(run, part, ref_len)
    if name in es.WITH_CSI:
        run_c, _, part_c = ctx.bam_encode_indexed(rep, yc, yx, yd, ref_len, n_dev=0, host_records=_host(recs), csi_depth=5)
        assert run_c == run
        check_csi_part(run, part_c, ref_len, 5)


@pytest.mark.parametrize("name", es.DEVICE_TILE)
def test_scene_as_a_device_decoded_tile(ctx, name):
    """the records read where tbk_bam_decode left them (another source alignment for the 16-lane copy: the file's header is in front of
    them), and half of them from there, half from the host"""
    recs, yc, yx, yd, ref_len, _ = es.get(name)
    n = len(recs)
    rep = np.arange(n, dtype=np.uint32)
    want = em.stream(recs, yc, yx, yd)
    sizes = em.cuts(es.lengths(es.get(name)))[2]
    bam = bc.by_member(bc.header_bytes() + b"".join(struct.pack("<I", len(r)) + r for r in recs))
    s, _ = ctx.bam_decode([bam])
    try:
        assert int(s.n_records) == n
        run, pay = ctx.bam_encode(rep, yc, yx, yd, n_dev=n)
        assert gzip.decompress(run) == want and pay == len(want)
        check_run(run, want)
        assert member_sizes(run) == sizes
        half = n // 2
        run2, _ = ctx.bam_encode(rep, yc, yx, yd, n_dev=half, host_records={i: recs[i] for i in range(half, n)})
        assert gzip.decompress(run2) == want
        assert member_sizes(run2) == sizes
        run3, _, part = ctx.bam_encode_indexed(rep, yc, yx, yd, ref_len, n_dev=n)
        assert run3 == run
        check_part(run, part, ref_len)
    finally:
        ctx.bam_release()


@pytest.mark.parametrize("name", list(es.REFUSALS))
def test_a_record_too_long_for_a_member_is_refused(ctx, name):
    """TBK_EUNSUPPORTED from the real length, no test hook: 65025 bytes, and a record that fits until its tags are appended; the context
    encodes the longest accepted record right after"""
    from tiebrush_amd.api import TbkError
    recs, yc, yx, yd, ref_len, _ = es.get(name)
    for indexed in (False, True):
        with pytest.raises(TbkError) as e:
            if indexed:
                ctx.bam_encode_indexed(np.arange(1, dtype=np.uint32), yc, yx, yd, ref_len, n_dev=0, host_records=_host(recs))
            else:
                ctx.bam_encode(np.arange(1, dtype=np.uint32), yc, yx, yd, n_dev=0, host_records=_host(recs))
        assert e.value.status == em.EUNSUPPORTED
        for ok in ("one_record/long", "one_record/short"):
            r, c, x, d, rl, _ = es.get(ok)
            run, pay, part = ctx.bam_encode_indexed(np.arange(1, dtype=np.uint32), c, x, d, rl, n_dev=0, host_records=_host(r))
            assert gzip.decompress(run) == em.stream(r, c, x, d) and pay == 4 + len(em.tag(r[0], c[0], x[0], d[0]))
            check_part(run, part, rl)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _inputs(d, long_raw):
    """three coordinate-sorted inputs of 40 records, every record a group of its own; one record of long_raw bytes among short ones"""
    paths = []
    for k in range(3):
        recs = []
        for i in range(40):
            pos = 100 + 30 * i + 10 * k
            if k == 1 and i == 17:
                r = es.sized(long_raw, pos, name=b"long_read", cigar=((40000, es.M),), aux=b"NHC\x01")
            else:
                r = es.sized(90 + (i * 7 + k) % 40, pos, name=b"s%d_%d" % (k, i), cigar=((50, es.M),), aux=b"NHC\x01")
            recs.append(struct.pack("<I", len(r)) + r)
        paths.append(os.path.join(d, "in%d.bam" % k))
        with open(paths[-1], "wb") as fh:
            fh.write(bc.by_member(bc.header_bytes() + b"".join(recs)))
    return paths


def _clean_env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TBK_TEST")}
    env.update(kw)
    return env


def _tiebrush(outdir, writer, inputs, extra=(), **env):
    os.makedirs(outdir, exist_ok=True)
    r = subprocess.run([os.path.join(BIN, "tiebrush"), "-o", "o.bam", "--writer", writer] + list(extra) + inputs, capture_output=True, text=True,
                       env=_clean_env(**env), cwd=outdir)
    return r, os.path.join(outdir, "o.bam")


def _record_stream(path):
    return gzip.decompress(_split_header(open(path, "rb").read())[1])


def test_cli_a_long_read_among_short_ones(tmp_path):
    """a record of 60 kB (l_seq about 40000): B drops to about 5 kB and the ranges inside the long record are empty; both writers, the
    same records, and each file's index the restatement of that file"""
    ins = _inputs(str(tmp_path), 60000)
    streams = {}
    for w in ("device", "host"):
        r, p = _tiebrush(str(tmp_path / w), w, ins, ["--index"], TBK_TIMING="1")
        assert r.returncode == 0, r.stderr
        assert ("device writer:" in r.stderr) == (w == "device") and "device writer stopped" not in r.stderr, r.stderr[-600:]
        data, bai = open(p, "rb").read(), open(p + ".bai", "rb").read()
        assert bai == br.expected_bai(data)
        br.validate(data, bai)
        streams[w] = _record_stream(p)
        assert len(br.read_bam(data)[2]) == 120
    assert streams["device"] == streams["host"]
    o, longest = 0, 0
    while o < len(streams["device"]):
        bs = struct.unpack_from("<I", streams["device"], o)[0]
        longest, o = max(longest, 4 + bs), o + 4 + bs
    assert 60000 < longest <= em.LONGEST


def test_cli_a_record_the_device_writer_cannot_take(tmp_path):
    """one record whose tagged length exceeds 65024: the device writer refuses its chunk by the record's real length (no test hook in the
    environment) and the host writer takes the output over"""
    ins = _inputs(str(tmp_path), em.LONGEST + 60)
    rd, d = _tiebrush(str(tmp_path / "device"), "device", ins, TBK_TIMING="1")
    assert rd.returncode == 0, rd.stderr
    assert "host writer" in rd.stderr, rd.stderr[-600:]
    rh, h = _tiebrush(str(tmp_path / "host"), "host", ins)
    assert rh.returncode == 0, rh.stderr
    assert _record_stream(d) == _record_stream(h)
    data = open(d, "rb").read()
    assert len(br.read_bam(data)[2]) == 120
