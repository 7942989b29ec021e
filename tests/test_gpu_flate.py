"""flate / gzip inflate on the device (kc_flate_inflate*, kc_gzip_inflate*, compress_amd.flate / compress_amd.gzip): the cases of
tests/flate_cases.py — the ones the CPU wave emulator runs (tests/test_emu_flate.py) — device-resident and through the host-buffer
forms, batches of mixed good and bad inputs, the scratch ceiling, DST_TOO_SMALL and the reader objects; the 2 x 2000 seeded
structured streams, the CRC-32 length sweep and the match-copy sweep.  tests/flate_model.py with stale_tables=False is the judge
(what the device implements; tests/test_ref_flate.py holds the model to the reference's own code on the same cases); its verdicts
are computed once on the host (flate_cases.verdict)."""
import io

import numpy as np
import pytest

import flate_cases as FC
import flate_model as M

pytestmark = pytest.mark.gpu
GUARD = 64


def pack(inputs):
    off = np.zeros(len(inputs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs])
    return np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy(), off


def batch_of(fmt, zdict=b"", multistream=True):
    from compress_amd import flate, gzip
    if fmt == "gzip":
        return flate.Batch("kc_gzip_inflate", gzip._ERRORS, multistream=multistream)
    return flate.Batch("kc_flate_inflate", flate._ERRORS, dict=zdict or None)


def run_device(inputs, fmt, zdict=b"", multistream=True, cap=None):
    """One device-resident batch: dst sized by the sizing pass unless `cap` is given, 64 guard bytes of 0xA5 on both sides.
    -> (return code, per input (bytes of its range, status, consumed, bound, bound-only status))"""
    import torch
    from compress_amd import KcError
    b = batch_of(fmt, zdict, multistream)
    try:
        src, off = pack(inputs)
        d_src = torch.from_numpy(src).cuda(0)
        bound, bst, _ = b.bounds(d_src.data_ptr(), off, True)
        if cap is None:
            cap = int(bound.sum())
        d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc = 0
        try:
            out_off, status, used = b.inflate(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap, True)
        except KcError as e:
            rc = e.status
        host = d_all.cpu().numpy()
    finally:
        b.close()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + cap:] == 0xA5), "written outside dst"
    if rc != 0:
        assert np.all(host == 0xA5), "dst touched by a call that failed"
        return rc, None
    assert int(out_off[-1]) == int(bound.sum())
    return 0, [(host[GUARD + int(out_off[i]):GUARD + int(out_off[i + 1])].tobytes(), int(status[i]), int(used[i]), int(bound[i]), int(bst[i]))
               for i in range(len(inputs))]


def judge(cases, results):
    bad = []
    for c, (got, st, used, bound, bst) in zip(cases, results):
        want, cls, wused = FC.verdict(c, stale_tables=False)
        if cls == M.OK:
            ok = (got, st, used, bound, bst) == (want, M.OK, wused, len(want), M.OK)
        else:  # nothing decoded stays: an empty range, or (gzip, behind complete members) a zero-filled one
            # (the sizing pass alone does not know a CRC-32: behind a wrong one it reports what it meets next, or nothing)
            ok = st == cls and used == 0 and got == bytes(len(got)) and bound == len(got) and (bst == cls or cls == M.CHECKSUM)
            if c.fmt == "flate":
                ok = ok and got == b""
        if not ok:
            bad.append((c.name, "model", M.NAMES[cls], len(want), wused, "device", st, len(got), used, bound, bst))
    assert not bad, bad[:10]


def test_directed_cases_device(kclib):
    for fmt, zdict, ms, cs in FC.batches(FC.cases()):
        rc, res = run_device([c.data for c in cs], fmt, zdict, ms)
        assert rc == 0
        judge(cs, res)


def test_mutations_device(kclib):
    fl, gz = FC.mutations()
    for cs in (fl, gz):
        rc, res = run_device([c.data for c in cs], cs[0].fmt)
        assert rc == 0
        judge(cs, res)


def test_large_streams_device(kclib):
    import corpora
    text = corpora.corpus("T", 32, 131072).tobytes()
    noise = np.random.default_rng(0xF1A7E).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    for fmt, zdict, ms, cs in FC.batches(FC.sized(text, noise)):
        want = {"size/noise": noise, "size/text-gzip": text[:1 << 20]}
        rc, res = run_device([c.data for c in cs], fmt)
        assert rc == 0
        for c, (got, st, used, bound, _) in zip(cs, res):  # (what zlib wrote decodes to what zlib read: no second walk by the model)
            assert (st, used, bound) == (0, len(c.data), len(got)) and got == want.get(c.name, text), c.name


def mixed(n):
    """n inputs, good and bad, with a zero-length one among them."""
    pool = [c for c in FC.cases() if c.fmt == "flate" and not c.dict and len(c.data) < 400]
    fl, _ = FC.mutations()
    pool += fl[:60]
    out = [pool[(i * 7) % len(pool)] for i in range(n)]
    if n > 1:
        out[n // 2] = FC.C("mixed/zero-length", b"")
    return out


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_batches_of_mixed_inputs(kclib, n):
    cs = mixed(n)
    rc, res = run_device([c.data for c in cs], "flate")
    assert rc == 0
    judge(cs, res)
    if n > 1:
        assert {r[1] for r in res} >= {M.OK, M.CORRUPT, M.EOF}


def test_dst_too_small(kclib):
    from compress_amd import _lib
    cs = [c for c in FC.cases() if c.name in ("fixed/len258-sym285", "stored/65535", "fixed/one-literal")]
    need = sum(len(FC.verdict(c)[0]) for c in cs)
    assert run_device([c.data for c in cs], "flate", cap=need - 1)[0] == _lib.KC_ERR_DST_TOO_SMALL
    gz = [c for c in FC.cases() if c.name in ("gzip/two-members", "gzip/flg-1e")]
    need = sum(len(FC.verdict(c)[0]) for c in gz)
    assert run_device([c.data for c in gz], "gzip", cap=need - 1)[0] == _lib.KC_ERR_DST_TOO_SMALL
    assert run_device([c.data for c in gz], "gzip", cap=need)[0] == 0


def test_one_gib_limit(kclib):
    """KC_FL_SIZE_EXCEEDED, the library's own limit of 1 GiB decoded per input, met by a match and by a literal: the sizing pass
    alone (nobody has to hold the GiB), device-resident.  The judge is arithmetic: flate_cases.at_the_limit says what a stream
    decodes to; a small stream of the same shape is also put before the model."""
    import torch
    small, n = FC.at_the_limit(5, 2)
    assert FC.verdict(FC.C("limit/shape", small)) == (bytes(1 + 258 * 5 + 2), M.OK, len(small))
    m = (FC.LIMIT - 1) // 258
    shapes = [(m, FC.LIMIT - 1 - 258 * m), (m, FC.LIMIT - 258 * m), (m + 1, 0), (5, 2)]   # exactly 1 GiB; one literal more; one match more
    streams = [FC.at_the_limit(*sh) for sh in shapes]
    assert [sz for _, sz in streams] == [FC.LIMIT, FC.LIMIT + 1, 1 + 258 * (m + 1), 1293] and streams[2][1] > FC.LIMIT
    inputs = [s for s, _ in streams]
    b = batch_of("flate")
    try:
        src, off = pack(inputs)
        bound, status, used = b.bounds(torch.from_numpy(src).cuda(0).data_ptr(), off, True)
    finally:
        b.close()
    assert [int(x) for x in status] == [M.OK, M.SIZE_EXCEEDED, M.SIZE_EXCEEDED, M.OK]
    assert [int(x) for x in bound] == [FC.LIMIT, 0, 0, 1293] and [int(x) for x in used] == [len(inputs[0]), 0, 0, len(inputs[3])]


def host_results(b, cases):
    src, off = pack([c.data for c in cases])
    bound, bst, _ = b.bounds(src.ctypes.data, off, False)
    outs, used = b.all_host(src, off, with_consumed=True)
    return [((o if isinstance(o, bytes) else b""), (0 if isinstance(o, bytes) else o.status), int(u), (len(o) if isinstance(o, bytes) else 0), int(s))
            for o, u, s in zip(outs, used, bst)]


def judge_host(cases, results):
    """The host forms hand out bytes or an error: status, bytes and consumed."""
    bad = []
    for c, (got, st, used, _, bst) in zip(cases, results):
        want, cls, wused = FC.verdict(c, stale_tables=False)
        ok = (got, st, used) == ((want, 0, wused) if cls == M.OK else (b"", cls, 0)) and (bst == cls or cls == M.CHECKSUM)
        if not ok:
            bad.append((c.name, M.NAMES[cls], st, len(got), used))
    assert not bad, bad[:10]


def test_host_buffer_forms(kclib):
    from compress_amd import flate, gzip
    for fmt, zdict, ms, cs in FC.batches(FC.cases()):
        b = batch_of(fmt, zdict, ms)
        try:
            judge_host(cs, host_results(b, cs))
        finally:
            b.close()
    fl = [c for c in FC.cases() if c.fmt == "flate" and not c.dict][:40]
    src, off = pack([c.data for c in fl])
    outs = flate.InflateAll(src, off)
    assert [o if isinstance(o, bytes) else o.status for o in outs] == [FC.verdict(c)[0] if FC.verdict(c)[1] == 0 else FC.verdict(c)[1] for c in fl]
    assert isinstance(outs[[c.name for c in fl].index("stored/len-nlen-mismatch")], flate.CorruptInputError)
    zeros = FC._deflate(bytes(1 << 20), 9)   # 1000 : 1, far above the first guess of the helper's own buffer: the second call
    assert flate.InflateAll(np.frombuffer(zeros, dtype=np.uint8), [0, len(zeros)]) == [bytes(1 << 20)]
    bound, status, used = flate.InflateBounds(src, off)
    assert [int(s) for s in status] == [FC.verdict(c)[1] for c in fl]
    gzs = [c for c in FC.cases() if c.fmt == "gzip" and c.multistream]
    src, off = pack([c.data for c in gzs])
    outs = gzip.GunzipAll(src, off)
    names = [c.name for c in gzs]
    assert isinstance(outs[names.index("gzip/bad-crc32")], gzip.ErrChecksum) and isinstance(outs[names.index("gzip/wrong-magic")], gzip.ErrHeader)
    assert outs[names.index("gzip/two-members")] == b"hello, " + b"world" * 100
    bound, status, used = gzip.GunzipBounds(src, off)
    assert int(bound[names.index("gzip/two-members")]) == 507 and int(used[names.index("gzip/two-members")]) == len(gzs[names.index("gzip/two-members")].data)


def test_generated_cases_device(kclib):
    """generated(seed, 2000) raw and as gzip members, one launch per batch (format, dictionary, Multistream), device-resident."""
    for cases in (FC.generated(), FC.generated_gzip()):
        assert len(cases) == 2000
        for fmt, zdict, ms, cs in FC.batches(cases):
            rc, res = run_device([c.data for c in cs], fmt, zdict, ms)
            assert rc == 0
            judge(cs, res)


def test_generated_cases_host_forms(kclib):
    for cases in (FC.generated(), FC.generated_gzip()):
        for fmt, zdict, ms, cs in FC.batches(cases):
            b = batch_of(fmt, zdict, ms)
            try:
                judge_host(cs, host_results(b, cs))
            finally:
                b.close()


def test_crc32_length_sweep_device(kclib):
    """The write pass's CRC-32 at the lengths where its split over the lanes changes (flate_cases.crc_sweep), the member's bytes at
    every residue mod 4 in dst; a trailer CRC with one bit flipped is CHECKSUM and leaves the planned range zero-filled."""
    cs = FC.crc_sweep()
    rc, res = run_device([c.data for c in cs], "gzip")
    assert rc == 0
    judge(cs, res)
    by_name = dict(zip((c.name for c in cs), res))
    for n in FC.CRC_SWEEP_TWINS:
        for first in (1, 2, 3):
            got, st = by_name["crc/len%d-first%d-bad-crc" % (n, first)][:2]
            assert (got, st) == (bytes(first + n), M.CHECKSUM)
    assert {(len(FC.verdict(c)[0])) for c in cs if FC.verdict(c)[1] == M.OK} >= {1 + 65535, 3 + 512, 2 + 769}


def test_match_copy_sweep_device(kclib):
    cs = FC.copy_sweep()
    assert all(FC.verdict(c)[1] == M.OK for c in cs)
    for fmt, zdict, ms, b in FC.batches(cs):
        rc, res = run_device([c.data for c in b], fmt, zdict, ms)
        assert rc == 0
        judge(b, res)


def test_host_call_cut_into_groups(kclib):
    """KC_OPT_MAX_SCRATCH_MIB = 1: a quarter of it per group, so the batch goes in several groups, and an input that does not fit
    alone is KC_FL_SIZE_EXCEEDED with its neighbours untouched."""
    from compress_amd import _lib
    cs = mixed(200) + [c for c in FC.cases() if c.name == "stored/65535"] * 6
    big = FC.C("big", FC._deflate(bytes(300000), 6))   # decodes to more than the quarter
    cs = cs[:100] + [big] + cs[100:]
    b = batch_of("flate")
    try:
        b.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 1)
        res = host_results(b, cs)
        assert b.ctx().get_option(_lib.OPT_LAST_BATCHES) >= 2
    finally:
        b.close()
    assert res[100][:3] == (b"", M.SIZE_EXCEEDED, 0)
    judge_host(cs[:100] + cs[101:], res[:100] + res[101:])


def test_readers(kclib):
    from compress_amd import flate, gzip
    payload = bytes((i * i) >> 3 & 255 for i in range(3 << 20))
    raw = FC._deflate(payload, 6)
    out = io.BytesIO()
    r = flate.NewReader(io.BytesIO(raw))
    assert r.WriteTo(out) == len(payload) and out.getvalue() == payload and r.consumed == len(raw)
    r.Reset(io.BytesIO(raw))
    got = bytearray()
    one = bytearray(1)
    for _ in range(1000):       # 1-byte pieces
        assert r.Read(one) == 1
        got += one
    mib = bytearray(1 << 20)    # 1 MiB pieces
    while True:
        n = r.Read(mib)
        if n == 0:
            break
        got += mib[:n]
    assert bytes(got) == payload
    r.Close()
    zd = b"a dictionary " * 20
    rd = flate.NewReaderDict(io.BytesIO(FC._deflate(b"a dictionary pays " * 9, 9, zdict=zd)), zd)
    out = io.BytesIO()
    assert rd.WriteTo(out) == 18 * 9 and out.getvalue() == b"a dictionary pays " * 9
    with pytest.raises(flate.CorruptInputError):
        flate.NewReader(io.BytesIO(b"\x07")).Read(bytearray(8))
    two = FC.gz_member(payload[:100000], flg=0x1e, extra=b"EX", name=b"n\xe4me", comment=b"cmt") + FC.gz_member(b"second")
    g = gzip.NewReader(io.BytesIO(two))
    out = io.BytesIO()
    assert g.WriteTo(out) == 100006 and out.getvalue() == payload[:100000] + b"second"
    h = g.Header
    assert (h.Name, h.Comment, h.Extra, h.ModTime, h.OS) == ("näme", "cmt", b"EX", 1234567890, 3)
    g.Reset(io.BytesIO(two))
    g.Multistream(False)
    buf = bytearray(1 << 20)
    assert g.Read(buf) == 100000 and g.Read(buf) == 0 and g.consumed == len(two) - len(FC.gz_member(b"second"))
    with pytest.raises(gzip.ErrChecksum):
        gzip.NewReader(io.BytesIO(FC.gz_member(b"hello", crc=7))).Read(buf)
    with pytest.raises(gzip.ErrHeader):
        gzip.NewReader(io.BytesIO(b"\x1f\x8b\x07" + bytes(20))).Read(buf)
