"""zlib inflate on the device (kc_zlib_inflate*, compress_amd.zlib): the cases of tests/zlib_cases.py — the ones the CPU wave
emulator runs (tests/test_emu_zlib.py) — device-resident with 64 guard bytes of 0xA5 on both sides of dst and through the
host-buffer forms: the directed cases, the 480 mutations, all 2000 wrapped seeded streams, the full Adler-32 sweep with 1 MiB and
4 MiB payloads, batches of mixed good and bad inputs, DST_TOO_SMALL, the scratch ceiling and the reader objects.
tests/zlib_model.py with stale_tables=False is the judge (tests/test_zlib_model.py holds it to the reference's vectors, to the
reference's inflate and to CPython's zlib); its verdicts are computed once on the host (zlib_cases.verdict)."""
import io
import struct
import zlib as host_zlib

import numpy as np
import pytest

import flate_cases as FC
import zlib_cases as ZC
import zlib_model as Z

pytestmark = pytest.mark.gpu
GUARD = 64


def pack(inputs):
    off = np.zeros(len(inputs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs])
    return np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy(), off


def batch_of(zdict=b""):
    from compress_amd import flate, zlib
    return flate.Batch("kc_zlib_inflate", zlib._ERRORS, dict=zdict or None)


def run_device(inputs, zdict=b"", cap=None):
    """One device-resident batch: dst sized by the sizing pass unless `cap` is given, 64 guard bytes of 0xA5 on both sides.
    -> (return code, per input (bytes of its range, status, consumed, bound, bound-only status))"""
    import torch
    from compress_amd import KcError
    b = batch_of(zdict)
    try:
        src, off = pack(inputs)
        d_src = torch.from_numpy(src).cuda(0)
        bound, bst, _ = b.bounds(d_src.data_ptr(), off, True)
        if cap is None:
            cap = int(bound.sum())
        d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert d_all.data_ptr() % 4 == 0
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
        want, cls, wused = ZC.verdict(c)
        if cls == Z.OK:
            ok = (got, st, used, bound, bst) == (want, Z.OK, wused, len(want), Z.OK)
        elif cls == Z.CHECKSUM:   # the sizing pass does not know the Adler-32: it plans the range, the write pass zero-fills it
            ok = (got, st, used, bound, bst) == (bytes(len(want)), cls, 0, len(want), Z.OK)
        else:                     # nothing decoded stays: an empty range
            ok = (got, st, used, bound, bst) == (b"", cls, 0, 0, cls)
        if not ok:
            bad.append((c.name, "model", Z.NAMES[cls], len(want), wused, "device", st, len(got), used, bound, bst))
    assert not bad, (len(bad), bad[:10])


def run_cases(cases):
    for zdict, cs in ZC.batches(cases):
        rc, res = run_device([c.data for c in cs], zdict)
        assert rc == 0
        judge(cs, res)


def test_directed_cases_device(kclib):
    run_cases(ZC.cases())


def test_mutations_device(kclib):
    run_cases(ZC.mutations())


def test_generated_cases_device(kclib):
    cs = ZC.generated()
    assert len(cs) == 2000
    run_cases(cs)


def host_results(b, cases):
    src, off = pack([c.data for c in cases])
    bound, bst, _ = b.bounds(src.ctypes.data, off, False)
    outs, used = b.all_host(src, off, with_consumed=True)
    return [((o if isinstance(o, bytes) else b""), (0 if isinstance(o, bytes) else o.status), int(u), int(s)) for o, u, s in zip(outs, used, bst)]


def judge_host(cases, results):
    """The host forms hand out bytes or an error: status, bytes and consumed."""
    bad = []
    for c, (got, st, used, bst) in zip(cases, results):
        want, cls, wused = ZC.verdict(c)
        ok = (got, st, used) == ((want, 0, wused) if cls == Z.OK else (b"", cls, 0)) and bst == (Z.OK if cls == Z.CHECKSUM else cls)
        if not ok:
            bad.append((c.name, Z.NAMES[cls], st, len(got), used, bst))
    assert not bad, (len(bad), bad[:10])


def test_host_buffer_forms(kclib):
    from compress_amd import zlib
    for cases in (ZC.cases(), ZC.mutations(), ZC.generated()):
        for zdict, cs in ZC.batches(cases):
            b = batch_of(zdict)
            try:
                judge_host(cs, host_results(b, cs))
            finally:
                b.close()
    cs = [c for c in ZC.cases() if not c.dict]
    names = [c.name for c in cs]
    src, off = pack([c.data for c in cs])
    outs = zlib.InflateAll(src, off)
    assert [o if isinstance(o, bytes) else o.status for o in outs] == [ZC.verdict(c)[0] if ZC.verdict(c)[1] == 0 else ZC.verdict(c)[1] for c in cs]
    assert isinstance(outs[names.index("trailer/one-bit")], zlib.ErrChecksum) and isinstance(outs[names.index("hdr/cinfo-8")], zlib.ErrHeader)
    assert isinstance(outs[names.index("fdict/none-given-id-other")], zlib.ErrDictionary) and outs[names.index("fdict/none-given-id-other")].name == "KC_FL_DICTIONARY"
    bound, status, used = zlib.InflateBounds(src, off)
    assert [int(s) for s in status] == [0 if ZC.verdict(c)[1] == Z.CHECKSUM else ZC.verdict(c)[1] for c in cs]
    c = next(c for c in ZC.cases() if c.name == "fdict/right-40000")
    assert zlib.InflateAll(*pack([c.data]), dict=c.dict) == [ZC.verdict(c)[0]]
    import torch
    d_src = torch.from_numpy(pack([c.data])[0]).cuda(0)
    d_dst = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    oo, st, used = zlib.InflateAllDevice(d_src.data_ptr(), [0, len(c.data)], d_dst.data_ptr(), 4096, dict=c.dict)
    assert (int(st[0]), int(used[0])) == (0, len(c.data)) and d_dst[:int(oo[1])].cpu().numpy().tobytes() == ZC.verdict(c)[0]


def big_cases():
    """1 MiB and 4 MiB of 0xFF and of random bytes, and a twin of each 1 MiB one with a trailer bit flipped: (first, case, payload,
    class).  Too long for the model: what zlib wrote decodes to what zlib read."""
    out = []
    for k, (n, fill) in enumerate(((1 << 20, "ff"), (1 << 20, "rand"), (4 << 20, "ff"), (4 << 20, "rand"))):
        payload = ZC.sweep_payload(n, fill)
        body = ZC._deflate_any(payload, fill)
        first = 1 + k % 3
        out.append((first, ZC.C("adler/len%d-%s-first%d" % (n, fill, first), ZC.wrap(body, payload)), payload, Z.OK))
        if n == 1 << 20:
            bad = struct.pack(">I", host_zlib.adler32(payload) ^ (1 << (7 + 13 * k)))
            out.append((first, ZC.C("adler/len%d-%s-first%d-bad" % (n, fill, first), ZC.wrap(body, payload, trailer=bad)), payload, Z.CHECKSUM))
    return out


def test_adler32_sweep_device(kclib):
    """The write pass's Adler-32 at every length x fill of the sweep, every range starting 1, 2 or 3 bytes behind a word boundary of
    dst (zlib_cases.layout), as ONE batch with the 1 MiB and 4 MiB payloads behind it; a trailer with one bit flipped is CHECKSUM and
    leaves the planned range zero-filled; 65521 bytes of 0xFF sum to the empty stream's 0x00000001."""
    sw = ZC.adler_sweep()
    big = big_cases()
    every = sw + [(f, c) for f, c, _, _ in big]
    sizes = [len(ZC.verdict(c)[0]) for _, c in sw] + [len(p) for _, _, p, _ in big]
    batch, at = ZC.layout(every, sizes)
    rc, res = run_device([c.data for c in batch])
    assert rc == 0
    judge([c for c in batch if c.name.startswith("head/")], [r for c, r in zip(batch, res) if c.name.startswith("head/")])
    judge([c for _, c in sw], [res[i] for i in at[:len(sw)]])
    start = np.cumsum([0] + [r[3] for r in res])
    assert [int(start[i]) % 4 for i in at] == [f for f, _ in every]
    for (first, c, payload, cls), i in zip(big, at[len(sw):]):
        want = (payload, Z.OK, len(c.data), len(payload), Z.OK) if cls == Z.OK else (bytes(len(payload)), Z.CHECKSUM, 0, len(payload), Z.OK)
        assert res[i] == want, c.name
    by = dict(zip((c.name for c in batch), res))
    for first in (1, 2, 3):
        assert by["%s-first%d" % (ZC.ADLER_WRAPS, first)][:2] == (b"\xff" * 65521, Z.OK)
        assert by["%s-first%d-bad" % (ZC.ADLER_WRAPS, first)][:2] == (bytes(65521), Z.CHECKSUM)


def mixed(n):
    """n inputs, good and bad, with a zero-length one among them."""
    pool = [c for c in ZC.cases() if not c.dict] + ZC.mutations()[:60]
    out = [pool[(i * 7) % len(pool)] for i in range(n)]
    if n > 1:
        out[n // 2] = ZC.C("mixed/zero-length", b"")
    return out


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_batches_of_mixed_inputs(kclib, n):
    cs = mixed(n)
    rc, res = run_device([c.data for c in cs])
    assert rc == 0
    judge(cs, res)
    if n > 1:
        assert {r[1] for r in res} >= {Z.OK, Z.EOF, Z.HEADER, Z.CHECKSUM}


def test_dst_too_small(kclib):
    from compress_amd import _lib
    cs = [c for c in ZC.cases() if c.name in ("cut/dynamic-whole", "trailer/one-bit", "hdr/cinfo-7")]
    assert len(cs) == 3
    need = sum(len(ZC.verdict(c)[0]) for c in cs)   # (the range of the one whose Adler-32 fails is planned too)
    assert run_device([c.data for c in cs], cap=need - 1)[0] == _lib.KC_ERR_DST_TOO_SMALL
    rc, res = run_device([c.data for c in cs], cap=need)
    assert rc == 0
    judge(cs, res)


def test_host_call_cut_into_groups(kclib):
    """KC_OPT_MAX_SCRATCH_MIB = 1: a quarter of it per group, so the batch goes in several groups, and an input that does not fit
    alone is KC_FL_SIZE_EXCEEDED with its neighbours untouched."""
    from compress_amd import _lib
    stored = next(c for _, c in ZC.adler_sweep() if c.name == "adler/len65535-rand-first1")
    cs = mixed(200) + [stored] * 6
    payload = bytes(300000)
    big = ZC.C("big", ZC.wrap(FC._deflate(payload, 6), payload))   # decodes to more than the quarter
    cs = cs[:100] + [big] + cs[100:]
    b = batch_of()
    try:
        b.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 1)
        res = host_results(b, cs)
        assert b.ctx().get_option(_lib.OPT_LAST_BATCHES) >= 2
    finally:
        b.close()
    assert res[100][:3] == (b"", Z.SIZE_EXCEEDED, 0)
    judge_host(cs[:100] + cs[101:], res[:100] + res[101:])


def test_readers(kclib):
    from compress_amd import zlib
    payload = bytes((i * i) >> 3 & 255 for i in range(3 << 20))
    raw = host_zlib.compress(payload, 6)
    out = io.BytesIO()
    r = zlib.NewReader(io.BytesIO(raw + b"behind"))
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
    co = host_zlib.compressobj(9, zdict=zd)
    with_dict = co.compress(b"a dictionary pays " * 9) + co.flush()
    assert with_dict[1] & 0x20
    rd = zlib.NewReaderDict(io.BytesIO(with_dict), zd)
    out = io.BytesIO()
    assert rd.WriteTo(out) == 18 * 9 and out.getvalue() == b"a dictionary pays " * 9
    rd.Reset(io.BytesIO(raw), zd)   # as a fresh NewReaderDict: the stream asks for no dictionary, and it is ignored
    assert rd.Read(mib) == 1 << 20 and bytes(mib) == payload[:1 << 20]
    buf = bytearray(64)
    with pytest.raises(zlib.ErrDictionary):
        zlib.NewReaderDict(io.BytesIO(with_dict), zd[:-1]).Read(buf)
    with pytest.raises(zlib.ErrDictionary):
        zlib.NewReader(io.BytesIO(with_dict)).Read(buf)
    with pytest.raises(zlib.ErrChecksum):
        zlib.NewReader(io.BytesIO(raw[:-1] + bytes([raw[-1] ^ 1]))).Read(buf)
    with pytest.raises(zlib.ErrHeader):
        zlib.NewReader(io.BytesIO(b"\x78\x9d" + raw[2:])).Read(buf)
    with pytest.raises(zlib.ErrUnexpectedEOF):
        zlib.NewReader(io.BytesIO(raw[:-1])).Read(buf)
    with pytest.raises(zlib.CorruptInputError):
        zlib.NewReader(io.BytesIO(b"\x78\x9c\x07")).Read(buf)
