"""zlib inflate on the CPU wave emulator (tools/hipemu): the sizing pass and the write pass of kc_zlib_size_kernel /
kc_zlib_write_kernel as one batch in plain memory (kcemu_zlib_inflate), over the cases of tests/zlib_cases.py — the directed ones,
the 480 mutations, the first 480 wrapped seeded streams, the Adler-32 sweep up to 65536 bytes — judged by tests/zlib_model.py with
stale_tables=False (what the device implements): bytes, status, consumed, bound and the sizing pass's status.  dst carries 0xA5
guards on both sides and stays untouched when the call fails."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import zlib_cases as ZC
import zlib_model as Z

GUARD = 64


def _declare(L):
    vp = C.c_void_p
    L.kcemu_zlib_inflate.restype = C.c_int
    L.kcemu_zlib_inflate.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def emu():
    return _declare(C.CDLL(emu_lib.build()))


def call(L, inputs, zdict, dst, cap):
    """One emulated batch: (return code, out_off, bound, status, consumed); dst None = the sizing pass alone."""
    n = len(inputs)
    src = np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy()
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs])
    oo, bd, st, cs = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.full(n + 1, 0xEE, np.uint32), np.zeros(n + 1, np.uint64)
    d = None if dst is None else dst.ctypes.data + GUARD
    dd = np.frombuffer(zdict + b"\0", dtype=np.uint8).copy()
    r = L.kcemu_zlib_inflate(src.ctypes.data, off.ctypes.data, n, dd.ctypes.data, len(zdict), d, cap, oo.ctypes.data, bd.ctypes.data, st.ctypes.data, cs.ctypes.data)
    return r, oo, bd[:n], st[:n], cs[:n]


def run_batch(L, inputs, zdict=b""):
    """-> per input (bytes of its range, status, consumed, bound, bound-only status)"""
    _, _, bd, bst, _ = call(L, inputs, zdict, None, 0)
    cap = int(bd.sum())
    dst = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    assert dst.ctypes.data % 4 == 0
    r, oo, bd2, st, cs = call(L, inputs, zdict, dst, cap)
    assert r == 0
    assert (dst[:GUARD] == 0xA5).all() and (dst[GUARD + cap:] == 0xA5).all(), "a write outside dst"
    assert int(oo[-1]) == cap and (bd == bd2).all()
    return [(dst[GUARD + int(oo[i]):GUARD + int(oo[i + 1])].tobytes(), int(st[i]), int(cs[i]), int(bd[i]), int(bst[i])) for i in range(len(inputs))]


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


@emu_lib._fanned(min_bytes=1)
def _emu_many(items, zdict=b""):
    """Independent inputs in forked children, a share each (wall-clock time only).  An item is a stream behind one byte `first`:
    0, or the bytes a head input puts in front of it in dst (then the two are a batch of their own)."""
    L = _declare(C.CDLL(emu_lib.build()))
    plain = [bytes(x[1:]) for x in items if x[0] == 0]
    res = iter(run_batch(L, plain, zdict)) if plain else iter(())
    return [next(res) if x[0] == 0 else run_batch(L, [ZC.head(x[0]).data, bytes(x[1:])], zdict)[1] for x in items]


def run_cases(cases):
    ZC.warm(cases)
    for zdict, cs in ZC.batches(cases):
        judge(cs, _emu_many([b"\0" + c.data for c in cs], zdict))


def test_directed_cases(emu):
    cases = ZC.cases()
    for zdict, cs in ZC.batches(cases):
        judge(cs, run_batch(emu, [c.data for c in cs], zdict))
    assert {ZC.verdict(c)[1] for c in cases} == {Z.OK, Z.CORRUPT, Z.EOF, Z.HEADER, Z.CHECKSUM, Z.DICTIONARY}


def test_mutations(emu):
    cs = ZC.mutations()
    assert len(cs) == 480
    run_cases(cs)


def test_generated_cases(emu):
    run_cases(ZC.generated()[:480])


def test_adler32_sweep(emu):
    """Every length x fill, the range starting 1, 2 and 3 bytes behind a word boundary of dst; the twins with one trailer bit flipped
    are CHECKSUM and leave their planned range zero-filled (judge); 65521 bytes of 0xFF sum to the empty stream's 0x00000001."""
    sw = ZC.adler_sweep()
    assert max(len(ZC.verdict(c)[0]) for _, c in sw) == 65536
    res = _emu_many([bytes([f]) + c.data for f, c in sw])
    judge([c for _, c in sw], res)
    by = dict(zip((c.name for _, c in sw), res))
    for first in (1, 2, 3):
        assert by["%s-first%d" % (ZC.ADLER_WRAPS, first)][:2] == (b"\xff" * 65521, Z.OK)
        assert by["%s-first%d-bad" % (ZC.ADLER_WRAPS, first)][:2] == (bytes(65521), Z.CHECKSUM)


def test_mixed_batch_of_65(emu):
    """65 inputs, good and bad, a zero-length one in the middle: one workgroup each, the neighbours of a failed one untouched."""
    pool = [c for c in ZC.cases() if not c.dict] + ZC.mutations()[:40]
    cs = [pool[(i * 7) % len(pool)] for i in range(65)]
    cs[32] = ZC.C("mixed/zero-length", b"")
    res = run_batch(emu, [c.data for c in cs])
    judge(cs, res)
    assert {r[1] for r in res} >= {Z.OK, Z.EOF, Z.HEADER, Z.CHECKSUM} and res[32][:2] == (b"", Z.EOF)


def test_dst_too_small_writes_nothing(emu):
    cs = [c for c in ZC.cases() if c.name in ("cut/dynamic-whole", "trailer/one-bit", "hdr/cinfo-7")]
    assert len(cs) == 3
    inputs = [c.data for c in cs]
    need = sum(len(ZC.verdict(c)[0]) for c in cs)   # (the range of the one whose Adler-32 fails is planned too)
    dst = np.full(need + 2 * GUARD, 0xA5, dtype=np.uint8)
    r, oo, _, _, _ = call(emu, inputs, b"", dst, need - 1)
    assert r == -2 and (dst == 0xA5).all() and int(oo[-1]) == need
    r, _, _, st, _ = call(emu, inputs, b"", dst, need)
    assert r == 0 and sorted(int(s) for s in st) == [Z.OK, Z.OK, Z.CHECKSUM]
