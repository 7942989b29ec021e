"""zip members on the CPU wave emulator (tools/hipemu): the locate, inflate, walk, store and finish kernels of kc_zip.hip under the
host sequence of kc_zip_host.h in plain memory (kcemu_zip_read), over the reference's fixtures, the hand-built cases, the stored
shapes and the 480 mutations of tests/zip_cases.py — judged by tests/zip_model.py: bytes, status and layout of every member.  dst
carries 0xA5 guards on both sides; a call answered with "dst too small" writes nothing.  The full stored sweep (every size x every
name length) runs with KC_TEST_FULL=1."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_lib
import zip_cases as ZC
import zip_model as Z

GUARD = 64
FULL = os.environ.get("KC_TEST_FULL") == "1"


def _declare(L):
    from compress_amd import _lib
    vp = C.c_void_p
    L.kcemu_zip_read.restype = C.c_int
    L.kcemu_zip_read.argtypes = [vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, vp, vp]
    return L


@pytest.fixture(scope="module")
def emu():
    return _declare(C.CDLL(emu_lib.build()))


def table(members):
    from compress_amd import _lib
    t = (_lib.ZipMember * max(len(members), 1))()
    for k, m in enumerate(members):
        t[k].header_offset, t[k].compressed_size, t[k].uncompressed_size = m.header_offset, m.compressed_size, m.uncompressed_size
        t[k].crc32, t[k].method, t[k].flags, t[k].is_dir = m.crc32, m.method, m.flags, int(m.is_dir)
    return t


def call(L, data, members, dst, cap):
    """One emulated call: (return code, out_off, status); dst None = the layout alone."""
    n = len(members)
    src = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(0, dtype=np.uint8)   # exactly len(data) bytes: nothing behind them
    oo, st = np.zeros(n + 1, np.uint64), np.full(n + 1, 0xEE, np.uint32)
    t = table(members)
    d = None if dst is None else dst.ctypes.data + GUARD
    r = L.kcemu_zip_read(src.ctypes.data if len(src) else None, len(data), C.addressof(t), n, d, cap, oo.ctypes.data, st.ctypes.data)
    return r, oo, st[:n]


def run(L, data, members):
    """-> per member (bytes of its range, status), the layout's total"""
    r, oo0, st0 = call(L, data, members, None, 0)
    assert r == 0
    cap = int(oo0[-1])
    dst = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    r, oo, st = call(L, data, members, dst, cap)
    assert r == 0
    assert (dst[:GUARD] == 0xA5).all() and (dst[GUARD + cap:] == 0xA5).all(), "a write outside dst"
    assert (oo == oo0).all()
    for i in range(len(members)):   # the layout-only call knows the verdicts that need no decoding
        assert st0[i] in (Z.OK, st[i])
    return [(dst[GUARD + int(oo[i]):GUARD + int(oo[i + 1])].tobytes(), int(st[i])) for i in range(len(members))], cap


def judge(L, cases):
    bad = []
    for c in cases:
        ms = ZC.members_of(c)
        want, total = Z.read_all(c.data, ms)
        got, cap = run(L, c.data, ms)
        if cap != total or got != want:
            k = next((i for i in range(len(ms)) if got[i] != want[i]), -1)
            bad.append((c.name, "layout", cap, total, "member", k, None if k < 0 else (Z.NAMES.get(got[k][1], got[k][1]), len(got[k][0]), Z.NAMES[want[k][1]], len(want[k][0]))))
    assert not bad, (len(bad), bad[:10])


@emu_lib._fanned(min_bytes=1)
def _judge_many(items):
    L = _declare(C.CDLL(emu_lib.build()))
    by = _judge_many.cases
    judge(L, [by[bytes(x).decode()] for x in items])
    return [0] * len(items)


def judge_fanned(cases):
    """Independent cases in forked children, a share each (wall-clock time only)."""
    _judge_many.cases = {c.name: c for c in cases}
    _judge_many([c.name.encode() for c in cases])


def test_reference_fixtures(emu):
    judge(emu, ZC.fixture_cases())


def test_directed_cases(emu):
    cs = ZC.directed()
    judge(emu, cs)
    seen = set()
    for c in cs:
        for m in ZC.members_of(c):
            Z.member(c.data, m)
            seen |= Z.fired
    assert seen == ZC.ALL_RULES


def test_stored_shapes(emu):
    judge(emu, [ZC.stored_cases(FULL)])


def test_mutations(emu):
    cs = ZC.mutations()
    assert len(cs) == 480
    judge_fanned(cs)


def test_dst_too_small_writes_nothing(emu):
    by = {c.name: c for c in ZC.directed()}
    c = by["merged/two-archives"]
    ms = ZC.members_of(c) + ZC.members_of(by["hdr/negative-offset"])
    need = 700
    dst = np.full(need + 2 * GUARD, 0xA5, dtype=np.uint8)
    r, oo, _ = call(emu, c.data, ms, dst, need - 1)
    assert r == -2 and (dst == 0xA5).all() and [int(x) for x in oo] == [0, 300, 400, 700, 700, 700]
    r, _, st = call(emu, c.data, ms, dst, need)
    assert r == 0 and [int(s) for s in st] == [Z.OK] * 4 + [Z.READAT]


def test_no_members(emu):
    r, oo, st = call(emu, b"abc", [], None, 0)
    assert r == 0 and int(oo[0]) == 0
