"""flate / gzip inflate on the CPU wave emulator (tools/hipemu): the sizing pass, the scan and the write pass of
compress_amd/csrc/kc_flate_inflate.hip as one batch in plain memory (kcemu_flate_inflate / kcemu_gzip_inflate), over every case of
tests/flate_cases.py — the directed shapes, the 2 x 480 mutations, the first 480 seeded structured streams raw and as gzip, the
CRC-32 length sweep, the match-copy sweep, the large streams — judged by tests/flate_model.py with stale_tables=False (what the
device implements; tests/test_ref_flate.py holds the model to the reference on the same cases): status, bytes, consumed and bound.
dst carries 0xA5 guards on both sides and stays untouched when the call fails."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import flate_cases as FC
import flate_model as M

GUARD = 64


def _declare(L):
    vp = C.c_void_p
    L.kcemu_flate_inflate.restype = C.c_int
    L.kcemu_flate_inflate.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp]
    L.kcemu_gzip_inflate.restype = C.c_int
    L.kcemu_gzip_inflate.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, C.c_uint64, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def emu():
    return _declare(C.CDLL(emu_lib.build()))


def call(L, inputs, fmt, zdict, multistream, dst, cap):
    """One emulated batch: (return code, out_off, bound, status, consumed); dst None = the sizing pass alone."""
    n = len(inputs)
    src = np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy()
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs])
    oo, bd, st, cs = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.full(n + 1, 0xEE, np.uint32), np.zeros(n + 1, np.uint64)
    d = None if dst is None else dst.ctypes.data + GUARD
    if fmt == "gzip":
        r = L.kcemu_gzip_inflate(src.ctypes.data, off.ctypes.data, n, int(multistream), d, cap, oo.ctypes.data, bd.ctypes.data, st.ctypes.data, cs.ctypes.data)
    else:
        dd = np.frombuffer(zdict + b"\0", dtype=np.uint8).copy()
        r = L.kcemu_flate_inflate(src.ctypes.data, off.ctypes.data, n, dd.ctypes.data, len(zdict), d, cap, oo.ctypes.data, bd.ctypes.data, st.ctypes.data, cs.ctypes.data)
    return r, oo, bd[:n], st[:n], cs[:n]


def run_batch(L, inputs, fmt, zdict, multistream):
    """-> per input (bytes of its range, status, consumed, bound, bound-only status)"""
    _, _, bd, bst, bcs = call(L, inputs, fmt, zdict, multistream, None, 0)
    cap = int(bd.sum())
    dst = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    r, oo, bd2, st, cs = call(L, inputs, fmt, zdict, multistream, dst, cap)
    assert r == 0
    assert (dst[:GUARD] == 0xA5).all() and (dst[GUARD + cap:] == 0xA5).all(), "a write outside dst"
    assert int(oo[-1]) == cap and (bd == bd2).all()
    return [(dst[GUARD + int(oo[i]):GUARD + int(oo[i + 1])].tobytes(), int(st[i]), int(cs[i]), int(bd[i]), int(bst[i])) for i in range(len(inputs))]


def judge(cases, results):
    bad = []
    for c, (got, st, used, bound, bst) in zip(cases, results):
        want, cls, wused = FC.verdict(c, stale_tables=False)
        if cls == M.OK:
            ok = (got, st, used, bound, bst) == (want, M.OK, wused, len(want), M.OK)
        else:  # nothing decoded stays: an empty range, or a zero-filled one
            # (the sizing pass alone does not know a CRC-32: behind a wrong one it reports what it meets next, or nothing)
            ok = st == cls and used == 0 and got == bytes(len(got)) and bound == len(got) and (bst == cls or cls == M.CHECKSUM)
            if c.fmt == "flate":
                ok = ok and got == b""
        if not ok:
            bad.append((c.name, "model", M.NAMES[cls], len(want), wused, "device", st, len(got), used, bound, bst))
    assert not bad, bad[:10]


def run_cases(L, cases):
    for fmt, zdict, ms, cs in FC.batches(cases):
        judge(cs, run_batch(L, [c.data for c in cs], fmt, zdict, ms))


def test_directed_cases(emu):
    cases = FC.cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    run_cases(emu, cases)


def test_budget_changes_nothing(emu):
    """The directed cases under a scratch budget of one byte: the device form of inflate keeps no scratch that grows with its inputs'
    bytes, so it has no cut to make and no input to refuse — every batch is one device batch, whatever the budget, with the same
    bytes, layout, statuses, consumed and bounds.  (The cuts of the inflate entry points are the host-buffer form's two sweeps.)"""
    for fmt, zdict, ms, cs in FC.batches(FC.cases()):
        inputs = [c.data for c in cs]
        one = run_batch(emu, inputs, fmt, zdict, ms)
        assert emu_lib.last_batches() == 1
        with emu_lib.scratch_budget(1):
            cut = run_batch(emu, inputs, fmt, zdict, ms)
            assert emu_lib.last_batches() == 1
        assert cut == one
        judge(cs, cut)


@emu_lib._fanned(min_bytes=1)
def _emu_many(items, fmt, zdict=b"", multistream=True):
    """Independent inputs of one format in forked children, a share each (wall-clock time only)."""
    L = _declare(C.CDLL(emu_lib.build()))
    return run_batch(L, [bytes(x) for x in items], fmt, zdict, multistream)


def run_cases_fanned(cases):
    FC.warm(cases)
    for fmt, zdict, ms, cs in FC.batches(cases):
        judge(cs, _emu_many([c.data for c in cs], fmt, zdict, ms))


def test_generated_cases(emu):
    """The first 480 seeded structured streams, raw and as gzip members: the share that holds 60 stale shapes per table (an empty
    table behind a used one: CORRUPT here, whatever the reference reads through it) and the codes longer than the primary tables."""
    fl, gz = FC.generated()[:480], FC.generated_gzip()[:480]
    for tag in ("stale-dist", "stale-lit", "stale-clen"):
        assert sum(1 for c in fl if tag in c.name) == 60
    for tag in ("longL", "longD"):
        assert sum(1 for c in fl if tag in c.name.split("/", 2)[2].split("+") and FC.verdict(c)[1] == M.OK) >= 30
    run_cases_fanned(fl)
    run_cases_fanned(gz)


def test_crc32_length_sweep(emu):
    cs = FC.crc_sweep()
    assert len(cs) == 3 * len(FC.CRC_SWEEP_LENGTHS) + 3 * len(FC.CRC_SWEEP_TWINS)
    run_cases_fanned(cs)
    res = dict(zip((c.name for c in cs), _emu_many([c.data for c in cs], "gzip")))
    for n in FC.CRC_SWEEP_TWINS:
        for first in (1, 2, 3):
            got, st = res["crc/len%d-first%d-bad-crc" % (n, first)][:2]
            assert (got, st) == (bytes(first + n), M.CHECKSUM)


def test_match_copy_sweep(emu):
    cs = FC.copy_sweep()
    assert len(cs) == 12 * 8 * 2 and all(FC.verdict(c)[1] == M.OK for c in cs)
    run_cases_fanned(cs)


def test_mutations(emu):
    fl, gz = FC.mutations()
    assert len(fl) == len(gz) == 480
    # Every case is judged; the model accepts at least a quarter and rejects at least a quarter of the raw streams and of all 960.
    # (Not of the gzip half alone: a member's CRC-32 and ISIZE refuse every mutation that changes or drops a decoded byte.)
    for cs in (fl, fl + gz):
        acc = sum(1 for c in cs if FC.verdict(c)[1] == M.OK)
        print("model accepts %d of %d" % (acc, len(cs)))
        assert acc * 4 >= len(cs) and (len(cs) - acc) * 4 >= len(cs), (acc, len(cs))
    judge(fl, _emu_many([c.data for c in fl], "flate"))
    judge(gz, _emu_many([c.data for c in gz], "gzip"))


def test_dst_too_small_writes_nothing(emu):
    cs = [c for c in FC.cases() if c.name in ("fixed/len258-sym285", "stored/65535", "fixed/one-literal")]
    assert len(cs) == 3
    inputs = [c.data for c in cs]
    need = sum(len(FC.verdict(c)[0]) for c in cs)
    dst = np.full(need + 2 * GUARD, 0xA5, dtype=np.uint8)
    r, _, _, _, _ = call(emu, inputs, "flate", b"", True, dst, need - 1)
    assert r == -2 and (dst == 0xA5).all()


def test_large_streams(emu):
    """4 MiB of corpus T at zlib levels 1 and 9, 1 MiB of random bytes (stored blocks), and 1 MiB of the text as a gzip member."""
    import corpora
    text = corpora.corpus("T", 32, 131072).tobytes()
    noise = np.random.default_rng(0xF1A7E).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    assert len(text) == 4 << 20
    cases = FC.sized(text, noise)
    fl = [c for c in cases if c.fmt == "flate"]
    gz = [c for c in cases if c.fmt == "gzip"]
    judge(fl, _emu_many([c.data for c in fl], "flate"))
    judge(gz, _emu_many([c.data for c in gz], "gzip"))
