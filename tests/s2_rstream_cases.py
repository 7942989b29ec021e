"""Shared by tests/test_emu_s2_rstream.py (the S2 stream reader's kernel and state machine on the CPU wave emulator) and
tests/test_gpu_s2_rstream.py (kc_s2_rstream_* on the device): a driver that feeds a stream in pieces with guard bytes around dst, the
reference's verdict restated for a sequential reader, and the inputs both files decode (those of tests/s2_decode_cases.py).

The judge is the reference's own sequential Reader (oracle_goref.s2_read_stream through s2_decode_cases.judge_stream).  Where it
refuses a stream, the reader must report the class of its error behind the bytes of every chunk in front of the error.  Those bytes
are found with the judge alone: of the cuts at the stream's 4-byte chunk headers (s2_decode_cases.headers) and at its end, the largest
one whose front the reference reads without error; what it returns for that front is the expected prefix.  headers() names a
position only when four bytes follow it, so the end of the last chunk it steps over is added to the cuts: with 1 to 3 stray bytes
behind a whole chunk (mutation 424: one byte inserted at the end) the reference's Reader hands that chunk out before its next
4-byte read fails, and without this cut the rule would ask for one chunk less than the reference delivers."""
import ctypes as C

import numpy as np

import s2_decode_cases as K

GUARD = 64
DST = 64 << 10  # (the item-1 streams hold blocks of at most 16 KiB)
OK, CORRUPT, CRC, UNSUPPORTED, UNEXPECTED_EOF, CALLBACK = 0, 1, 2, 3, 6, 7
BAD_ARG, DST_TOO_SMALL = -1, -2
u64, vp = C.c_uint64, C.c_void_p
FEED_ARGS = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32)]
SKIPPABLE_FN = C.CFUNCTYPE(C.c_int, vp, C.c_uint8, C.POINTER(C.c_uint8), u64, u64)
NO_FN = C.cast(None, SKIPPABLE_FN)  # a null function pointer: removes a callback


class Api:
    """new(chunks=, max_block=, ignore_crc=, ignore_id=) -> handle; the other six as kc_s2_rstream_* take them behind the handle."""

    def __init__(self, new, feed, skip, skip_left, on_skippable, reset, free):
        self.new, self.feed, self.skip, self.skip_left, self.on_skippable, self.reset, self.free = new, feed, skip, skip_left, on_skippable, reset, free


def max_buf(max_block):
    """MaxEncodedLen(max_block) + 4 (s2/encode.go:389-418, s2/reader.go:42)."""
    n = int(max_block)
    n += (n.bit_length() + 7) // 7
    n += 0 if max_block == 0 else 1 if max_block < 60 else 2 if max_block < 1 << 8 else 3 if max_block < 1 << 16 else 4 if max_block < 1 << 24 else 5
    return n + 4


def feed(S, h, data, piece=None, eof=True, dst_cap=DST, events=None):
    """Feeds `data` to the open stream h: whole (piece None) or in pieces of `piece` bytes, the last one with the eof flag when eof.
    Every call gets dst_cap bytes of 0xA5 with GUARD bytes of 0xA5 on both sides; nothing outside dst[0, produced) may change.
    Returns (delivered bytes, status, kc_status, bytes consumed); events (a list) gets ("out", bytes) per delivery."""
    data = bytes(data)
    step = piece or max(len(data), 1)
    buf = np.full(dst_cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    consumed, produced, status = u64(), u64(), C.c_uint32()
    out, pend, pos, total = bytearray(), b"", 0, 0
    while True:
        pend += data[pos:pos + step]
        pos = min(pos + step, len(data))
        last = pos >= len(data)
        while True:
            rc = S.feed(h, pend, len(pend), int(eof and last), buf.ctypes.data + GUARD, dst_cap, C.byref(consumed), C.byref(produced), C.byref(status))
            if rc != 0:
                assert consumed.value == 0 and produced.value == 0 and np.all(buf == 0xA5), "a refused call consumed or wrote something"
                return bytes(out), int(status.value), rc, total
            assert consumed.value <= len(pend) and produced.value <= dst_cap
            k = int(produced.value)
            assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + k:] == 0xA5), "written at or behind dst + produced"
            if k:
                out += buf[GUARD:GUARD + k].tobytes()
                if events is not None:
                    events.append(("out", buf[GUARD:GUARD + k].tobytes()))
                buf[GUARD:GUARD + k] = 0xA5
            pend = pend[consumed.value:]
            total += int(consumed.value)
            if status.value:
                return bytes(out), int(status.value), 0, total
            if not (consumed.value or produced.value):
                break
        if last:
            return bytes(out), 0, 0, total


def run(S, data, piece=None, eof=True, dst_cap=DST, skip=(), **opts):
    """One stream from new to free: the skips, then feed()."""
    h = S.new(**opts)
    assert h
    try:
        for n in skip:
            assert S.skip(h, n) == 0
        return feed(S, h, data, piece, eof, dst_cap)
    finally:
        S.free(h)


_expected = {}


def expected(G, stream, **kw):
    """('ok', 0, bytes) or ('err', class, prefix) of a sequential read of `stream`, from the reference's Reader alone.  Computed once
    per input and left unchanged."""
    key = (bytes(stream), tuple(sorted(kw.items())))
    if key not in _expected:
        kind, v = K.judge_stream(G, stream, 1 << 23, **kw)
        if kind == "ok":
            _expected[key] = ("ok", 0, v)
        else:
            got = None
            hs = K.headers(stream)
            after = hs[-1] + 4 + (stream[hs[-1] + 1] | stream[hs[-1] + 2] << 8 | stream[hs[-1] + 3] << 16) if hs else 0
            for h in sorted(set(hs + [0, min(after, len(stream)), len(stream)]), reverse=True):
                k2, v2 = K.judge_stream(G, stream[:h], 1 << 23, **kw)
                if k2 == "ok":
                    got = v2
                    break
            assert got is not None, "the reference refuses the empty front"
            _expected[key] = ("err", v, got)
    return _expected[key]


_mut = {}


def mutation_set(G):
    """The 480 mutations of s2_decode_cases with what a sequential reader owes for each; the census of the set is asserted here, from
    the judge alone, so that a thinner set cannot pass unnoticed."""
    if "m" not in _mut:
        bases = [s for _, s, _ in K.item1_streams(G)[:8]]
        muts = K.mutations(bases)
        exp = [expected(G, m) for m in muts]
        refused = [e for e in exp if e[0] == "err"]
        census = {c: sum(1 for e in refused if e[1] == c) for c in (CORRUPT, CRC, UNSUPPORTED)}
        assert len(muts) == 480 and len(refused) == 476 and census == {CORRUPT: 301, CRC: 162, UNSUPPORTED: 13}, (len(muts), len(refused), census)
        assert sum(1 for e in refused if e[2]) == 317
        _mut["m"] = (muts, exp)
    return _mut["m"]


def check_mutations(G, S, piece, **opts):
    muts, exp = mutation_set(G)
    wrong = []
    for k, (m, (kind, cls, want)) in enumerate(zip(muts, exp)):
        out, status, rc, _ = run(S, m, piece, **opts)
        if (rc, status, out) != (0, cls, want):
            wrong.append("mutation %d [pieces of %s]: rc %d, status %d with %d bytes; the reference: class %d behind %d bytes" % (k, piece, rc, status, len(out), cls, len(want)))
    assert not wrong, "\n".join(wrong[:20])


def skip_base(G):
    """'writer level 0 block 4096': (stream, text, data chunks)."""
    name, s, t = K.item1_streams(G)[0]
    assert name == "writer level 0 block 4096"
    dc = K.data_chunks(s)
    assert len(dc) == 7 and all(ty == 0 for _, ty, _ in dc)
    return s, t, dc


def second_chunk_broken(s, dc):
    """The stream with its second data chunk's stored CRC flipped, and with that chunk's body overwritten by 0xFF.  The body is what a
    pass by the header does not read: everything behind the chunk header, the stored CRC and the block's uvarint."""
    p, _, ln = dc[1]
    a = bytearray(s)
    a[p + 4] ^= 0x40
    b = bytearray(s)
    q = p + 8
    while b[q] & 0x80:
        q += 1
    b[q + 1:p + 4 + ln] = b"\xff" * (p + 4 + ln - q - 1)
    return bytes(a), bytes(b)


def callback_stream(G):
    """identifier, chunk A, 0x80 with 10 bytes, 0x81 with 70 000 bytes, chunk B, padding, 0x99 with 0 bytes; (stream, A, B, payloads)."""
    t = K.tom()
    A, B = t[:3000], t[3000:7000]

    def skippable(id, payload):
        n = len(payload)
        return bytes([id, n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF]) + payload
    pay = {0x80: bytes(range(10)), 0x81: bytes((i * 7 + (i >> 8)) & 0xFF for i in range(70000)), 0x99: b""}
    s = (K.MAGIC + K.chunk_of(G.s2_encode(A), A) + skippable(0x80, pay[0x80]) + skippable(0x81, pay[0x81]) + K.chunk_of(G.s2_encode(B), B) +
         skippable(0xfe, b"\0" * 33) + skippable(0x99, b""))
    return s, A, B, pay


class Recorder:
    """Callbacks that record ("cb", id) once per chunk and collect the pieces; fail_on: the id whose callback returns 1."""

    def __init__(self, events, fail_on=None):
        self.events, self.fail_on = events, fail_on
        self.pieces, self.lefts = {}, {}

        def fn(user, id, piece, n, left):
            if id not in self.pieces or self.lefts[id][-1] == 0:
                self.events.append(("cb", id))
                self.pieces[id] = b""
                self.lefts[id] = []
            self.pieces[id] += bytes(piece[:n]) if n else b""
            self.lefts[id].append(int(left))
            return 1 if id == self.fail_on else 0
        self.fn = SKIPPABLE_FN(fn)


# ---- the tests both files run; S is an Api, G the judge ----
def t_item1(G, S, pieces, chunk_counts):
    for name, s, want in K.item1_streams(G):
        assert expected(G, s) == ("ok", 0, want), name
        for piece in pieces:
            for chunks in chunk_counts:
                kw = {} if chunks is None else {"chunks": chunks}
                assert run(S, s, piece, **kw) == (want, 0, 0, len(s)), (name, piece, chunks)
                h = S.new(**kw)
                try:  # without the eof flag: the same bytes, and the end is only then told
                    assert feed(S, h, s, piece, eof=False) == (want, 0, 0, len(s)), (name, piece, chunks, "no eof")
                    assert feed(S, h, b"", eof=True) == (b"", 0, 0, 0), (name, piece, chunks, "the final feed")
                finally:
                    S.free(h)


def t_end_rules(G, S):
    s, t, dc = skip_base(G)
    stored = K.MAGIC + bytes([1, 104, 0, 0]) + K.crc32c_masked(t[:100]).to_bytes(4, "little") + t[:100]
    assert expected(G, stored) == ("ok", 0, t[:100])
    pad = K.MAGIC + bytes([0xfe, 50, 0, 0]) + b"\0" * 50
    assert expected(G, pad) == ("ok", 0, b"")
    assert run(S, b"") == (b"", 0, 0, 0)
    assert run(S, K.MAGIC) == (b"", 0, 0, 10)
    two = s[:dc[2][0]]  # identifier and two whole chunks
    cases = [("%d stray bytes" % k, two + s[dc[2][0]:dc[2][0] + k], t[:8192], len(two)) for k in (1, 2, 3)]
    cases.append(("inside a header", K.MAGIC[:2], b"", 0))
    cases.append(("inside a compressed chunk", s[:dc[2][0] + 100], t[:8192], len(two)))
    cases.append(("inside a stored chunk", stored[:-1], b"", 10))
    cases.append(("inside padding", pad[:-1], b"", None))
    for name, data, front, boundary in cases:
        assert expected(G, data) == ("err", CORRUPT, front), name
        for piece in (None, 7):
            out, status, rc, consumed = run(S, data, piece)
            assert (out, status, rc) == (front, CORRUPT, 0), (name, piece)
            out, status, rc, consumed = run(S, data, piece, eof=False)  # the same bytes without eof: the call waits
            assert (out, status, rc) == (front, 0, 0), (name, piece, "no eof")
            if boundary is not None:
                assert consumed == boundary, (name, piece, consumed)
            else:
                assert consumed == len(data), (name, "a padding chunk's payload is counted down as it comes")


def t_limits(G, S, big):
    """big: (4 MiB of text, its stream as one 4 MiB block)."""
    t4, s4 = big
    assert run(S, s4, dst_cap=4 << 20) == (t4, 0, 0, len(s4))
    h = S.new()
    try:
        out, status, rc, consumed = feed(S, h, s4, dst_cap=(4 << 20) - 1)
        assert (out, status, rc, consumed) == (b"", 0, DST_TOO_SMALL, 0)
        assert feed(S, h, s4, dst_cap=(4 << 20) + 100) == (t4, 0, 0, len(s4)), "the stream stays usable"
    finally:
        S.free(h)
    s64 = G.s2_stream(t4[:200000], block_size=64 << 10)
    assert expected(G, s64, max_block=32 << 10) == ("err", CORRUPT, b"")
    assert run(S, s64, dst_cap=1 << 20, max_block=32 << 10)[:3] == (b"", CORRUPT, 0)
    assert run(S, s64, dst_cap=1 << 20, max_block=64 << 10) == (t4[:200000], 0, 0, len(s64))
    assert run(S, s64[10:], dst_cap=1 << 20)[:3] == (b"", CORRUPT, 0)
    assert run(S, s64[10:], dst_cap=1 << 20, ignore_id=True) == (t4[:200000], 0, 0, len(s64) - 10)
    bad = bytearray(s64)
    bad[K.data_chunks(s64)[1][0] + 5] ^= 0x10
    assert expected(G, bytes(bad)) == ("err", CRC, t4[:65536])
    assert run(S, bytes(bad), dst_cap=1 << 20)[:3] == (t4[:65536], CRC, 0)
    assert expected(G, bytes(bad), ignore_crc=True) == ("ok", 0, t4[:200000])
    assert run(S, bytes(bad), dst_cap=1 << 20, ignore_crc=True) == (t4[:200000], 0, 0, len(s64))


def t_skip(G, S):
    s, t, dc = skip_base(G)
    for n in (0, 1, 4095, 4096, 4097, 8192, len(t) - 1, len(t)):
        for piece in (None, 7):
            assert run(S, s, piece, skip=(n,)) == (t[n:], 0, 0, len(s)), (n, piece)
    for piece in (None, 7):
        assert run(S, s, piece, skip=(len(t) + 1,))[:3] == (b"", UNEXPECTED_EOF, 0), piece
    assert run(S, s, skip=(1000, 3097)) == (t[4097:], 0, 0, len(s))
    for chunks in (1, 3):
        assert run(S, s, 1000, skip=(4097,), chunks=chunks) == (t[4097:], 0, 0, len(s)), chunks
    crc, body = second_chunk_broken(s, dc)
    assert expected(G, crc) == ("err", CRC, t[:4096]) and expected(G, body) == ("err", CORRUPT, t[:4096])
    for data, cls in ((crc, CRC), (body, CORRUPT)):
        for piece in (None, 7):
            assert run(S, data, piece, skip=(8192,)) == (t[8192:], 0, 0, len(s)), (cls, piece)
            assert run(S, data, piece, skip=(5000,))[:3] == (b"", cls, 0), (cls, piece)
    # a feed that holds a skipped chunk's header and 100 bytes of its body consumes them
    h = S.new()
    try:
        assert S.skip(h, 8192) == 0
        front = dc[1][0] + 4 + 100
        assert feed(S, h, s[:front], eof=False) == (b"", 0, 0, front)
        assert S.skip_left(h) == 0
        assert feed(S, h, s[front:]) == (t[8192:], 0, 0, len(s) - front)
    finally:
        S.free(h)


def t_callbacks(G, S):
    s, A, B, pay = callback_stream(G)
    assert expected(G, s) == ("ok", 0, A + B)
    for piece in (None, 1000):
        events = []
        rec = Recorder(events)
        h = S.new()
        try:
            for id in (0x80, 0x81, 0x99):
                assert S.on_skippable(h, id, rec.fn, None) == 0
            assert S.on_skippable(h, 0x7f, rec.fn, None) == BAD_ARG and S.on_skippable(h, 0xfe, rec.fn, None) == BAD_ARG
            assert feed(S, h, s, piece, events=events) == (A + B, 0, 0, len(s)), piece
        finally:
            S.free(h)
        joined = []  # deliveries next to each other are one event
        for e in events:
            if e[0] == "out" and joined and joined[-1][0] == "out":
                joined[-1] = ("out", joined[-1][1] + e[1])
            else:
                joined.append(e)
        assert joined == [("out", A), ("cb", 0x80), ("cb", 0x81), ("out", B), ("cb", 0x99)], [(k, v if k == "cb" else len(v)) for k, v in joined]
        assert rec.pieces == pay
        assert rec.lefts[0x99] == [0] and rec.lefts[0x80][-1] == 0 and rec.lefts[0x81][-1] == 0
        assert rec.lefts[0x81] == sorted(rec.lefts[0x81], reverse=True)
    # a callback that refuses: A is delivered, B never; a removed callback lets the chunk pass
    events = []
    rec = Recorder(events, fail_on=0x81)
    h = S.new()
    try:
        assert S.on_skippable(h, 0x81, rec.fn, None) == 0
        assert feed(S, h, s, 1000, events=events)[:3] == (A, CALLBACK, 0)
        assert feed(S, h, b"", events=events)[:3] == (b"", CALLBACK, 0), "the stream stays failed"
        assert ("cb", 0x80) not in events, "an id without a callback is passed"
        assert S.reset(h) == 0 and S.on_skippable(h, 0x81, NO_FN, None) == 0
        events.clear()
        assert feed(S, h, s, events=events) == (A + B, 0, 0, len(s)) and all(e[0] == "out" for e in events)
    finally:
        S.free(h)


def t_reset(G, S):
    """Reset after an error reads a second stream; options (here: ignore_crc, one chunk per launch) and callbacks stay."""
    s, t, dc = skip_base(G)
    crc, _ = second_chunk_broken(s, dc)
    cs, A, B, pay = callback_stream(G)
    events = []
    rec = Recorder(events)
    h = S.new(chunks=1, ignore_crc=True)
    try:
        assert S.on_skippable(h, 0x80, rec.fn, None) == 0
        assert feed(S, h, s[:dc[3][0]] + b"\x02\x00\x00\x00")[:3] == (t[:12288], UNSUPPORTED, 0)
        assert S.skip(h, 5) == 0 and S.reset(h) == 0 and S.skip_left(h) == 0
        assert feed(S, h, crc, 1000) == (t, 0, 0, len(s)), "ReaderIgnoreCRC did not survive the reset"
        assert S.reset(h) == 0
        assert feed(S, h, cs, events=events) == (A + B, 0, 0, len(cs))
        assert ("cb", 0x80) in events and rec.pieces[0x80] == pay[0x80]
    finally:
        S.free(h)


def t_refusal_behind_progress(G, S):
    """KC_ERR_DST_TOO_SMALL promises that nothing was consumed.  A call that has already counted a payload down in front of the chunk
    that cannot fit reports that progress with KC_OK; the next call, which starts at the chunk, refuses, and the stream stays usable."""
    t = K.tom()[:1024]
    pad = bytes([0xfe, 50, 0, 0]) + b"\0" * 50
    stored = bytes([1, (len(t) + 4) & 0xFF, (len(t) + 4) >> 8, 0]) + K.crc32c_masked(t).to_bytes(4, "little") + t
    s = K.MAGIC + pad + stored
    assert expected(G, s) == ("ok", 0, t)
    for piece in (None, 30):  # whole; the padding payload split over two feeds
        h = S.new()
        try:
            out, status, rc, consumed = feed(S, h, s, piece, dst_cap=500)  # (feed() itself asserts that the refused call consumed nothing)
            assert (out, status, rc) == (b"", 0, DST_TOO_SMALL) and consumed == 64, (piece, rc, consumed)
            assert feed(S, h, s[64:], dst_cap=2000) == (t, 0, 0, len(s) - 64), "the stream stays usable"
        finally:
            S.free(h)
    # the same with a callback on the chunk in front, and a skipped chunk's body tail: the callback fires once
    s = K.MAGIC + bytes([0x85, 50, 0, 0]) + bytes(range(50)) + stored + stored
    events = []
    rec = Recorder(events)
    h = S.new()
    try:
        assert S.on_skippable(h, 0x85, rec.fn, None) == 0 and S.skip(h, 1024) == 0
        front = 64 + 4 + 100  # the callback chunk whole, then the first stored chunk's header and 100 bytes of the body the skip passes
        assert feed(S, h, s[:front], eof=False, dst_cap=500) == (b"", 0, 0, front)
        out, status, rc, consumed = feed(S, h, s[front:], dst_cap=500)
        assert (out, status, rc, consumed) == (b"", 0, DST_TOO_SMALL, len(stored) - 104), (rc, consumed)
        assert feed(S, h, s[front + consumed:], dst_cap=1024) == (t, 0, 0, len(stored))
        assert events.count(("cb", 0x85)) == 1 and rec.pieces[0x85] == bytes(range(50))
    finally:
        S.free(h)


def t_callback_removed_in_flight(G, S):
    """A callback taken away between two feeds while its chunk is partly handed over: the rest of the chunk is counted down."""
    s, A, B, pay = callback_stream(G)
    events = []
    rec = Recorder(events)
    h = S.new()
    try:
        assert S.on_skippable(h, 0x81, rec.fn, None) == 0
        cut = s.index(pay[0x81][:64]) + 1000
        assert feed(S, h, s[:cut], eof=False, events=events)[:3] == (A, 0, 0)
        assert rec.pieces[0x81] == pay[0x81][:1000]
        assert S.on_skippable(h, 0x81, NO_FN, None) == 0
        assert feed(S, h, s[cut:], events=events)[:3] == (B, 0, 0)
        assert rec.pieces[0x81] == pay[0x81][:1000]
    finally:
        S.free(h)
