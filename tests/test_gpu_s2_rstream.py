"""The S2 stream reader on the device: kc_s2_rstream_* through the C ABI with the cases the CPU wave emulator runs too
(tests/s2_rstream_cases.py, tests/test_emu_s2_rstream.py), judged by the reference's own sequential Reader (translated:
oracle_goref.s2_read_stream), and compress_amd.s2.StreamReader on top of it."""
import ctypes as C
import io

import pytest

import s2_decode_cases as K
import s2_rstream_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own s2.Reader, translated) is the judge of these tests"
    return oracle_goref


@pytest.fixture(scope="module")
def S():
    """kc_s2_rstream_* on one context; chunks=None is the context's default for KC_OPT_S2_RSTREAM_CHUNKS."""
    from compress_amd import _lib
    ctx = _lib.Context(0)
    L = ctx.L
    default = ctx.get_option(_lib.OPT_S2_RSTREAM_CHUNKS)
    assert 1 <= default <= 4096

    def new(chunks=None, max_block=4 << 20, ignore_crc=False, ignore_id=False):
        ctx.set_option(_lib.OPT_S2_RSTREAM_CHUNKS, default if chunks is None else chunks)
        o = C.c_void_p(L.kc_s2_ropts_default())
        assert L.kc_s2_ropts_max_block_size(o, max_block) == 0 and L.kc_s2_ropts_ignore_crc(o, int(ignore_crc)) == 0
        assert L.kc_s2_ropts_ignore_stream_identifier(o, int(ignore_id)) == 0
        h = L.kc_s2_rstream_new(ctx.h, o)
        L.kc_s2_ropts_free(o)  # (the stream holds a copy)
        return h
    yield R.Api(new, L.kc_s2_rstream_feed, L.kc_s2_rstream_skip, L.kc_s2_rstream_skip_left, L.kc_s2_rstream_on_skippable, L.kc_s2_rstream_reset,
                L.kc_s2_rstream_free)
    ctx.close()


@pytest.fixture(scope="module")
def text():
    return K.tom()


# ---- the C ABI: the emulator suite's cases ----
@pytest.mark.parametrize("piece", (None, 4099, 7))
def test_item1_streams(G, S, piece):
    R.t_item1(G, S, (piece,), (None, 1))


def test_mutations_class_and_prefix(G, S):
    R.check_mutations(G, S, None)


def test_end_rules(G, S):
    R.t_end_rules(G, S)


def test_limits(G, S, kclib):
    import corpora
    t4 = corpora.corpus("T", 1, 4 << 20).tobytes()
    R.t_limits(G, S, (t4, G.s2_stream(t4, block_size=4 << 20)))


def test_option_bounds(S):
    from compress_amd import _lib, KcError
    ctx = _lib.Context(0)
    try:
        for bad in (0, 4097, -1):
            with pytest.raises(KcError):
                ctx.set_option(_lib.OPT_S2_RSTREAM_CHUNKS, bad)
        ctx.set_option(_lib.OPT_S2_RSTREAM_CHUNKS, 4096)
        assert ctx.get_option(_lib.OPT_S2_RSTREAM_CHUNKS) == 4096
    finally:
        ctx.close()


def test_refusal_consumes_nothing_behind_progress(G, S):
    R.t_refusal_behind_progress(G, S)


def test_callback_removed_in_flight(G, S):
    R.t_callback_removed_in_flight(G, S)


def test_skip(G, S):
    R.t_skip(G, S)


def test_skip_and_read_equal_the_forward_only_readseeker(G, S):
    """Skip(n) + Read(k) through the stream reader against the existing forward-only s2.NewReadSeeker(..., random=False) on the same input."""
    from compress_amd import s2
    s, t, _ = R.skip_base(G)
    for n, k in ((0, 10), (1, 4096), (4095, 2), (8192, 5000), (len(t) - 3, 3)):
        rs = s2.NewReadSeeker(s, random=False)
        rs.Skip(n)
        want = bytearray(k)
        assert rs.Read(want) == k
        rs.Close()
        sr = s2.NewStreamReader(io.BytesIO(s))
        sr.Skip(n)
        got = bytearray(k)
        assert sr.Read(got) == k and got == want == t[n:n + k], (n, k)
        sr.Close()


def test_callbacks(G, S):
    R.t_callbacks(G, S)


def test_reset_keeps_options_and_callbacks(G, S):
    R.t_reset(G, S)


# ---- s2.StreamReader ----
class Trickle:
    """A reader that serves at most 1000 bytes per call and records what it was asked for; it cannot seek."""

    def __init__(self, data):
        self.data, self.pos, self.asked = bytes(data), 0, []

    def read(self, n=-1):
        self.asked.append(n)
        k = 1000 if n is None or n < 0 else min(n, 1000)
        b = self.data[self.pos:self.pos + k]
        self.pos += len(b)
        return b


def read_all(rd, size):
    out = bytearray()
    p = bytearray(size)
    while True:
        n = rd.Read(p)
        if n == 0:
            return bytes(out)
        out += p[:n]


@pytest.mark.parametrize("size", (1, 10, 4097, 1 << 20))
def test_read_sizes(G, text, size):
    from compress_amd import s2
    s = K.item1_streams(G)[0][1]
    rd = s2.NewStreamReader(io.BytesIO(s))
    if size == 1:
        assert b"".join(bytes([rd.ReadByte()]) for _ in range(100)) == text[:100]
        assert read_all(rd, 1) == text[100:]
    else:
        assert read_all(rd, size) == text
        with pytest.raises(EOFError):
            rd.ReadByte()
    rd.Close()


def test_reader_that_trickles_is_never_asked_for_more_than_batch_bytes(G, text):
    from compress_amd import s2
    s = K.item1_streams(G)[1][1]
    r = Trickle(s)
    rd = s2.NewStreamReader(r, batch_bytes=5000)
    assert read_all(rd, 4097) == text
    assert r.asked and max(r.asked) <= 5000 and min(r.asked) > 0
    with pytest.raises(s2.ErrCantSeek):
        rd.ReadSeeker(True)
    rd.Close()


def test_empty_read_fires_a_pending_callback(G):
    from compress_amd import s2
    s, A, B, pay = R.callback_stream(G)
    seen = []
    rd = s2.NewStreamReader(io.BytesIO(s), skippable={0x80: lambda r: seen.append((0x80, r.read())), 0x81: lambda r: seen.append((0x81, r.read())),
                                                     0x99: lambda r: seen.append((0x99, r.read()))})
    p = bytearray(len(A))
    assert rd.Read(p) == len(A) and bytes(p) == A and seen == []
    assert rd.Read(bytearray(0)) == 0  # the peek: advances to chunk B
    assert seen == [(0x80, pay[0x80]), (0x81, pay[0x81])]
    assert read_all(rd, 1000) == B and seen[-1] == (0x99, b"")
    rd.Close()
    with pytest.raises(ValueError):
        s2.NewStreamReader(io.BytesIO(s), skippable={0x7f: lambda r: None})

    class Mine(Exception):
        pass

    def boom(r):
        raise Mine()
    rd = s2.NewStreamReader(io.BytesIO(s), skippable={0x81: boom})
    assert read_all_until(rd, Mine) == A
    rd.Close()


def read_all_until(rd, exc):
    out = bytearray()
    p = bytearray(1000)
    with pytest.raises(exc):
        while True:
            n = rd.Read(p)
            assert n > 0, "the stream ended without its error"
            out += p[:n]
    return bytes(out)


def test_error_is_raised_behind_its_prefix(G):
    from compress_amd import s2
    muts, exp = R.mutation_set(G)
    picked = [(m, e) for m, e in zip(muts, exp) if e[0] == "err" and e[2]][:6] + [(m, e) for m, e in zip(muts, exp) if e[0] == "err" and not e[2]][:2]
    for m, (_, cls, want) in picked:
        rd = s2.NewStreamReader(io.BytesIO(m), batch_bytes=3000)
        out = bytearray()
        p = bytearray(1000)
        with pytest.raises(s2.S2DecodeError) as ei:
            while True:
                n = rd.Read(p)
                assert n > 0, "the stream ended without its error"
                out += p[:n]
        assert ei.value.status == cls and bytes(out) == want
        with pytest.raises(s2.S2DecodeError):
            rd.Read(p)
        rd.Close()


def test_forward_only_readseeker(G, text):
    from compress_amd import s2
    s = K.item1_streams(G)[0][1]
    rd = s2.NewStreamReader(Trickle(s))
    rs = rd.ReadSeeker(False)
    p = bytearray(100)
    assert rs.Seek(5000) == 5000 and rs.Read(p) == 100 and bytes(p) == text[5000:5100]
    assert rs.Seek(50, s2.SeekCurrent) == 5150
    assert rs.ReadAt(p, 9000) == 100 and bytes(p) == text[9000:9100]
    assert rs.Seek(0, s2.SeekCurrent) == 9100, "ReadAt moves the cursor"
    for refused in (lambda: rs.Seek(9099), lambda: rs.Seek(0, s2.SeekEnd), lambda: rs.ReadAt(p, 0)):
        with pytest.raises(s2.S2DecodeError) as ei:
            refused()
        assert ei.value.name == "KC_S2D_UNSUPPORTED"
    with pytest.raises(s2.S2DecodeError) as ei:
        rs.Seek(len(text) + 1)
    assert ei.value.name == "KC_S2D_UNEXPECTED_EOF"
    rd.Close()
    with pytest.raises(ValueError):
        s2.NewStreamReader(io.BytesIO(s)).Skip(-1)
    # random access: the whole-input seeker over a seekable r
    sx = K.item1_streams(G)[7][1]  # index + padding
    rd = s2.NewStreamReader(io.BytesIO(sx))
    rr = rd.ReadSeeker(True)
    assert rr.ReadAt(p, 20000) == 100 and bytes(p) == text[20000:20100] and rr.ReadAt(p, 10) == 100 and bytes(p) == text[10:110]
    rr.Close()
    rd.Close()


def test_reset_reads_a_second_stream(G, text):
    from compress_amd import s2
    a, b = K.item1_streams(G)[0][1], K.item1_streams(G)[6][1]  # S2 with 4 KiB blocks, then Snappy-framed
    rd = s2.NewStreamReader(io.BytesIO(a[:5000]), s2.ReaderMaxBlockSize(64 << 10))
    with pytest.raises(s2.S2DecodeError):
        read_all(rd, 4096)
    rd.Reset(io.BytesIO(b))
    assert read_all(rd, 4096) == text
    rd.Close()


LEVELS = ("fast", "better", "best", "uncompressed", "snappy")


@pytest.mark.parametrize("level", LEVELS)
def test_the_device_writers_streams_read_back(kclib, level):
    """300 000 bytes of corpus T through the device's own s2.NewWriter at every level, 64 KiB blocks (index and padding on one of
    them), read back through the stream reader in a window of two chunks per launch."""
    import corpora
    from compress_amd import _lib, s2
    t = corpora.corpus("T", 1, 300000).tobytes()
    opts = {"fast": [], "better": [s2.WriterBetterCompression()], "best": [s2.WriterBestCompression()], "uncompressed": [s2.WriterUncompressed()],
            "snappy": [s2.WriterSnappyCompat()]}[level]
    if level == "better":
        opts += [s2.WriterAddIndex(), s2.WriterPadding(4096)]
    w = io.BytesIO()
    sw = s2.NewWriter(w, s2.WriterBlockSize(64 << 10), *opts, device=0)
    sw.Write(t)
    sw.Close()
    rd = s2.NewStreamReader(io.BytesIO(w.getvalue()), batch_bytes=100000)
    rd.ctx().set_option(_lib.OPT_S2_RSTREAM_CHUNKS, 2)
    rd.Reset(io.BytesIO(w.getvalue()))  # (a stream takes the option when it is made)
    assert read_all(rd, 70001) == t
    rd.Close()
