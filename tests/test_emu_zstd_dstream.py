"""The zstd stream reader (kc_zstd_dstream.hip, kc_zdstream_host.h) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_zstd_dstream_new / _feed / _free — the product's state machine over plain memory), judged by the reference's own DecodeAll
(translated: oracle_goref.zstd_decode_all) with the stream form's substitutions (tests/zstd_dstream_cases.py)."""
import ctypes as C
import io
import random

import numpy as np
import pytest

import zstd_dstream_cases as K
import zstd_frame_cases as zc


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference decoder) is not built")
    return oracle_goref


def emu_stream(blocks=512, dicts=(), max_memory=64 << 30, max_window=1 << 29, ignore_checksum=False):
    import emu_lib
    L = emu_lib.lib()
    L.kcemu_zstd_dstream_new.restype = C.c_void_p
    L.kcemu_zstd_dstream_new.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.kcemu_zstd_dstream_feed.restype = C.c_int
    L.kcemu_zstd_dstream_feed.argtypes = K.FEED_ARGS
    L.kcemu_zstd_dstream_free.restype = None
    L.kcemu_zstd_dstream_free.argtypes = [C.c_void_p]
    doff = np.zeros(len(dicts) + 1, dtype=np.uint64)
    doff[1:] = np.cumsum([len(d) for d in dicts])
    dblob = np.frombuffer(b"".join(dicts) + b"\0", dtype=np.uint8).copy()

    def new():
        h = L.kcemu_zstd_dstream_new(max_memory, max_window, int(ignore_checksum), blocks, dblob.ctypes.data, doff.ctypes.data, len(dicts))
        assert h, "a dictionary was refused"
        return h
    return K.Stream(new, L.kcemu_zstd_dstream_feed, L.kcemu_zstd_dstream_free)


RAW_DICTS = [zc.raw_dict_blob(i, d) for i, d in zc.DICTS.items()]


# ---- 1. the hand-built frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", (512, 1))
def test_frame_cases_as_streams(G, blocks):
    """Every case of zstd_frame_cases.cases() fed whole, in pieces of 7 and of 1000 bytes: the reference's bytes with status 0, or a
    status of the reference's class behind a prefix of the plaintext."""
    S = emu_stream(blocks, RAW_DICTS)
    cs = [c for c in zc.cases() if zc.full() or not c.big]
    wrong = []
    for c in cs:
        want, err = zc.reference(G, c)
        for piece in (None, 7, 1000):
            if piece == 7 and len(c.data) > 40000 and not zc.full():
                piece = 4099  # (the long frames: an odd piece that still cuts every block)
            out, status, rc = K.run(S, c.data, piece)
            w = K.judge_one("%s [pieces of %s]" % (c.name, piece), c.data, want, err, out, status, rc, plain=c.plain)
            if w:
                wrong.append(w)
    assert not wrong, "\n".join(wrong)


# ---- 2. the reference encoder's streams ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text():
    return K.twain()[:300000]


@pytest.mark.parametrize("level", (1, 2, 3))
def test_encoder_streams(G, text, level):
    """300 000 bytes of Tom Sawyer through the reference's stream writer: three blocks, with and without a checksum; every block in
    one launch, and each in its own."""
    for crc in (False, True):
        z = G.zstd_encode_stream(text, level=level, crc=crc)
        assert K.ref(G, z)[0] == text
        for blocks, piece in ((512, None), (1, None), (512, 50000), (1, 4099)):
            assert K.run(emu_stream(blocks), z, piece) == (text, 0, 0), (level, crc, blocks, piece)


@pytest.mark.parametrize("window", (8 << 10, 16 << 10))
def test_small_windows_slide_on_every_launch(G, text, window):
    for level in (1, 2, 3):
        z = G.zstd_encode_stream(text, level=level, window_size=window, crc=True)
        assert K.ref(G, z)[0] == text
        assert K.run(emu_stream(1), z) == (text, 0, 0), level
        assert K.run(emu_stream(3), z, 1000) == (text, 0, 0), level


def test_composite_stream_and_cut_points(G):
    data, plain, cuts = K.composite(G)
    assert K.ref(G, data)[0] == plain
    for blocks in (512, 1):
        S = emu_stream(blocks)
        assert K.run(S, data) == (plain, 0, 0)
        assert K.run(S, data, cuts=cuts) == (plain, 0, 0)
        for c in cuts:
            assert K.run(S, data, cuts=[c]) == (plain, 0, 0), c
    assert K.run(emu_stream(), b"") == (b"", 0, 0)  # an empty stream is a clean end


# ---- 3. dictionaries -------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_one_block_per_launch(G):
    """dict-tests-small.zip: the full-format dictionary's tables and repeat offsets are the first carried state."""
    dicts, frames = K.dict_frames()
    S = emu_stream(1, list(dicts.values()) + RAW_DICTS)
    for m, z in frames:
        want, err = K.ref(G, z, dict_blob=dicts[K.frame_dict_id(z)])
        assert want is not None, (m, err)
        assert K.run(S, z) == (want, 0, 0), m
        assert K.run(S, z, 777) == (want, 0, 0), m
    out, status, rc = K.run(emu_stream(1), frames[0][1])
    assert (out, K.NAMES[status], rc) == (b"", "UNKNOWN_DICT", 0)
    for c in zc.cases():  # raw dictionaries
        if c.dicts and c.expect == "valid":
            assert K.run(S, c.data) == (c.plain, 0, 0), c.name


# ---- 4. error delivery -----------------------------------------------------------------------------------------------------------
def test_bad_members_behind_a_good_frame(G, text):
    good = G.zstd_encode_stream(text[:150000], level=1, crc=True)
    S = emu_stream(512)
    wrong = []
    for m, z in K.members("bad.zip"):
        want, err = K.ref(G, z)
        assert want is None, m
        out, status, rc = K.run(S, good + z)
        if rc != 0 or status == 0 or out[:150000] != text[:150000]:
            wrong.append("%s: kc_status %d, status %s, %d bytes" % (m, rc, K.NAMES.get(status, status), len(out)))
            continue
        w = K.judge_one(m, z, None, err, b"", status, rc)
        if w:
            wrong.append(w)
    assert not wrong, "\n".join(wrong)


def test_checksum_mismatch_comes_last(G, text):
    z = bytearray(G.zstd_encode_stream(text, level=1, crc=True))
    z[-1] ^= 0x40
    for blocks in (512, 1):
        out, status, rc = K.run(emu_stream(blocks), bytes(z), 30000)
        assert (out, K.NAMES[status], rc) == (text, "CRC", 0)
        assert K.run(emu_stream(blocks, ignore_checksum=True), bytes(z)) == (text, 0, 0)


def test_truncations_give_eof_behind_a_prefix(G, text):
    z = G.zstd_encode_stream(text, level=1, crc=True)
    rng = random.Random(0x5EED0040)
    for cut in sorted(rng.randrange(1, len(z)) for _ in range(40)):
        for blocks in (512, 1):
            out, status, rc = K.run(emu_stream(blocks), z[:cut], 65536)
            assert rc == 0 and K.NAMES[status] == "EOF" and text[:len(out)] == out, (cut, blocks, K.NAMES[status], len(out))


# ---- 5. seeded mutations ---------------------------------------------------------------------------------------------------------
def test_differential_on_mutations(G):
    """Accepted or refused as the reference's DecodeAll, its bytes where it accepts, its class where it refuses — KC_ZD_EOF and
    KC_ZD_CORRUPT counting as one class: the reference's DecodeAll decodes and executes a block's sequences in one loop, its stream
    form and this one finish the block's entropy stage first, so a block with a bad offset early and a dry bit reader late is named
    differently by the two.  120 of the 480 cases by default (every fourth), all with KC_TEST_FULL=1."""
    cases = K.mutation_cases(G)
    pick = range(len(cases)) if zc.full() else range(0, len(cases), 4)
    wrong = []
    accepted = 0
    for i in pick:
        z = cases[i]
        want, err = K.ref(G, z)
        accepted += want is not None
        out, status, rc = K.run(emu_stream(512 if i % 8 else 1), z)
        w = K.judge_one("mutation %d" % i, z, want, err, out, status, rc, loose_eof=True)
        if w:
            wrong.append(w)
    assert not wrong, "\n".join(wrong)
    assert 0 < accepted < len(pick)


# ---- 6. the reader class ---------------------------------------------------------------------------------------------------------
class _Short(io.RawIOBase):
    """A reader that returns short reads."""

    def __init__(self, data):
        self.data, self.pos, self.rng = data, 0, random.Random(7)

    def read(self, n=-1):
        k = min(self.rng.randrange(1, 5000), n if n and n > 0 else 5000)
        b = self.data[self.pos:self.pos + k]
        self.pos += len(b)
        return b


def _decoder_on_emulator(r, blocks=512, batch_bytes=1 << 16):
    """zstd.Decoder with its stream on the emulator's functions (no device, no library)."""
    from compress_amd import zstd
    S = emu_stream(blocks)
    d = zstd.Decoder.__new__(zstd.Decoder)
    d._o, d._ctx, d._sb, d._closed, d._batch_bytes = None, None, None, False, batch_bytes
    d._open = lambda rr: zstd.StreamBuffer(S.new, S.feed, S.free, rr, batch_bytes)
    d.Reset(r)
    return d


def test_reader_class_on_the_emulator(G, text):
    from compress_amd import zstd
    z = G.zstd_encode_stream(text, level=2, crc=True)
    for size in (1, 100, 1 << 20):
        d = _decoder_on_emulator(io.BytesIO(z))
        got, p = bytearray(), bytearray(size)
        limit = 3000 if size == 1 else len(text) + 1
        while len(got) < limit:
            n = d.Read(p)
            if n == 0:
                break
            got += p[:n]
        assert bytes(got) == text[:len(got)] and len(got) >= min(limit, len(text)), size
        d.Close()
    d = _decoder_on_emulator(_Short(z))
    w = io.BytesIO()
    assert d.WriteTo(w) == len(text) and w.getvalue() == text
    assert d.Read(bytearray(10)) == 0  # the clean end
    # a failed stream, then Reset onto a second one
    d.Reset(io.BytesIO(z[:len(z) // 2]))
    p = bytearray(1 << 20)
    n = d.Read(p)
    assert 0 < n < len(text) and bytes(p[:n]) == text[:n]
    with pytest.raises(zstd.DecodeError) as ei:
        while True:
            n2 = d.Read(p)
            assert bytes(p[:n2]) == text[n:n + n2]
            n += n2
    assert ei.value.name == "KC_ZD_EOF"
    d.Reset(io.BytesIO(z))
    assert d.IOReadCloser().read() == text
    d.Reset(io.BytesIO(b""))
    assert d.Read(bytearray(5)) == 0  # an empty reader
    d.Reset(None)
    with pytest.raises(zstd.ErrDecoderNilInput):
        d.Read(bytearray(5))
    with pytest.raises(NotImplementedError):
        d.WriteTo(io.BytesIO())
    d.Reset(io.BytesIO(z))
    d.Close()
    with pytest.raises(zstd.ErrDecoderClosed):
        d.Read(bytearray(5))
    with pytest.raises(zstd.ErrDecoderClosed):
        d.Reset(io.BytesIO(z))
