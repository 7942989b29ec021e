"""The zstd stream reader on the device: kc_zstd_dstream_new / _feed / _free (kc_zstd_dstream.hip, kc_zstd_dstream_api.cpp) and
zstd.NewReader(r) / Read / WriteTo (compress_amd.zstd.Decoder), judged by the reference's own DecodeAll (translated:
oracle_goref.zstd_decode_all) with the stream form's substitutions (tests/zstd_dstream_cases.py)."""
import io
import random
import threading

import pytest

import zstd_dstream_cases as K
import zstd_frame_cases as zc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own DecodeAll, translated) is the judge of these tests"
    return oracle_goref


@pytest.fixture(scope="module")
def text():
    return K.twain()[:300000]


class _Dev:
    """A decoder's options and context behind the three stream functions; blocks = KC_OPT_DSTREAM_BLOCKS."""

    def __init__(self, blocks=512, *opts):
        from compress_amd import zstd, _lib
        self.d = zstd.NewReader(None, *opts)
        ctx = self.d.ctx()
        ctx.set_option(_lib.OPT_DSTREAM_BLOCKS, blocks)
        assert ctx.get_option(_lib.OPT_DSTREAM_BLOCKS) == blocks
        L = ctx.L
        self.S = K.Stream(lambda: L.kc_zstd_dstream_new(ctx.h, self.d._o), L.kc_zstd_dstream_feed, L.kc_zstd_dstream_free)

    def close(self):
        self.d.Close()


@pytest.fixture(scope="module")
def devs(kclib):
    made = {}

    def get(blocks=512, key=None, *opts):
        k = (blocks, key)
        if k not in made:
            made[k] = _Dev(blocks, *opts)
        return made[k].S
    yield get
    for v in made.values():
        v.close()


def _raw_dict_opts():
    from compress_amd import zstd
    return [zstd.WithDecoderDictRaw(i, c) for i, c in zc.DICTS.items()]


# ---- 1. the hand-built frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", (512, 1))
def test_frame_cases_as_streams(kclib, G, devs, blocks):
    S = devs(blocks, "raw", *_raw_dict_opts())
    wrong = []
    for c in zc.cases():
        want, err = zc.reference(G, c)
        for piece in (None, 7, 1000):
            if piece == 7 and len(c.data) > 40000:
                piece = 4099  # (the long frames: an odd piece that still cuts every block)
            out, status, rc = K.run(S, c.data, piece)
            w = K.judge_one("%s [pieces of %s]" % (c.name, piece), c.data, want, err, out, status, rc, plain=c.plain)
            if w:
                wrong.append(w)
    assert not wrong, "\n".join(wrong)


# ---- 2. the reference encoder's streams ------------------------------------------------------------------------------------------
def test_encoder_streams(kclib, G, devs, text):
    for level in (1, 2, 3):
        for crc in (False, True):
            z = G.zstd_encode_stream(text, level=level, crc=crc)
            for blocks, piece in ((512, None), (1, None), (512, 50000), (1, 4099)):
                assert K.run(devs(blocks), z, piece) == (text, 0, 0), (level, crc, blocks, piece)


@pytest.mark.parametrize("window", (8 << 10, 16 << 10))
def test_small_windows_slide_on_every_launch(kclib, G, devs, text, window):
    for level in (1, 2, 3):
        z = G.zstd_encode_stream(text, level=level, window_size=window, crc=True)
        assert K.run(devs(1), z) == (text, 0, 0), level
        assert K.run(devs(3), z, 1000) == (text, 0, 0), level


def test_composite_stream_and_cut_points(kclib, G, devs):
    data, plain, cuts = K.composite(G)
    assert K.ref(G, data)[0] == plain
    for blocks in (512, 1):
        S = devs(blocks)
        assert K.run(S, data) == (plain, 0, 0)
        assert K.run(S, data, cuts=cuts) == (plain, 0, 0)
        for c in cuts:
            assert K.run(S, data, cuts=[c]) == (plain, 0, 0), c
    assert K.run(devs(), b"") == (b"", 0, 0)


# ---- 3. dictionaries -------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_one_block_per_launch(kclib, G, devs):
    from compress_amd import zstd
    dicts, frames = K.dict_frames()
    S = devs(1, "dicts", zstd.WithDecoderDicts(*dicts.values()), *_raw_dict_opts())
    for m, z in frames:
        want, err = K.ref(G, z, dict_blob=dicts[K.frame_dict_id(z)])
        assert want is not None, (m, err)
        assert K.run(S, z) == (want, 0, 0), m
        assert K.run(S, z, 777) == (want, 0, 0), m
    out, status, rc = K.run(devs(1), frames[0][1])
    assert (out, K.NAMES[status], rc) == (b"", "UNKNOWN_DICT", 0)
    for c in zc.cases():
        if c.dicts and c.expect == "valid":
            assert K.run(S, c.data) == (c.plain, 0, 0), c.name


# ---- 4. error delivery -----------------------------------------------------------------------------------------------------------
def test_bad_members_behind_a_good_frame(kclib, G, devs, text):
    good = G.zstd_encode_stream(text[:150000], level=1, crc=True)
    S = devs(512)
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


def test_checksum_mismatch_comes_last(kclib, G, devs, text):
    from compress_amd import zstd
    z = bytearray(G.zstd_encode_stream(text, level=1, crc=True))
    z[-1] ^= 0x40
    for blocks in (512, 1):
        out, status, rc = K.run(devs(blocks), bytes(z), 30000)
        assert (out, K.NAMES[status], rc) == (text, "CRC", 0)
        assert K.run(devs(blocks, "nocrc", zstd.IgnoreChecksum(True)), bytes(z)) == (text, 0, 0)


def test_truncations_give_eof_behind_a_prefix(kclib, G, devs, text):
    z = G.zstd_encode_stream(text, level=1, crc=True)
    rng = random.Random(0x5EED0040)
    for cut in sorted(rng.randrange(1, len(z)) for _ in range(40)):
        for blocks in (512, 1):
            out, status, rc = K.run(devs(blocks), z[:cut], 65536)
            assert rc == 0 and K.NAMES[status] == "EOF" and text[:len(out)] == out, (cut, blocks, K.NAMES[status], len(out))


# ---- 5. seeded mutations ---------------------------------------------------------------------------------------------------------
def test_differential_on_mutations(kclib, G, devs):
    """All 480 cases: accepted or refused as the reference's DecodeAll, its bytes where it accepts, its class where it refuses, with
    KC_ZD_EOF and KC_ZD_CORRUPT counting as one class (tests/test_emu_zstd_dstream.py says why)."""
    cases = K.mutation_cases(G)
    wrong = []
    accepted = 0
    for i, z in enumerate(cases):
        want, err = K.ref(G, z)
        accepted += want is not None
        out, status, rc = K.run(devs(512 if i % 8 else 1), z)
        w = K.judge_one("mutation %d" % i, z, want, err, out, status, rc, loose_eof=True)
        if w:
            wrong.append(w)
    assert not wrong, "\n".join(wrong)
    assert accepted * 5 >= len(cases) and (len(cases) - accepted) * 5 >= len(cases)


# ---- 6. the reader --------------------------------------------------------------------------------------------------------------
class _Short(io.RawIOBase):
    def __init__(self, data):
        self.data, self.pos, self.rng = data, 0, random.Random(7)

    def read(self, n=-1):
        k = min(self.rng.randrange(1, 5000), n if n and n > 0 else 5000)
        b = self.data[self.pos:self.pos + k]
        self.pos += len(b)
        return b


def test_new_reader(kclib, G, text):
    from compress_amd import zstd
    z = G.zstd_encode_stream(text, level=2, crc=True)
    for size in (1, 100, 1 << 20):
        d = zstd.NewReader(io.BytesIO(z), batch_bytes=1 << 16)
        got, p = bytearray(), bytearray(size)
        limit = 3000 if size == 1 else len(text) + 1
        while len(got) < limit:
            n = d.Read(p)
            if n == 0:
                break
            got += p[:n]
        assert bytes(got) == text[:len(got)] and len(got) >= min(limit, len(text)), size
        d.Close()
    d = zstd.NewReader(_Short(z))
    w = io.BytesIO()
    assert d.WriteTo(w) == len(text) and w.getvalue() == text
    assert d.Read(bytearray(10)) == 0
    d.Reset(io.BytesIO(z[:len(z) // 2]))  # a stream that fails, then Reset onto a second one
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
    assert d.DecodeAll(z) == text  # the stateless form beside a stream
    d.Reset(io.BytesIO(b""))
    assert d.Read(bytearray(5)) == 0
    d.Close()
    with pytest.raises(zstd.ErrDecoderClosed):
        d.Read(bytearray(5))


def test_nil_input_is_still_not_implemented(kclib):
    from compress_amd import zstd
    d = zstd.NewReader(None)
    with pytest.raises(NotImplementedError):
        d.Read(bytearray(4))
    with pytest.raises(zstd.ErrDecoderNilInput):
        d.WriteTo(io.BytesIO())
    d.Reset(None)
    with pytest.raises(zstd.ErrDecoderNilInput):
        d.Read(bytearray(4))
    d.Close()


def test_device_encoder_stream_read_back(kclib):
    """3 MiB through the device's own Encoder.Write / Close, read back with every block in one launch and with five blocks per launch,
    where the launch boundaries fall off the blocks that define the tables."""
    import corpora
    from compress_amd import zstd, _lib
    src = corpora.corpus("T", 24, 128 << 10).tobytes()
    w = io.BytesIO()
    enc = zstd.NewWriter(w, zstd.WithEncoderLevel(zstd.SpeedFastest), zstd.WithEncoderCRC(True))
    for at in range(0, len(src), 700000):
        enc.Write(src[at:at + 700000])
    enc.Close()
    z = w.getvalue()
    for blocks in (512, 5):
        d = zstd.NewReader(None)
        d.ctx().set_option(_lib.OPT_DSTREAM_BLOCKS, blocks)
        d.Reset(io.BytesIO(z))
        out = io.BytesIO()
        assert d.WriteTo(out) == len(src) and out.getvalue() == src, blocks
        d.Close()


def test_two_decoders_on_two_threads(kclib, G, text):
    from compress_amd import zstd
    zs = [G.zstd_encode_stream(text[k * 1000:], level=1 + k, crc=True) for k in range(2)]
    res = [None, None]

    def work(k):
        try:
            for _ in range(3):
                d = zstd.NewReader(io.BytesIO(zs[k]), batch_bytes=1 << 17)
                w = io.BytesIO()
                d.WriteTo(w)
                d.Close()
                assert w.getvalue() == text[k * 1000:]
            res[k] = True
        except BaseException as e:  # noqa: BLE001
            res[k] = e
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res == [True, True], res


def test_dst_of_exactly_one_blocks_bound(kclib, G, devs, text):
    """dst_cap == min(window, 128 KiB): one block per call fits, the guard bytes stay (K.run checks them after every call); one byte
    less is KC_ERR_DST_TOO_SMALL."""
    z = G.zstd_encode_stream(text, level=1, crc=True)  # window 4 MiB: the bound is 128 KiB
    assert K.run(devs(512), z, dst_cap=128 << 10) == (text, 0, 0)
    out, status, rc = K.run(devs(512), z, dst_cap=(128 << 10) - 1)
    assert rc == -2 and out == b""
    z8 = G.zstd_encode_stream(text, level=1, window_size=8 << 10, crc=True)
    assert K.run(devs(512), z8, dst_cap=8 << 10) == (text, 0, 0)
