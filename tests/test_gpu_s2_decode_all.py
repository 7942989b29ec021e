"""s2.Reader / s2.Decode on the device as a product (kc_s2_decode_streams[_dev], kc_s2_decode_blocks_all[_dev], compress_amd.s2.Reader):
batches of independent inputs, no decoded size supplied, CRCs checked, judged by the reference's own Reader and Decode (translated:
oracle_goref.s2_read_stream / s2_decode).  The cases are those of tests/s2_decode_cases.py, the ones the CPU wave emulator runs too
(tests/test_emu_s2_decode_all.py), plus what needs the device: streams of the device encoder at every level, the host-buffer entry
points and their batches."""
import io

import numpy as np
import pytest

import corpora
import s2_decode_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own s2.Reader, translated) is the judge of these tests"
    return oracle_goref


_verdicts = {}


def judged(G, stream, **kw):
    """The judge's verdict, computed once per (input, options) and left unchanged."""
    key = (stream, tuple(sorted(kw.items())))
    if key not in _verdicts:
        _verdicts[key] = K.judge_stream(G, stream, 1 << 20, **kw)
    return _verdicts[key]


def run(inputs, blocks=False, max_block=4 << 20, ignore_crc=False, ignore_id=False, cap=None):
    """One device-resident batch through compress_amd.s2.Reader: dst sized by the plan unless `cap` is given, 64 guard bytes of 0xA5 on
    both sides of it."""
    import torch
    from compress_amd import s2, KcError
    opts = [s2.ReaderMaxBlockSize(max_block)]
    if ignore_crc:
        opts.append(s2.ReaderIgnoreCRC())
    if ignore_id:
        opts.append(s2.ReaderIgnoreStreamIdentifier())
    rd = s2.NewReader(None, *opts)
    try:
        n = len(inputs)
        src, off = K.pack(inputs)
        d_src = torch.from_numpy(src).cuda(0)
        bound, _ = rd.DecodeBoundsDevice(d_src.data_ptr(), off, blocks=blocks)
        if cap is None:
            cap = int(bound.sum())
        d_all = torch.full((cap + 2 * K.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc = 0
        out_off, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        try:
            fn = rd.DecodeBlocksDevice if blocks else rd.DecodeStreamsDevice
            out_off, status = fn(d_src.data_ptr(), off, d_all.data_ptr() + K.GUARD, cap)
        except KcError as e:
            rc = e.status
        host = d_all.cpu().numpy()
    finally:
        rd.Close()
    assert np.all(host[:K.GUARD] == 0xA5) and np.all(host[K.GUARD + cap:] == 0xA5), "written outside dst"
    if rc != 0:
        assert np.all(host == 0xA5), "dst touched by a call that failed"
    return K.Result(rc, host[K.GUARD:K.GUARD + cap], out_off, status, bound)


def test_one_batch_of_everything(kclib, G):
    items = K.item1_streams(G)
    verdicts = [judged(G, s) for _, s, _ in items]
    for (name, _, want), (kind, got) in zip(items, verdicts):
        assert kind == "ok" and got == want, name
    res = run([s for _, s, _ in items])
    ok, _ = K.check(res, verdicts)
    assert ok == len(items)
    assert [int(b) for b in res.bound] == [len(w) for _, _, w in items]


def test_sizes_at_the_limits(kclib, G):
    t = corpora.corpus("T", 1, 4 << 20).tobytes()
    big = [G.s2_stream(t, block_size=4 << 20), G.s2_stream(t[:3 << 20], block_size=1 << 20)]
    verdicts = [K.judge_stream(G, s, 4 << 20) for s in big]
    assert [k for k, _ in verdicts] == ["ok", "ok"] and verdicts[0][1] == t and verdicts[1][1] == t[:3 << 20]
    assert K.check(run(big), verdicts)[0] == 2
    s64 = G.s2_stream(t[:200000], block_size=64 << 10)
    v = K.judge_stream(G, s64, 1 << 20, max_block=32 << 10)
    assert v == ("err", K.CORRUPT)
    K.check(run([s64], max_block=32 << 10), [v])
    v = K.judge_stream(G, s64, 1 << 20, max_block=64 << 10)
    assert v == ("ok", t[:200000])
    K.check(run([s64], max_block=64 << 10), [v])
    K.check(run([s64[10:]], ignore_id=True), [("ok", t[:200000])])
    v = K.judge_stream(G, s64[10:], 1 << 20)
    assert v == ("err", K.CORRUPT)
    K.check(run([s64[10:]]), [v])


def test_hand_built_blocks(kclib, G):
    hand = K.hand_blocks(G)
    named = hand + K.regression_blocks()
    named.append(("rawsnappy", open(K.S2IN + "/Mark.Twain-Tom.Sawyer.txt.rawsnappy", "rb").read()))
    blocks = [b for _, b in named]
    verdicts = [K.judge_block(G, b, 1 << 20) for b in blocks]
    assert all(k == "ok" for k, _ in verdicts[:len(hand)]), [nm for (nm, _), (k, _) in zip(named, verdicts) if k != "ok"]
    assert verdicts[-1] == ("ok", K.tom()[:len(K.tom()) // 2])
    res = run(blocks, blocks=True)
    ok, _ = K.check(res, verdicts, "bare blocks")
    assert ok >= len(hand) + 1
    streams, sv = [], []
    for b, (k, v) in zip(blocks, verdicts):  # the same as chunks, one stream each
        streams.append(K.MAGIC + K.chunk_of(b, v if k == "ok" else b""))
        sv.append(K.judge_stream(G, streams[-1], 1 << 20))
        assert (sv[-1] == ("ok", v)) if k == "ok" else (sv[-1][0] == "err")
    K.check(run(streams), sv, "chunks")


def test_literal_of_16_mib_in_a_bare_block(kclib, G):
    """The 5-byte literal tag: one literal of 16 777 217 bytes."""
    lit = np.random.default_rng(5).integers(0, 256, 16777217, dtype=np.uint8).tobytes()
    blk = K.uvarint(len(lit)) + G.s2_emit("literal", 0, 0, lit)
    assert blk[len(K.uvarint(len(lit)))] == 63 << 2
    v = K.judge_block(G, blk, len(lit))
    assert v == ("ok", lit)
    K.check(run([blk], blocks=True), [v])


@pytest.mark.parametrize("ignore_crc", [False, True])
def test_mutations(kclib, G, ignore_crc):
    """480 mutations, seed 0x52D0001, of the first eight streams of the batch of everything (s2_decode_cases.mutations).  The reference
    alone gives for this recipe: with CRC checking 301 corrupt, 162 CRC, 13 unsupported, 4 decode; with ignore_crc 128 decode (108 of
    them to bytes other than the source), 313 corrupt, 39 unsupported."""
    bases = [s for _, s, _ in K.item1_streams(G)[:8]]
    muts = K.mutations(bases)
    verdicts = [judged(G, m, ignore_crc=ignore_crc) for m in muts]
    res = run(muts, ignore_crc=ignore_crc)
    ok, classes = K.check(res, verdicts)
    if ignore_crc:
        assert ok >= 96, ok
    else:
        assert all(classes.get(c, 0) >= 10 for c in (K.CORRUPT, K.CRC, K.UNSUPPORTED)), classes


def test_first_error_wins_in_stream_order(kclib, G):
    cases = K.first_error_cases(G)
    verdicts = [judged(G, s) for _, s, _ in cases]
    assert verdicts == [("err", want) for _, _, want in cases]
    K.check(run([s for _, s, _ in cases]), verdicts)


def test_refusals_between_good_neighbours(kclib, G):
    items = K.item1_streams(G)
    bases = [s for _, s, _ in items[:8]]
    bad = [m for m in K.mutations(bases) if judged(G, m, ignore_crc=False)[0] == "err"][:16]
    assert len(bad) == 16
    inputs = []
    for i, (_, s, _) in enumerate(items):
        inputs.append(s)
        inputs.append(bad[i])
    inputs += bad[len(items):]
    verdicts = [judged(G, s, ignore_crc=False) for s in inputs]
    res = run(inputs)
    ok, classes = K.check(res, verdicts)
    assert ok == len(items) and sum(classes.values()) == 16
    short = run(inputs, cap=int(res.out_off[-1]) - 1)  # (run() checks that dst is untouched)
    assert short.rc == K.DST_TOO_SMALL


# ---- what needs the device ----
LEVELS = ("LevelDefault", "LevelBetter", "LevelBest", "LevelSnappy", "LevelUncompressed")


def _encode_stream(level, d_src, blk_off):
    """EncodeStreamDevice of the blocks at `level`: the stream as a device tensor."""
    import torch
    from compress_amd import s2
    enc = s2.BlockEncoder(level=getattr(s2, level))
    try:
        n = len(blk_off) - 1
        cap = sum(((s2.MaxEncodedLen(int(blk_off[i + 1] - blk_off[i])) + 8 + 15) & ~15) for i in range(n)) + 64
        d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        oo = enc.EncodeStreamDevice(d_src.data_ptr(), blk_off, d_dst.data_ptr(), cap)
        return d_dst[:int(oo[-1])].clone()
    finally:
        enc.Close()


def test_streams_of_the_device_encoder_at_every_level(kclib):
    """EncodeStreamDevice at every level over 2 048 x 64 KiB J blocks -> DecodeStreamsDevice -> the source."""
    import torch
    from compress_amd import s2
    nblk, bs = 2048, 64 << 10
    src = corpora.corpus("J", nblk, bs)
    d_src = torch.from_numpy(src).cuda(0)
    blk_off = np.arange(nblk + 1, dtype=np.uint64) * bs
    rd = s2.NewReader(None)
    try:
        for level in LEVELS:
            d_enc = _encode_stream(level, d_src, blk_off)
            off = np.array([0, d_enc.numel()], dtype=np.uint64)
            bound, st = rd.DecodeBoundsDevice(d_enc.data_ptr(), off)
            assert (int(bound[0]), int(st[0])) == (nblk * bs, 0), level
            d_all = torch.full((nblk * bs + 2 * K.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
            out_off, status = rd.DecodeStreamsDevice(d_enc.data_ptr(), off, d_all.data_ptr() + K.GUARD, nblk * bs)
            assert int(status[0]) == 0 and [int(x) for x in out_off] == [0, nblk * bs], level
            assert torch.equal(d_all[K.GUARD:K.GUARD + nblk * bs], d_src), level
            assert bool((d_all[:K.GUARD] == 0xA5).all()) and bool((d_all[K.GUARD + nblk * bs:] == 0xA5).all()), level
    finally:
        rd.Close()


@pytest.fixture(scope="module")
def twelve_streams(kclib):
    """12 streams of 256 x 64 KiB J blocks (192 MiB decoded), the levels in turn: (host bytes of each stream, the source)."""
    import torch
    nblk, bs = 256, 64 << 10
    src = corpora.corpus("J", 12 * nblk, bs)
    d_src = torch.from_numpy(src).cuda(0)
    blk_off = np.arange(nblk + 1, dtype=np.uint64) * bs
    streams = []
    for k in range(12):
        d_enc = _encode_stream(LEVELS[k % len(LEVELS)], d_src[k * nblk * bs:(k + 1) * nblk * bs], blk_off)
        streams.append(d_enc.cpu().numpy().tobytes())
    return streams, src


def test_host_buffer_entry_and_its_batches(kclib, twelve_streams):
    """The host-buffer entry gives the bytes of the _dev entry; with the scratch ceiling lowered the same bytes come from at least 3
    batches."""
    import torch
    from compress_amd import s2, _lib
    streams, src = twelve_streams
    buf, off = K.pack(streams)
    rd = s2.NewReader(None)
    try:
        d_in = torch.from_numpy(buf).cuda(0)
        d_out = torch.empty(len(src), dtype=torch.uint8, device="cuda:0")
        out_off, status = rd.DecodeStreamsDevice(d_in.data_ptr(), off, d_out.data_ptr(), len(src))
        assert not status.any() and int(out_off[-1]) == len(src)
        dev = d_out.cpu().numpy()
        assert np.array_equal(dev, src)
        outs = rd.DecodeStreams(buf, off)
        assert all(isinstance(o, bytes) for o in outs)
        assert b"".join(outs) == dev.tobytes()
        assert rd.ctx().get_option(_lib.OPT_LAST_BATCHES) == 1
        rd.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 320)  # a quarter of it per group: at most four streams (16 MiB decoded + their bytes each)
        outs = rd.DecodeStreams(buf, off)
        assert rd.ctx().get_option(_lib.OPT_LAST_BATCHES) >= 3
        assert all(isinstance(o, bytes) for o in outs)
        assert b"".join(outs) == dev.tobytes()
    finally:
        rd.Close()


def test_a_stream_that_cannot_fit(kclib, G, twelve_streams):
    """Host-buffer entry: an input whose bytes and decoded bytes exceed a quarter of the scratch ceiling gets KC_S2D_SIZE_EXCEEDED and a
    zero-filled planned range (include/kcgpu.h); its neighbours decode."""
    from compress_amd import s2, _lib
    streams, src = twelve_streams
    small = K.item1_streams(G)[0][1]
    inputs = [small, streams[0], small]
    buf, off = K.pack(inputs)
    rd = s2.NewReader(None)
    try:
        rd.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 32)
        ctx = rd.ctx()
        n = 3
        bound, st = rd.DecodeBounds(buf, off)
        assert [int(b) for b in bound] == [len(K.tom()), 256 * 65536, len(K.tom())] and not st.any()
        cap = int(bound.sum())
        dst = np.full(cap + 2 * K.GUARD, 0xA5, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        ctx.check(ctx.L.kc_s2_decode_streams(ctx.h, rd._o, buf.ctypes.data, off.ctypes.data, n, dst.ctypes.data + K.GUARD, cap, out_off.ctypes.data,
                                             status.ctypes.data))
        assert np.all(dst[:K.GUARD] == 0xA5) and np.all(dst[K.GUARD + cap:] == 0xA5)
        res = K.Result(0, dst[K.GUARD:K.GUARD + cap], out_off, status, bound)
        assert [int(s) for s in status] == [K.OK, K.SIZE_EXCEEDED, K.OK]
        assert [int(x) for x in out_off] == [0, len(K.tom()), len(K.tom()) + 256 * 65536, cap]
        assert res.out(0) == K.tom() and res.out(2) == K.tom() and not np.any(np.frombuffer(res.out(1), dtype=np.uint8))
        outs = rd.DecodeStreams(buf, off)
        assert isinstance(outs[1], s2.S2DecodeError) and outs[1].name == "KC_S2D_SIZE_EXCEEDED"
    finally:
        rd.Close()


def test_python_interface(kclib, G):
    """s2.Decode / DecodedLen / DecodeConcurrent / DecodeStreams / DecodeBlocks, S2DecodeError carrying the class; what stays out raises."""
    from compress_amd import s2
    t = K.tom()
    blk = G.s2_encode(t)
    assert s2.DecodedLen(blk) == len(t) and s2.Decode(None, blk) == t
    with pytest.raises(s2.S2DecodeError) as e:
        s2.Decode(None, blk[:-3])
    assert e.value.name == "KC_S2D_CORRUPT"
    with pytest.raises(s2.S2DecodeError):
        s2.DecodedLen(b"\xff\xff\xff\xff\xff\x01")
    good = G.s2_stream(t, block_size=4 << 10)
    bad_crc = bytearray(good)
    bad_crc[K.data_chunks(good)[2][0] + 5] ^= 1
    bad_type = bytearray(good)
    bad_type[K.data_chunks(good)[3][0]] = 0x05
    rd = s2.NewReader(io.BytesIO(good), s2.ReaderAllocBlock(4096))
    try:
        w = io.BytesIO()
        assert rd.DecodeConcurrent(w, 0) == len(t) and w.getvalue() == t
        rd.Reset(io.BytesIO(bytes(bad_crc)))
        w = io.BytesIO()
        with pytest.raises(s2.S2DecodeError) as e:
            rd.DecodeConcurrent(w)
        assert e.value.name == "KC_S2D_CRC" and w.getvalue() == b""
        inputs = [good, bytes(bad_crc), bytes(bad_type), good[:-5], b""]
        buf, off = K.pack(inputs)
        outs = rd.DecodeStreams(buf, off)
        assert outs[0] == t and outs[4] == b""
        assert [o.name for o in outs[1:4]] == ["KC_S2D_CRC", "KC_S2D_UNSUPPORTED", "KC_S2D_CORRUPT"]
        for o, s in zip(outs[1:4], inputs[1:4]):
            assert judged(G, s) == ("err", o.status)
        bbuf, boff = K.pack([blk, blk[:100], G.s2_encode(t[:5000], level=2)])
        bouts = rd.DecodeBlocks(bbuf, boff)
        assert bouts[0] == t and isinstance(bouts[1], s2.S2DecodeError) and bouts[2] == t[:5000]
        for call in (lambda: rd.Read(bytearray(10)), lambda: rd.Skip(5), lambda: rd.ReadSeeker(), lambda: rd.ReadByte(),
                     lambda: s2.NewReader(None, s2.ReaderSkippableCB(0x80, None))):
            with pytest.raises(NotImplementedError):
                call()
        for bad in (lambda: s2.ReaderMaxBlockSize(0), lambda: s2.ReaderMaxBlockSize((4 << 20) + 1), lambda: s2.ReaderAllocBlock(100)):
            with pytest.raises(ValueError):
                bad()
    finally:
        rd.Close()
