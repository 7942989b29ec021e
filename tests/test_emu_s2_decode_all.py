"""The s2.Reader / s2.Decode kernels (kc_s2_plan.hip, kc_s2_decode_all.hip) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_s2_decode_streams / kcemu_s2_decode_blocks_all — plan, decode, CRC, verdict, zero-fill as one batch) against the reference's own
Reader and Decode (translated: oracle_goref.s2_read_stream / s2_decode).  The cases are those of tests/s2_decode_cases.py."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import s2_decode_cases as K


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference reader) is not built")
    return oracle_goref


def run(inputs, blocks=False, max_block=4 << 20, ignore_crc=False, ignore_id=False, cap=None):
    L = emu_lib.lib()
    vp = C.c_void_p
    L.kcemu_s2_decode_streams.restype = C.c_int
    L.kcemu_s2_decode_streams.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint64, vp, vp, vp]
    L.kcemu_s2_decode_blocks_all.restype = C.c_int
    L.kcemu_s2_decode_blocks_all.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp]
    n = len(inputs)
    src, off = K.pack(inputs)
    if cap is None:  # a first call with no room at all returns the layout: the bounds
        cap = int(run(inputs, blocks, max_block, ignore_crc, ignore_id, cap=0).bound.sum())
    dst = np.full(cap + 2 * K.GUARD, 0xA5, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    bound = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n + 1, dtype=np.uint32)
    if blocks:
        rc = L.kcemu_s2_decode_blocks_all(src.ctypes.data, off.ctypes.data, n, dst.ctypes.data + K.GUARD, cap, out_off.ctypes.data, bound.ctypes.data,
                                          status.ctypes.data)
    else:
        rc = L.kcemu_s2_decode_streams(src.ctypes.data, off.ctypes.data, n, max_block, emu_lib_max_buf(max_block), int(ignore_crc), int(ignore_id),
                                       dst.ctypes.data + K.GUARD, cap, out_off.ctypes.data, bound.ctypes.data, status.ctypes.data)
    assert np.all(dst[:K.GUARD] == 0xA5) and np.all(dst[K.GUARD + cap:] == 0xA5), "written outside dst"
    if rc != 0:
        assert np.all(dst == 0xA5), "dst touched by a call that failed"
    return K.Result(rc, dst[K.GUARD:K.GUARD + cap], out_off, status[:n], bound[:n])


def emu_lib_max_buf(max_block):
    """MaxEncodedLen(max_block) + 4 (s2/encode.go:389-418, s2/reader.go:42)."""
    n = int(max_block)
    n += (n.bit_length() + 7) // 7
    n += 0 if max_block == 0 else 1 if max_block < 60 else 2 if max_block < 1 << 8 else 3 if max_block < 1 << 16 else 4 if max_block < 1 << 24 else 5
    return n + 4


def test_max_buf_is_the_references(G):
    for n in (1, 59, 60, 255, 256, 4096, 65535, 65536, 1 << 20, 4 << 20):
        assert emu_lib_max_buf(n) == G.s2_max_encoded_len(n) + 4, n


def test_one_batch_of_everything(G):
    items = K.item1_streams(G)
    verdicts = [K.judge_stream(G, s, 1 << 20) for _, s, _ in items]
    for (name, _, want), (kind, got) in zip(items, verdicts):
        assert kind == "ok" and got == want, name
    res = run([s for _, s, _ in items])
    ok, _ = K.check(res, verdicts)
    assert ok == len(items)
    assert [int(b) for b in res.bound] == [len(w) for _, _, w in items]


def test_sizes_at_the_limits(kclib, G):
    import corpora
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


def test_hand_built_blocks(G):
    hand = K.hand_blocks(G)
    named = hand + K.regression_blocks()
    raw = open(K.S2IN + "/Mark.Twain-Tom.Sawyer.txt.rawsnappy", "rb").read()
    named.append(("rawsnappy", raw))
    blocks = [b for _, b in named]
    verdicts = [K.judge_block(G, b, 1 << 20) for b in blocks]
    assert all(k == "ok" for k, _ in verdicts[:len(hand)]), [nm for (nm, _), (k, _) in zip(named, verdicts) if k != "ok"]
    assert verdicts[-1] == ("ok", K.tom()[:len(K.tom()) // 2])
    res = run(blocks, blocks=True)
    ok, _ = K.check(res, verdicts, "bare blocks")
    assert ok >= len(hand) + 1
    # the same as chunks of one stream each (those that decode; a chunk holds at most 4 MiB)
    streams, sv = [], []
    for b, (k, v) in zip(blocks, verdicts):
        if k == "ok":
            streams.append(K.MAGIC + K.chunk_of(b, v))
            sv.append(K.judge_stream(G, streams[-1], 1 << 20))
            assert sv[-1] == ("ok", v)
        else:
            streams.append(K.MAGIC + K.chunk_of(b, b""))
            sv.append(K.judge_stream(G, streams[-1], 1 << 20))
            assert sv[-1][0] == "err"
    K.check(run(streams), sv, "chunks")


def test_literal_of_16_mib_in_a_bare_block(G):
    """The 5-byte literal tag: one literal of 16 777 217 bytes."""
    lit = np.random.default_rng(5).integers(0, 256, 16777217, dtype=np.uint8).tobytes()
    blk = K.uvarint(len(lit)) + G.s2_emit("literal", 0, 0, lit)
    assert blk[len(K.uvarint(len(lit)))] == 63 << 2
    v = K.judge_block(G, blk, len(lit))
    assert v == ("ok", lit)
    K.check(run([blk], blocks=True), [v])


@pytest.mark.parametrize("ignore_crc", [False, True])
def test_mutations(G, ignore_crc):
    """480 mutations, seed 0x52D0001, of the first eight streams of the batch of everything (s2_decode_cases.mutations).  The reference
    alone gives for this recipe: with CRC checking 301 corrupt, 162 CRC, 13 unsupported, 4 decode; with ignore_crc 128 decode (108 of
    them to bytes other than the source), 313 corrupt, 39 unsupported."""
    bases = [s for _, s, _ in K.item1_streams(G)[:8]]
    muts = K.mutations(bases)
    verdicts = [K.judge_stream(G, m, 1 << 20, ignore_crc=ignore_crc) for m in muts]
    res = run(muts, ignore_crc=ignore_crc)
    ok, classes = K.check(res, verdicts)
    if ignore_crc:
        assert ok >= 96, ok
    else:
        assert all(classes.get(c, 0) >= 10 for c in (K.CORRUPT, K.CRC, K.UNSUPPORTED)), classes


def test_first_error_wins_in_stream_order(G):
    cases = K.first_error_cases(G)
    verdicts = [K.judge_stream(G, s, 1 << 20) for _, s, _ in cases]
    assert verdicts == [("err", want) for _, _, want in cases]
    K.check(run([s for _, s, _ in cases]), verdicts)


def test_refusals_between_good_neighbours(G):
    items = K.item1_streams(G)
    bases = [s for _, s, _ in items[:8]]
    bad = [m for m in K.mutations(bases) if K.judge_stream(G, m, 1 << 20)[0] == "err"][:16]
    assert len(bad) == 16
    inputs = []
    for i, (_, s, _) in enumerate(items):
        inputs.append(s)
        inputs.append(bad[i])
    inputs += bad[len(items):]
    verdicts = [K.judge_stream(G, s, 1 << 20) for s in inputs]
    res = run(inputs)
    ok, classes = K.check(res, verdicts)
    assert ok == len(items) and sum(classes.values()) == 16
    total = int(res.out_off[-1])
    short = run(inputs, cap=total - 1)  # (run() checks that dst is untouched)
    assert short.rc == K.DST_TOO_SMALL


def test_budget_cuts_change_nothing(G):
    """The batch of refusals between good neighbours, with the first-error streams behind it, as one device batch and again under the
    least scratch budget the largest input fits alone (its chunk records plus the 1/8 allowance, as the sequence reports it): at
    least three batches; the same bytes, layout, bounds and statuses.  s2.Reader's device form never refuses an input for size."""
    items = K.item1_streams(G)
    bad = [m for m in K.mutations([s for _, s, _ in items[:8]]) if K.judge_stream(G, m, 1 << 20)[0] == "err"][:len(items)]
    inputs = [x for pair in zip([s for _, s, _ in items], bad) for x in pair] + [s for _, s, _ in K.first_error_cases(G)]
    one = run(inputs)
    assert one.rc == 0 and emu_lib.last_batches() == 1
    need = emu_lib.last_max_need()
    assert 0 < need < (1 << 20)
    with emu_lib.scratch_budget(need):
        cut = run(inputs, cap=len(one.dst))
        batches = emu_lib.last_batches()
    assert batches >= 3, batches
    assert cut.rc == 0 and np.array_equal(cut.dst, one.dst) and np.array_equal(cut.out_off, one.out_off)
    assert np.array_equal(cut.status, one.status) and np.array_equal(cut.bound, one.bound)
    assert (one.status == 0).sum() >= len(items) and (one.status != 0).sum() >= len(bad)
