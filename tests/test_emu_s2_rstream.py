"""The S2 stream reader (kc_s2_rstream.hip, kc_s2rstream_host.h) on the CPU wave emulator (tools/hipemu/kcemu.cpp: kcemu_s2_rstream_new /
_feed / _skip / _skip_left / _on_skippable / _reset / _free — the product's state machine over plain memory), judged by the reference's
own sequential Reader (translated: oracle_goref.s2_read_stream).  The cases are those of tests/s2_rstream_cases.py."""
import ctypes as C

import pytest

import s2_rstream_cases as R


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference reader) is not built")
    return oracle_goref


@pytest.fixture(scope="module")
def S():
    import emu_lib
    L = emu_lib.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.kcemu_s2_rstream_new.restype = vp
    L.kcemu_s2_rstream_new.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32]
    L.kcemu_s2_rstream_feed.restype = C.c_int
    L.kcemu_s2_rstream_feed.argtypes = R.FEED_ARGS
    L.kcemu_s2_rstream_skip.restype = C.c_int
    L.kcemu_s2_rstream_skip.argtypes = [vp, u64]
    L.kcemu_s2_rstream_skip_left.restype = u64
    L.kcemu_s2_rstream_skip_left.argtypes = [vp]
    L.kcemu_s2_rstream_on_skippable.restype = C.c_int
    L.kcemu_s2_rstream_on_skippable.argtypes = [vp, C.c_uint8, R.SKIPPABLE_FN, vp]
    L.kcemu_s2_rstream_reset.restype = C.c_int
    L.kcemu_s2_rstream_reset.argtypes = [vp]
    L.kcemu_s2_rstream_free.restype = None
    L.kcemu_s2_rstream_free.argtypes = [vp]

    def new(chunks=4096, max_block=4 << 20, ignore_crc=False, ignore_id=False):
        return L.kcemu_s2_rstream_new(max_block, R.max_buf(max_block), int(ignore_crc), int(ignore_id), chunks)
    return R.Api(new, L.kcemu_s2_rstream_feed, L.kcemu_s2_rstream_skip, L.kcemu_s2_rstream_skip_left, L.kcemu_s2_rstream_on_skippable,
                 L.kcemu_s2_rstream_reset, L.kcemu_s2_rstream_free)


def test_max_buf_is_the_references(G):
    for n in (1, 59, 60, 255, 256, 4096, 65535, 65536, 1 << 20, 4 << 20):
        assert R.max_buf(n) == G.s2_max_encoded_len(n) + 4, n


@pytest.mark.parametrize("piece", (None, 1000, 7, 1))
def test_item1_streams(G, S, piece):
    R.t_item1(G, S, (piece,), (4096, 3, 1))


@pytest.mark.parametrize("piece", (None, 1000))
def test_mutations_class_and_prefix(G, S, piece):
    R.check_mutations(G, S, piece)


def test_end_rules(G, S):
    R.t_end_rules(G, S)


def test_limits(G, S):
    import corpora
    t4 = corpora.corpus("T", 1, 4 << 20).tobytes()
    R.t_limits(G, S, (t4, G.s2_stream(t4, block_size=4 << 20)))


def test_refusal_consumes_nothing_behind_progress(G, S):
    R.t_refusal_behind_progress(G, S)


def test_callback_removed_in_flight(G, S):
    R.t_callback_removed_in_flight(G, S)


def test_skip(G, S):
    R.t_skip(G, S)


def test_callbacks(G, S):
    R.t_callbacks(G, S)


def test_reset_keeps_options_and_callbacks(G, S):
    R.t_reset(G, S)
