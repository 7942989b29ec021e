"""Ranged reads (kc_s2_ranges.hip: the ranged plan and the clipped decode) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_s2_read_ranges — Index.Find, plan, decode, CRC, verdict, zero-fills as one batch) and the index behind them (kc_s2_index.cpp,
plain host code) against the reference's own Reader and Writer (translated: oracle_goref.s2_read_stream / s2_stream).  The cases are
those of tests/s2_range_cases.py, the ones the device runs too (tests/test_gpu_s2_ranges.py)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import s2_decode_cases as K
import s2_range_cases as R


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference reader) is not built")
    return oracle_goref


def elib():
    from compress_amd import _lib
    L = emu_lib.lib()
    if not getattr(L, "_s2r", False):
        _lib.declare_s2_index(L)
        vp = C.c_void_p
        L.kcemu_s2_read_ranges.restype = C.c_int
        L.kcemu_s2_read_ranges.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint64, vp, vp, vp]
        L._s2r = True
    return L


def run(streams, indexes, requests, cap=None, max_block=4 << 20, ignore_crc=False, ignore_id=False):
    L = elib()
    ns, m = len(streams), len(requests)
    src, off = K.pack(streams)
    src = src[:max(len(src) - 1, 1)].copy()  # exactly the inputs (pack() pads one byte)
    handles = (C.c_void_p * max(ns, 1))()
    made = []
    try:
        for k, b in enumerate(indexes or []):
            if b is not None:
                h = L.kc_s2_index_new()
                made.append(h)
                assert L.kc_s2_index_load(h, bytes(b), len(b), None) == 0
                handles[k] = h
        rs = np.array([r[0] for r in requests] + [0], dtype=np.uint32)
        ro = np.array([r[1] for r in requests] + [0], dtype=np.uint64)
        rl = np.array([r[2] for r in requests] + [0], dtype=np.uint64)
        if cap is None:
            cap = int(rl[:m].sum())
        dst = np.full(cap + 2 * R.GUARD, 0xA5, dtype=np.uint8)
        out_off = np.zeros(m + 1, dtype=np.uint64)
        got = np.zeros(m + 1, dtype=np.uint64)
        status = np.zeros(m + 1, dtype=np.uint32)
        rc = L.kcemu_s2_read_ranges(src.ctypes.data, off.ctypes.data, ns, handles if indexes is not None else None, rs.ctypes.data, ro.ctypes.data,
                                    rl.ctypes.data, m, max_block, R.max_buf(max_block), int(ignore_crc), int(ignore_id),
                                    dst.ctypes.data + R.GUARD, cap, out_off.ctypes.data, got.ctypes.data, status.ctypes.data)
    finally:
        for h in made:
            L.kc_s2_index_free(h)
    assert np.all(dst[:R.GUARD] == 0xA5) and np.all(dst[R.GUARD + cap:] == 0xA5), "written outside dst"
    if rc != 0:
        assert np.all(dst == 0xA5), "dst touched by a call that failed"
    return R.RResult(rc, dst[R.GUARD:R.GUARD + cap], out_off, got[:m], status[:m])


def test_one_batch_of_everything(G):
    streams, indexes, requests, want = R.everything(G)
    classes = R.check(run(streams, indexes, requests), requests, want)
    assert all(classes.get(c, 0) >= 10 for c in (R.OK, R.EOF, R.UNEXPECTED_EOF)), classes


def test_budget_cuts_change_nothing(G):
    """The batch of everything as one device batch and again under the least scratch budget the largest request fits alone (its
    chunk records and clip slots plus the 1/8 allowance, as the sequence reports it): at least three batches; the same bytes,
    layout, `got` and statuses.  One byte less changes nothing either: the device form of the ranged reads never refuses a request
    for size — the one that does not fit runs as a batch of its own (only the host-buffer form has a ceiling, a quarter of the
    budget for a request's slice and range)."""
    streams, indexes, requests, want = R.everything(G)
    one = run(streams, indexes, requests)
    assert one.rc == 0 and emu_lib.last_batches() == 1
    need = emu_lib.last_max_need()
    assert 0 < need < (1 << 20)
    for budget in (need, need - 1):
        with emu_lib.scratch_budget(budget):
            cut = run(streams, indexes, requests)
            batches = emu_lib.last_batches()
        assert batches >= 3, (budget, batches)
        assert cut.rc == 0 and np.array_equal(cut.dst, one.dst) and np.array_equal(cut.out_off, one.out_off)
        assert np.array_equal(cut.got, one.got) and np.array_equal(cut.status, one.status)
    R.check(one, requests, want)


def test_corrupt_input_under_a_dense_index(G):
    """480 single-bit mutations, seed 0x52D0002, of the seven small streams read through their dense indexes (s2_range_cases.corrupt_cases);
    the judge is the reference's sequential Reader over the stream's identifier + mutated[first covered header : cut].  The reference
    alone gives for this recipe: kind (c) 160 OK of 160; kinds (a) and (b) together 261 CRC, 53 corrupt, 4 unsupported, 2 OK."""
    cases = R.corrupt_cases(G)
    want = [R.judge_range(G, ji, rel, rq[1]) for _, _, rq, _, ji, rel in cases]
    kinds = [c[3] for c in cases]
    assert all(w[0] == R.OK for w, k in zip(want, kinds) if k == "c")
    ab = [w[0] for w, k in zip(want, kinds) if k != "c"]
    assert ab.count(R.CORRUPT) >= 50 and ab.count(R.CRC) >= 50, {s: ab.count(s) for s in set(ab)}
    bases = [R.decoded(G, s) for _, s in R.small_streams(G)]
    for k, ((_, _, rq, kind, _, _), w) in enumerate(zip(cases, want)):
        if kind == "c":  # the pristine bytes
            assert w[1] == bases[k % len(bases)][rq[0]:rq[0] + rq[1]], k
    requests = [(k, rq[0], rq[1]) for k, (_, _, rq, _, _, _) in enumerate(cases)]
    res = run([c[0] for c in cases], [c[1] for c in cases], requests)
    R.check(res, requests, want)


def test_the_skipped_region_of_the_3_mib_stream(G):
    """A walk from the index entry at 1 MiB to a range ten chunks behind it: a reserved chunk type in a skipped chunk's header is
    KC_S2D_UNSUPPORTED (reader.go:826); a flipped body byte in a skipped compressed chunk is not noticed (reader.go:671); a range in
    front of the bad header is served."""
    big = R.big_stream(G)
    dec = R.decoded(G, big)
    tab = R.chunk_table(big)
    assert len(tab) == 48 and all(big[p] == 0 for p, _, _ in tab)
    off, ln = (1 << 20) + 10 * 65536 + 5, 3000
    bad_type = bytearray(big)
    bad_type[tab[20][0]] = 0x02
    bad_body = bytearray(big)
    bad_body[tab[20][0] + 100] ^= 0x10
    ix = R.writer_index(big)
    requests = [(0, off, ln), (1, off, ln), (2, off, ln), (1, (1 << 20) + 2 * 65536 + 9, 100)]
    want = [(R.OK, dec[off:off + ln]), (R.UNSUPPORTED, b""), (R.OK, dec[off:off + ln]), (R.OK, dec[(1 << 20) + 2 * 65536 + 9:][:100])]
    R.check(run([big, bytes(bad_type), bytes(bad_body)], [ix, ix, ix], requests), requests, want)
    R.check(run([bytes(bad_type), bytes(bad_body)], None, [(0, off, ln), (1, off, ln)]), [(0, off, ln), (1, off, ln)], want[1:3])


def test_reader_options(G):
    s = R.small_streams(G)[0][1]
    dec = R.decoded(G, s)
    dx = R.dense_index(s)
    tab = R.chunk_table(s)
    rq = [(0, 5000, 6000)]
    assert run([s], [dx], rq, max_block=2048).status[0] == R.CORRUPT
    b = bytearray(s)
    b[tab[1][0] + 4] ^= 1  # the stored CRC of a covered chunk
    assert run([bytes(b)], [dx], rq).status[0] == R.CRC
    R.check(run([bytes(b)], [dx], rq, ignore_crc=True), rq, [(R.OK, dec[5000:11000])])
    # no identifier at the front: refused from the start and from an index entry alike, unless identifiers are ignored
    cut = s[10:]
    from compress_amd import s2
    sh = s2.Index(4096)
    u = 0
    for p, _, dl in tab:
        sh.info.append([p - 10, u])
        u += dl
    shifted = sh.append_to(u, len(cut))
    for index in (None, [shifted]):
        assert run([cut], index, rq).status[0] == R.CORRUPT
        R.check(run([cut], index, rq, ignore_id=True), rq, [(R.OK, dec[5000:11000])])


def test_api_edges(G):
    s = R.small_streams(G)[0][1]
    rq = [(0, 10, 100), (0, 0, 50)]
    assert run([s], None, rq, cap=149).rc == R.DST_TOO_SMALL  # (run() checks that dst is untouched)
    assert run([s], None, []).rc == 0
    assert run([], None, []).rc == 0
    assert run([s], None, [(1, 0, 1)]).rc == R.BAD_ARG
    assert run([], None, [(0, 0, 0)]).rc == R.BAD_ARG


# ---- the index ----
def _load(b):
    """(status, entries, totals, est, rest) of kc_s2_index_load."""
    L = elib()
    h = L.kc_s2_index_new()
    try:
        used = C.c_uint64(0)
        rc = L.kc_s2_index_load(h, bytes(b), len(b), C.byref(used))
        n = L.kc_s2_index_entries(h, None, None, 0)
        c, u = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        L.kc_s2_index_entries(h, c.ctypes.data, u.ctypes.data, n)
        return rc, [(int(c[k]), int(u[k])) for k in range(n)], (L.kc_s2_index_total_uncompressed(h), L.kc_s2_index_total_compressed(h)), \
            L.kc_s2_index_est_block_uncompressed(h), bytes(b)[used.value:]
    finally:
        L.kc_s2_index_free(h)


def _index_stream(stream):
    L = elib()
    out = C.create_string_buffer(4096)
    n, st = C.c_uint64(0), C.c_uint32(0)
    assert L.kc_s2_index_stream(bytes(stream), len(stream), out, 4096, C.byref(n), C.byref(st)) == 0
    return st.value, out.raw[:n.value]


def test_load_of_the_writers_index(G):
    """Every entry (c, u) of the reference Writer's index: stream[c] is a data chunk header and the chunks in front of it decode to u
    bytes; append_to(Load(x)) == x."""
    from compress_amd import s2
    for stream in (R.big_stream(G), R.small_streams(G)[-1][1]):
        x = R.writer_index(stream)
        rc, entries, totals, est, rest = _load(x)
        assert rc == 0 and rest == b""
        dec = R.decoded(G, stream)
        assert totals[0] == len(dec)
        tab = R.chunk_table(stream)
        starts, u = {}, 0
        for p, _, dl in tab:
            starts[p] = u
            u += dl
        assert entries and all(starts.get(c) == uu and stream[c] <= 1 for c, uu in entries), entries
        for c, uu in entries:  # the reference's decode of the chunks in front of the entry
            assert len(R.decoded(G, stream[:c])) == uu
        w = s2.Index(est)
        w.info = [list(e) for e in entries]
        assert w.append_to(*totals) == x
    assert [e[1] for e in _load(R.writer_index(R.big_stream(G)))[1]] == [0, 1 << 20, 2 << 20]
    for _, s in R.small_streams(G):
        d = R.dense_index(s)
        rc, entries, totals, est, _ = _load(d)
        assert rc == 0 and entries == [(p, u) for (p, _, _), u in zip(R.chunk_table(s), R.bounds_of(s))]
        w = s2.Index(est)
        w.info = [list(e) for e in entries]
        assert w.append_to(*totals) == d


def test_load_stream_finds_the_index_behind_padding(G):
    L = elib()
    s = R.small_streams(G)[-1][1]
    assert any(s[p] == 0xfe for p in K.headers(s)), "no padding chunk in the stream"
    h = L.kc_s2_index_new()
    try:
        assert L.kc_s2_index_load_stream(h, s, len(s)) == 0
        assert L.kc_s2_index_total_uncompressed(h) == len(K.tom())
        c, u = C.c_int64(), C.c_int64()
        assert L.kc_s2_index_find(h, 5000, C.byref(c), C.byref(u)) == 0 and (c.value, u.value) == (10, 0)
        assert L.kc_s2_index_find(h, -1, C.byref(c), C.byref(u)) == 0
        assert L.kc_s2_index_find(h, len(K.tom()) + 1, C.byref(c), C.byref(u)) == R.UNEXPECTED_EOF
        assert L.kc_s2_index_find(h, -len(K.tom()) - 1, C.byref(c), C.byref(u)) == R.UNEXPECTED_EOF
        plain = R.small_streams(G)[0][1]
        assert L.kc_s2_index_load_stream(h, plain, len(plain)) == R.UNSUPPORTED
        assert L.kc_s2_index_load_stream(h, s[-9:], 9) == R.UNEXPECTED_EOF
    finally:
        L.kc_s2_index_free(h)
    big = R.big_stream(G)
    h = L.kc_s2_index_new()
    try:
        assert L.kc_s2_index_load_stream(h, big, len(big)) == 0
        tab = R.chunk_table(big)
        c, u = C.c_int64(), C.c_int64()
        for off, k in ((0, 0), ((1 << 20) - 1, 0), (1 << 20, 16), ((2 << 20) + 5, 32), (3 << 20, 32), (-1, 32), (-(2 << 20), 16)):
            assert L.kc_s2_index_find(h, off, C.byref(c), C.byref(u)) == 0 and (c.value, u.value) == (tab[k][0], k * 65536), off
    finally:
        L.kc_s2_index_free(h)


def test_index_stream_equals_the_writers_index(G):
    """IndexStream(stream without index) == the index the reference's Writer appended to the same data, for inputs of at least one
    block.  For an input shorter than a block the reference's two estimates of the block size differ (the Writer's is its block
    size, IndexStream's the first chunk's decoded length): there the comparison is with the Python Index port fed the chunk table."""
    from compress_amd import s2
    t = K.tom()
    data3 = (t * ((3 << 20) // len(t) + 1))[:3 << 20]
    for data, kw in ((t, dict(block_size=4 << 10)), (t, dict(block_size=4 << 10, level=3)), (t, dict(block_size=4 << 10, snappy=True)),
                     (data3, dict(block_size=64 << 10)), (data3[:(2 << 20) + 77], dict(block_size=1 << 20))):
        with_ix = G.s2_stream(data, add_index=True, **kw)
        x = R.writer_index(with_ix)
        plain = with_ix[:-len(x)]
        assert plain == G.s2_stream(data, **kw)
        assert _index_stream(plain) == (0, x), kw
    short = G.s2_stream(t[:1000], block_size=4 << 10)
    w = s2.Index(1000)
    w.add(10, 0)
    assert _index_stream(short) == (0, w.append_to(1000, len(short)))
    assert _index_stream(b"") == (0, s2.Index(0).append_to(0, 0))
    # IndexStream's own checks (index.go:437-511)
    s = G.s2_stream(t, block_size=4 << 10)
    tab = R.chunk_table(s)
    for name, mut, want in (("no identifier first", s[10:], R.CORRUPT), ("a padding chunk shorter than 4", s + b"\xfe\x03\x00\x00abc", R.CORRUPT),
                            ("truncated chunk", s[:-1], R.UNEXPECTED_EOF), ("truncated header", s + b"\x00\x01", R.UNEXPECTED_EOF),
                            ("reserved type", s + b"\x05\x04\x00\x00abcd", R.UNSUPPORTED), ("skippable", s + b"\x80\x04\x00\x00abcd", R.OK),
                            ("identifier of 7 bytes", s + b"\xff\x07\x00\x00S2sTwOx", R.CORRUPT), ("another magic", s + b"\xff\x06\x00\x00S2sTwX", R.CORRUPT)):
        assert _index_stream(mut)[0] == want, name
    big_dl = bytearray(s)
    big_dl[tab[0][0] + 8:tab[0][0] + 10] = b"\xff\xff"  # the first block's uvarint now says more than 4 MiB (or does not end)
    assert _index_stream(bytes(big_dl))[0] == R.CORRUPT


def test_every_return_of_index_load():
    """One case per return statement of Index.Load (s2/index.go:238-374), named by its line.  The cases and their expected results are
    hand-built from reading that code: no translated Load exists in the tree to judge them."""
    for name, b, want, rest in R.load_cases():
        rc, _, _, _, got_rest = _load(b)
        assert rc == want, (name, R.NAMES[rc])
        if rest is not None:
            assert got_rest == rest, name
