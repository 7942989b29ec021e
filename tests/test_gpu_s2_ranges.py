"""Ranged reads on the device through the C ABI (kc_s2_read_ranges[_dev], compress_amd.s2.Reader.ReadRanges[Device], s2.NewReadSeeker):
batches of (stream, offset, length) requests served through the S2 index, judged by the reference's own Reader (translated:
oracle_goref.s2_read_stream).  The cases are those of tests/s2_range_cases.py, the ones the CPU wave emulator runs too
(tests/test_emu_s2_ranges.py), plus what needs the library: the host-buffer form and its batches, the Python cursor."""
import io

import numpy as np
import pytest

import s2_decode_cases as K
import s2_range_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own s2.Reader, translated) is the judge of these tests"
    return oracle_goref


def _reader(max_block=4 << 20, ignore_crc=False, ignore_id=False):
    from compress_amd import s2
    opts = [s2.ReaderMaxBlockSize(max_block)]
    if ignore_crc:
        opts.append(s2.ReaderIgnoreCRC())
    if ignore_id:
        opts.append(s2.ReaderIgnoreStreamIdentifier())
    return s2.NewReader(None, *opts)


def run(streams, indexes, requests, cap=None, **kw):
    """One device-resident batch through Reader.ReadRangesDevice: 64 guard bytes of 0xA5 on both sides of dst."""
    import torch
    from compress_amd import KcError
    rd = _reader(**kw)
    try:
        m = len(requests)
        src, off = K.pack(streams)
        d_src = torch.from_numpy(src).cuda(0)
        if cap is None:
            cap = sum(r[2] for r in requests)
        d_all = torch.full((cap + 2 * R.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc, out_off, got, status = 0, np.zeros(m + 1, dtype=np.uint64), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
        try:
            out_off, got, status = rd.ReadRangesDevice(d_src.data_ptr(), off, requests, d_all.data_ptr() + R.GUARD, cap, indexes)
        except KcError as e:
            rc = e.status
        host = d_all.cpu().numpy()
    finally:
        rd.Close()
    assert np.all(host[:R.GUARD] == 0xA5) and np.all(host[R.GUARD + cap:] == 0xA5), "written outside dst"
    if rc != 0:
        assert np.all(host == 0xA5), "dst touched by a call that failed"
    return R.RResult(rc, host[R.GUARD:R.GUARD + cap], out_off, got, status)


def run_host(streams, indexes, requests, scratch_mib=None, **kw):
    """The same through the host-buffer entry (kc_s2_read_ranges), straight through the C ABI with guards round dst."""
    from compress_amd import _lib, s2
    rd = _reader(**kw)
    try:
        if scratch_mib:
            rd.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, scratch_mib)
        m = len(requests)
        src, off = K.pack(streams)
        cap = sum(r[2] for r in requests)
        real = rd._ranges

        def guarded(fn, src_ptr, in_off, rq, ix, dst_ptr, dst_cap):  # ReadRanges with guard bytes round its dst
            dst = np.full(cap + 2 * R.GUARD, 0xA5, dtype=np.uint8)
            out = real(fn, src_ptr, in_off, rq, ix, dst.ctypes.data + R.GUARD, cap)
            assert np.all(dst[:R.GUARD] == 0xA5) and np.all(dst[R.GUARD + cap:] == 0xA5), "written outside dst"
            guarded.res = R.RResult(0, dst[R.GUARD:R.GUARD + cap], *out)
            return out

        rd._ranges = guarded
        rd.ReadRanges(src, off, requests, indexes)
        return guarded.res, rd.ctx().get_option(_lib.OPT_LAST_BATCHES)
    finally:
        rd.Close()


def test_one_batch_of_everything(kclib, G):
    streams, indexes, requests, want = R.everything(G)
    classes = R.check(run(streams, indexes, requests), requests, want)
    assert all(classes.get(c, 0) >= 10 for c in (R.OK, R.EOF, R.UNEXPECTED_EOF)), classes


def test_the_same_batch_through_the_host_buffer_form(kclib, G):
    """kc_s2_read_ranges stages per request only the bytes its index entry points at; with the scratch ceiling lowered the same
    answers come from several groups."""
    streams, indexes, requests, want = R.everything(G)
    res, batches = run_host(streams, indexes, requests)
    R.check(res, requests, want)
    res2, batches2 = run_host(streams, indexes, requests, scratch_mib=16)  # a quarter of it per group: the 3 MiB stream's unindexed reads fill one
    R.check(res2, requests, want)
    assert batches2 > batches >= 1


def test_corrupt_input_under_a_dense_index(kclib, G):
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
    R.check(run([c[0] for c in cases], [c[1] for c in cases], requests), requests, want)


def test_the_skipped_region_of_the_3_mib_stream(kclib, G):
    """A walk from the index entry at 1 MiB to a range ten chunks behind it: a reserved chunk type in a skipped chunk's header is
    KC_S2D_UNSUPPORTED (reader.go:826); a flipped body byte in a skipped compressed chunk is not noticed (reader.go:671); a range in
    front of the bad header is served."""
    big = R.big_stream(G)
    dec = R.decoded(G, big)
    tab = R.chunk_table(big)
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


def test_reader_options_and_api_edges(kclib, G):
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
    rq2 = [(0, 10, 100), (0, 0, 50)]
    assert run([s], None, rq2, cap=149).rc == R.DST_TOO_SMALL  # (run() checks that dst and the guards are untouched)
    assert run([s], None, []).rc == 0
    assert run([], None, []).rc == 0
    assert run([s], None, [(1, 0, 1)]).rc == R.BAD_ARG
    assert run([], None, [(0, 0, 0)]).rc == R.BAD_ARG


def test_python_index_and_index_stream(kclib, G):
    from compress_amd import s2
    big = R.big_stream(G)
    x = R.writer_index(big)
    ix = s2.Index()
    assert ix.Load(x + b"rest") == b"rest"
    assert [u for _, u in ix.info] == [0, 1 << 20, 2 << 20] and ix.TotalUncompressed == 3 << 20
    assert ix.append_to(ix.TotalUncompressed, ix.TotalCompressed) == x
    ix2 = s2.Index()
    ix2.LoadStream(big)
    assert ix2.info == ix.info and ix2.Find((1 << 20) + 5) == tuple(ix.info[1]) and ix2.Find(-1) == tuple(ix.info[2])
    with pytest.raises(s2.S2DecodeError) as e:
        ix2.Find((3 << 20) + 1)
    assert e.value.name == "KC_S2D_UNEXPECTED_EOF"
    import json
    j = json.loads(ix.JSON())
    assert j["total_uncompressed"] == 3 << 20 and j["offsets"][1] == {"compressed": ix.info[1][0], "uncompressed": 1 << 20} and j["est_block_uncompressed"] == 65536
    assert s2.IndexStream(big[:-len(x)]) == x and s2.IndexStream(io.BytesIO(big[:-len(x)])) == x
    with pytest.raises(s2.S2DecodeError) as e:
        s2.IndexStream(big[10:])
    assert e.value.name == "KC_S2D_CORRUPT"
    for name, b, want, rest in R.load_cases():
        if want:
            with pytest.raises(s2.S2DecodeError) as e:
                s2.Index().Load(b)
            assert e.value.status == want, name
        else:
            assert s2.Index().Load(b) == rest, name


def test_read_seeker_cursor(kclib, G):
    """s2.NewReadSeeker: ReadAt then Read continues where ReadAt stopped (reader.go:859); Seek from the start, the current position and
    the end; a Seek before the start raises; without an index random=True is refused and random=False is forward-only; the unchanged
    Reader.ReadSeeker still raises."""
    from compress_amd import s2
    big = R.big_stream(G)
    dec = R.decoded(G, big)
    M = 1 << 20
    rs = s2.NewReadSeeker(big)
    try:
        p = bytearray(1000)
        assert rs.ReadAt(p, M + 77) == 1000 and bytes(p) == dec[M + 77:M + 1077]
        q = bytearray(500)
        assert rs.Read(q) == 500 and bytes(q) == dec[M + 1077:M + 1577]
        assert rs.Seek(-77, s2.SeekCurrent) == M + 1500
        assert rs.ReadByte() == dec[M + 1500]
        assert rs.Seek(-10, s2.SeekEnd) == 3 * M - 10
        p = bytearray(100)
        assert rs.Read(p) == 10 and bytes(p[:10]) == dec[-10:] and rs.Read(p) == 0
        with pytest.raises(EOFError):
            rs.ReadByte()
        assert rs.Seek(5, s2.SeekStart) == 5
        rs.Skip(65536)
        assert rs.ReadByte() == dec[65541]
        with pytest.raises(ValueError):
            rs.Seek(-1, s2.SeekStart)
        with pytest.raises(ValueError):
            rs.Seek(-3 * M - 1, s2.SeekEnd)
        with pytest.raises(s2.S2DecodeError) as e:
            rs.Seek(3 * M + 1, s2.SeekStart)
        assert e.value.name == "KC_S2D_UNEXPECTED_EOF"
        with pytest.raises(s2.S2DecodeError) as e:
            rs.Skip(3 * M)
        assert e.value.name == "KC_S2D_UNEXPECTED_EOF"
        assert rs.ReadAt(p, 3 * M - 3) == 3
    finally:
        rs.Close()
    plain = big[:-len(R.writer_index(big))]
    with pytest.raises(s2.ErrCantSeek):
        s2.NewReadSeeker(plain)
    with pytest.raises(s2.ErrCantSeek):
        s2.NewReadSeeker(plain, index=b"\x99\x00\x00\x00 not an index at all")
    rs = s2.NewReadSeeker(io.BytesIO(plain), index=R.writer_index(big))  # a supplied index wins
    try:
        p = bytearray(64)
        assert rs.ReadAt(p, 2 * M + 3) == 64 and bytes(p) == dec[2 * M + 3:2 * M + 67]
        assert rs.Seek(-1, s2.SeekEnd) == 3 * M - 1
    finally:
        rs.Close()
    fw = s2.NewReadSeeker(plain, random=False)
    try:
        assert fw.Seek(70000, s2.SeekStart) == 70000
        p = bytearray(10)
        assert fw.Read(p) == 10 and bytes(p) == dec[70000:70010]
        assert fw.Seek(5, s2.SeekCurrent) == 70015
        with pytest.raises(s2.S2DecodeError) as e:
            fw.Seek(100, s2.SeekStart)  # backward
        assert e.value.name == "KC_S2D_UNSUPPORTED"
        with pytest.raises(s2.S2DecodeError):
            fw.Seek(-1, s2.SeekEnd)  # no index: no end to count from (reader.go:941)
    finally:
        fw.Close()
    rd = s2.NewReader(io.BytesIO(big))
    try:
        with pytest.raises(NotImplementedError):
            rd.ReadSeeker()
    finally:
        rd.Close()
