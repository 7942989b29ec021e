"""The stateless writers on the device (kc_flate_stateless_deflate*, kc_gzip_stateless_deflate*, compress_amd.flate / compress_amd.gzip):
every case of tests/stateless_cases.py device-resident through the C ABI and through the Python API's host-buffer forms, against the
model (tests/stateless_model.py): bytes, out_off and the bound, behind 0xA5 guards on both sides of a dst that is not word-aligned.
The device's output goes back through the device's own inflate; many short inputs in one batch and one input of many blocks, across a
group cut under a small scratch budget."""
import gzip as host_gzip
import io
import zlib

import numpy as np
import pytest

import deflate_cases as D
import stateless_cases as S
import stateless_model as M

pytestmark = pytest.mark.gpu
GUARD = 37  # odd: dst + GUARD is not word-aligned
ALL = S.all_cases()


def groups(cases):
    g = {}
    for c in cases:
        g.setdefault((c[2], c[3]), []).append(c)
    return g


GROUPS = groups(ALL)
KEYS = sorted(GROUPS, key=lambda k: (not k[0], len(k[1]), k[1]))


def run_device(datas, gz, eof=True, dic=b"", cap=None, scratch_mib=None):
    """One device-resident call: (rc, outputs or None, out_off, batches).  Checks the guards, and that a refused call wrote nothing."""
    import torch
    from compress_amd import KcError, _lib, flate
    src, off = D.pack(datas)
    d_src = torch.from_numpy(np.concatenate([src, np.zeros(1, dtype=np.uint8)])).cuda(0)
    b = flate.StatelessBatch("kc_gzip_stateless_deflate" if gz else "kc_flate_stateless_deflate", eof, dic)
    try:
        if scratch_mib is not None:
            b.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, scratch_mib)
        bound = b.bound(off)
        assert bound == sum(M.bound(len(d), 0 if gz else len(dic)) + (20 if gz else 0) for d in datas)
        if cap is None:
            cap = bound
        d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc, out_off = 0, None
        try:
            out_off = b.deflate(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap, True)
        except KcError as e:
            rc, out_off = e.status, e.out_off
        batches = b.ctx().get_option(_lib.OPT_LAST_BATCHES)
        host = d_all.cpu().numpy()
    finally:
        b.close()
    assert np.all(host[:GUARD] == 0xA5), "written in front of dst"
    if rc != 0:
        assert np.all(host == 0xA5), "dst touched by a call that failed"
        return rc, None, out_off, batches
    total = int(out_off[-1])
    assert total <= cap and np.all(host[GUARD + total:] == 0xA5), "written behind the output"
    return 0, [host[GUARD + int(out_off[i]):GUARD + int(out_off[i + 1])].tobytes() for i in range(len(datas))], out_off, batches


def check(cs, outs, out_off, wants):
    at = 0
    bad = []
    for i, c in enumerate(cs):
        if outs[i] != wants[i] or int(out_off[i]) != at:
            bad.append((c[0], len(outs[i]), len(wants[i]), int(out_off[i]), at))
        at += len(wants[i])
    assert not bad, bad[:10]
    assert int(out_off[len(cs)]) == at


def test_all_cases_device(kclib):
    """Every case, one device-resident call per (eof, dict) with all its inputs mixed in one batch."""
    for key in KEYS:
        cs = GROUPS[key]
        rc, outs, out_off, _ = run_device([c[1] for c in cs], False, key[0], key[1])
        assert rc == 0
        check(cs, outs, out_off, [S.model(c).data for c in cs])


def test_gzip_device(kclib):
    """Write + Close per input: every third case, in one call."""
    cs = ALL[::3]
    rc, outs, out_off, _ = run_device([c[1] for c in cs], True)
    assert rc == 0
    check(cs, outs, out_off, [S.model_gzip(c) for c in cs])


def test_python_api(kclib):
    """The host-buffer forms through compress_amd.flate.StatelessDeflateAll / compress_amd.gzip.GzipAll."""
    from compress_amd import flate, gzip
    for key in KEYS:
        cs = GROUPS[key]
        src, off = D.pack([c[1] for c in cs])
        assert flate.StatelessDeflateAll(src, off, key[0], key[1]) == [S.model(c).data for c in cs]
    cs = ALL[1::7]
    src, off = D.pack([c[1] for c in cs])
    assert gzip.GzipAll(src, off, gzip.StatelessCompression) == [S.model_gzip(c) for c in cs]


def test_capacity(kclib):
    from compress_amd import _lib
    cs = [c for c in GROUPS[(True, b"")] if len(c[1]) <= 1000]
    for gz in (False, True):
        wants = [S.model_gzip(c) if gz else S.model(c).data for c in cs]
        total = sum(len(w) for w in wants)
        rc, outs, out_off, _ = run_device([c[1] for c in cs], gz, cap=total)
        assert rc == 0
        check(cs, outs, out_off, wants)
        rc, outs, out_off, _ = run_device([c[1] for c in cs], gz, cap=total - 1)
        assert rc == _lib.KC_ERR_DST_TOO_SMALL and int(out_off[len(cs)]) == total


def test_device_inflates_what_it_wrote(kclib):
    """The eof cases written on the device and read by the device's own InflateAll / GunzipAll (with the dictionary where one was
    given), and by CPython."""
    from compress_amd import flate, gzip
    pack = lambda outs: (np.frombuffer(b"".join(outs), dtype=np.uint8), np.cumsum([0] + [len(o) for o in outs]).astype(np.uint64))  # noqa: E731
    for key in KEYS:
        if not key[0]:
            continue
        cs = GROUPS[key]
        src, off = D.pack([c[1] for c in cs])
        outs = flate.StatelessDeflateAll(src, off, True, key[1])
        back = flate.InflateAll(*pack(outs), dict=key[1] or None)
        for c, got in zip(cs, back):
            if c[0] in S.NO_FINAL_BLOCK:   # a stream without a final block, as the reference writes it: the input ends inside the stream
                assert isinstance(got, flate.ErrUnexpectedEOF), c[0]
            else:
                assert got == c[1], c[0]
        assert key[1] or sum(c[0] in S.NO_FINAL_BLOCK for c in cs) == len(S.NO_FINAL_BLOCK)
    cs = GROUPS[(True, b"")][::2]
    src, off = D.pack([c[1] for c in cs])
    outs = gzip.GzipAll(src, off, gzip.StatelessCompression)
    assert gzip.GunzipAll(*pack(outs)) == [c[1] for c in cs]
    assert all(host_gzip.decompress(o) == c[1] for o, c in zip(outs, cs))


def test_many_short_inputs_and_many_blocks_across_group_cuts(kclib):
    """One batch of 1 024 inputs of 1 .. 4 096 bytes and one input of 2 MiB (84 blocks in one chain), under a scratch budget of
    12 MiB: the call is cut into groups of inputs and writes the same bytes."""
    rng = np.random.default_rng(1024)
    lens = rng.integers(1, 4097, size=1024)
    lens[:8] = (1, 12, 13, 4096, 4095, 14, 3, 64)
    datas = []
    at = 0
    for k, n in enumerate(lens):
        datas.append(rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() if k % 5 == 0 else D.text(int(n), 12345 + at))
        at += int(n)
    big = np.frombuffer(D.text(2 << 20, 4242), dtype=np.uint8).copy()
    for a in (3 << 15, 20 << 15, 21 << 15):
        big[a:a + 50000] = rng.integers(0, 256, size=50000, dtype=np.uint8)
    big[40 << 15:(40 << 15) + 100000] = 7
    datas.insert(500, big.tobytes())
    rc, outs, out_off, batches = run_device(datas, False, scratch_mib=12)
    assert rc == 0 and batches > 1
    for k, d in enumerate(datas):
        assert zlib.decompress(outs[k], -15) == d, k
    for k in list(range(0, len(datas), 41)) + [500]:  # the model on a sample (it is the slow side)
        assert outs[k] == M.stateless_deflate(datas[k]), k
    res = M.stateless_deflate_ex(datas[500])
    assert all(res.counts[k] > 0 for k in ("stored-no-match", "dyn-first-table", "cannot-reuse"))
    rc, outs1, _, batches1 = run_device(datas[495:505], True)
    assert rc == 0 and batches1 == 1 and outs1 == [M.gzip_stateless(d) for d in datas[495:505]]


def test_writer_objects(kclib):
    from compress_amd import KcError, flate, gzip
    data = D.text(70001, 99)
    w = io.BytesIO()
    fw = flate.NewStatelessWriter(w)
    fw.Write(data[:1000])
    fw.Write(data[1000:])
    fw.Close()
    fw.Close()
    want = M.stateless_deflate(data[:1000], False) + M.stateless_deflate(data[1000:], False) + M.stateless_deflate(b"", True)
    assert w.getvalue() == want and zlib.decompress(want, -15) == data
    w2 = io.BytesIO()
    fw.Reset(w2)
    fw.Close()
    assert w2.getvalue() == bytes([3, 0])
    w = io.BytesIO()
    flate.StatelessDeflate(w, data, True, data[:5000])
    assert w.getvalue() == M.stateless_deflate(data, True, data[:5000])
    w = io.BytesIO()
    gw = gzip.NewWriterLevel(w, gzip.StatelessCompression)
    gw.Write(data[:30000])
    assert gw.Flush() is None
    gw.Write(data[30000:])
    gw.Close()
    body = M.stateless_deflate(data[:30000], False) + M.stateless_deflate(data[30000:], False) + bytes([3, 0])
    assert w.getvalue()[:10] == M.GZIP_HEADER and w.getvalue()[10:-8] == body and host_gzip.decompress(w.getvalue()) == data
    w = io.BytesIO()
    gw = gzip.NewWriterLevel(w, gzip.StatelessCompression)
    gw.Write(data)
    gw.Close()
    assert w.getvalue() == M.gzip_stateless(data)
    w = io.BytesIO()
    gzip.NewWriterLevel(w, gzip.StatelessCompression).Close()
    assert w.getvalue() == M.gzip_stateless(b"")
    # the levels of flate.NewWriter stay as they were: stateless is no level of it, in the reference or here
    for level in (-3, -1, 0, 1, 6, 9):
        with pytest.raises(KcError):
            flate.NewWriter(io.BytesIO(), level)
    for level in (-1, 0, 1, 6, 9):
        with pytest.raises(KcError):
            gzip.GzipAll(np.zeros(1, dtype=np.uint8), np.array([0, 1], dtype=np.uint64), level)
        with pytest.raises(KcError):
            gzip.NewWriterLevel(io.BytesIO(), level)
