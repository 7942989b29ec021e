"""The HuffmanOnly writers on the device (kc_flate_deflate*, kc_gzip_deflate*, compress_amd.flate / compress_amd.gzip): every case of
tests/deflate_cases.py — the ones the CPU wave emulator runs (tests/test_emu_deflate.py) and the other 240 seeded ones —
device-resident through the C ABI and through the Python API's host-buffer forms, against the model (tests/deflate_model.py): bytes,
out_off and the bound, behind 0xA5 guards on both sides of a dst that is not word-aligned.  The device's output goes back through
the device's own inflate; many short chains in one batch; many blocks in one chain."""
import gzip as host_gzip
import io
import zlib

import numpy as np
import pytest

import deflate_cases as D
import deflate_model as M

pytestmark = pytest.mark.gpu
GUARD = 37  # odd: dst + GUARD is not word-aligned
ALL = D.directed() + D.seeded()
GROUPS = D.groups(ALL)


def run_device(datas, gz, key, cap=None):
    """One device-resident call: (rc, outputs or None, out_off).  Checks the guards, and that a refused call wrote nothing."""
    import torch
    from compress_amd import KcError, flate
    block, penalty, end = key
    src, off = D.pack(datas)
    d_src = torch.from_numpy(np.concatenate([src, np.zeros(1, dtype=np.uint8)])).cuda(0)
    b = flate.WriteBatch("kc_gzip_deflate" if gz else "kc_flate_deflate", flate.HuffmanOnly, end == M.END_FLUSH, block, penalty)
    try:
        bound = b.bound(off)
        assert bound == sum(M.bound(len(d), block) + (18 if gz else 0) for d in datas)
        if cap is None:
            cap = bound
        d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc, out_off = 0, None
        try:
            out_off = b.deflate(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap, True)
        except KcError as e:
            rc, out_off = e.status, e.out_off
        host = d_all.cpu().numpy()
    finally:
        b.close()
    assert np.all(host[:GUARD] == 0xA5), "written in front of dst"
    if rc != 0:
        assert np.all(host == 0xA5), "dst touched by a call that failed"
        return rc, None, out_off
    total = int(out_off[-1])
    assert total <= cap and np.all(host[GUARD + total:] == 0xA5), "written behind the output"
    return 0, [host[GUARD + int(out_off[i]):GUARD + int(out_off[i + 1])].tobytes() for i in range(len(datas))], out_off


def check(cs, outs, out_off, gz):
    at = 0
    bad = []
    for i, c in enumerate(cs):
        want = D.model(c, gz)[0]
        if outs[i] != want or int(out_off[i]) != at:
            bad.append((c[0], len(outs[i]), len(want), int(out_off[i]), at))
        at += len(want)
    assert not bad, bad[:10]
    assert int(out_off[len(cs)]) == at


@pytest.mark.parametrize("gz", [False, True], ids=["flate", "gzip"])
def test_all_cases_device(kclib, gz):
    """Every case, one device-resident call per (block, penalty, end) with all its inputs mixed in one batch."""
    for key in sorted(GROUPS):
        cs = GROUPS[key]
        rc, outs, out_off = run_device([c[1] for c in cs], gz, key)
        assert rc == 0
        check(cs, outs, out_off, gz)


def test_all_cases_python_api(kclib):
    """The host-buffer forms through compress_amd.flate.DeflateAll / compress_amd.gzip.GzipAll."""
    from compress_amd import flate, gzip
    for key in sorted(GROUPS):
        block, penalty, end = key
        cs = GROUPS[key]
        src, off = D.pack([c[1] for c in cs])
        kw = dict(flush=end == M.END_FLUSH, block=block, penalty=penalty)
        assert flate.DeflateAll(src, off, flate.HuffmanOnly, **kw) == [D.model(c)[0] for c in cs]
        assert gzip.GzipAll(src, off, gzip.HuffmanOnly, **kw) == [D.model(c, True)[0] for c in cs]


def test_capacity(kclib):
    from compress_amd import _lib
    key = (D.BLOCK, D.PENALTY, M.END_CLOSE)
    cs = [c for c in GROUPS[key] if c[0].startswith(("sweep-", "one-", "multi-reuse"))]
    for gz in (False, True):
        total = sum(len(D.model(c, gz)[0]) for c in cs)
        rc, outs, out_off = run_device([c[1] for c in cs], gz, key, cap=total)
        assert rc == 0
        check(cs, outs, out_off, gz)
        rc, outs, out_off = run_device([c[1] for c in cs], gz, key, cap=total - 1)
        assert rc == _lib.KC_ERR_DST_TOO_SMALL and int(out_off[len(cs)]) == total


def test_device_inflates_what_it_wrote(kclib):
    """The Close-ended cases at compressor.init's own values, written on the device and read by the device's own InflateAll /
    GunzipAll, and by CPython."""
    from compress_amd import flate, gzip
    cs = [c for c in GROUPS[(D.BLOCK, D.PENALTY, M.END_CLOSE)]]
    src, off = D.pack([c[1] for c in cs])
    for mod, write, read in ((flate, flate.DeflateAll, flate.InflateAll), (gzip, gzip.GzipAll, gzip.GunzipAll)):
        outs = write(src, off, mod.HuffmanOnly)
        back = read(np.frombuffer(b"".join(outs), dtype=np.uint8), np.cumsum([0] + [len(o) for o in outs]).astype(np.uint64))
        assert back == [c[1] for c in cs]
    assert all(host_gzip.decompress(o) == c[1] for o, c in zip(outs, cs))


def test_many_short_chains(kclib):
    """One batch of 2 048 inputs of 1 .. 4 096 bytes."""
    from compress_amd import flate
    rng = np.random.default_rng(2048)
    lens = rng.integers(1, 4097, size=2048)
    lens[:8] = (1, 2, 4096, 4095, 1025, 1024, 3, 64)
    body = D.text(int(lens.sum()), 12345)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src = np.frombuffer(body, dtype=np.uint8).copy()
    for k in range(0, 2048, 5):  # every fifth input incompressible
        src[int(off[k]):int(off[k + 1])] = rng.integers(0, 256, size=int(lens[k]), dtype=np.uint8)
    outs = flate.DeflateAll(src, off, flate.HuffmanOnly)
    raw = src.tobytes()
    for k in range(2048):
        assert zlib.decompress(outs[k], -15) == raw[int(off[k]):int(off[k + 1])], k
    for k in range(0, 2048, 97):  # the model on a sample (it is the slow side)
        assert outs[k] == M.deflate(raw[int(off[k]):int(off[k + 1])]), k


def test_many_blocks_in_one_chain(kclib):
    """One input of 8 MiB: 256 blocks in one chain, text with stretches of random bytes and of one byte."""
    from compress_amd import gzip
    rng = np.random.default_rng(8)
    src = np.frombuffer(D.text(8 << 20, 4242), dtype=np.uint8).copy()
    for at in (3 << 15, 40 << 15, 41 << 15, 200 << 15):
        src[at:at + 50000] = rng.integers(0, 256, size=50000, dtype=np.uint8)
    src[100 << 15:(100 << 15) + 100000] = 7
    off = np.array([0, len(src)], dtype=np.uint64)
    out = gzip.GzipAll(src, off, gzip.HuffmanOnly)[0]
    raw = src.tobytes()
    assert host_gzip.decompress(out) == raw
    res = M.deflate_ex(raw)
    assert out[10:-8] == res.data and all(res.counts[k] > 0 for k in ("quick-stored", "first-table", "reuse", "new-table-eob-owed"))


def test_writer_objects(kclib):
    from compress_amd import KcError, flate, gzip
    data = D.text(70001, 99)
    w = io.BytesIO()
    fw = flate.NewWriter(w, flate.HuffmanOnly)
    fw.Write(data[:1000])
    fw.Write(data[1000:])
    with pytest.raises(NotImplementedError):
        fw.Flush()
    fw.Close()
    assert w.getvalue() == M.deflate(data)
    w2 = io.BytesIO()
    fw.Reset(w2)
    fw.Close()
    assert w2.getvalue() == M.deflate(b"")
    w = io.BytesIO()
    gw = gzip.NewWriterLevel(w, gzip.HuffmanOnly)
    gw.Write(data)
    gw.Close()
    assert w.getvalue() == M.gzip_deflate(data)
    for level in (-1, 0, 1, 6, 9):
        with pytest.raises(KcError):
            flate.NewWriter(io.BytesIO(), level)
        with pytest.raises(KcError):
            flate.DeflateAll(np.zeros(1, dtype=np.uint8), np.array([0, 1], dtype=np.uint64), level)
