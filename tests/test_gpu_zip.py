"""zip members on the device (kc_zip_read*, compress_amd.zip): the reference's fixtures, the hand-built cases with the full stored
sweep, and the 480 mutations of tests/zip_cases.py — each set as ONE device-resident batch over the merged buffers with 64 guard
bytes of 0xA5 on both sides of dst, and case by case through the host-buffer form, where every buffer ends where its case says —
judged by tests/zip_model.py (tests/test_zip_model.py pins it): bytes, status and layout.  Then the Python objects, and an archive
of 2048 members deflated by CPython at levels 1, 6 and 9, for which no device writer exists."""
import ctypes as C
import io
import zlib as host_zlib

import numpy as np
import pytest

import zip_cases as ZC
import zip_model as Z
from test_emu_zip import table

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from compress_amd import _lib
    c = _lib.Context(0, None)
    yield c
    c.close()


def read_device(ctx, data, members, cap=None):
    """kc_zip_read_dev -> (return code, out_off, status, dst with its guards)"""
    import torch
    n = len(members)
    src = np.frombuffer(data + b"\0", dtype=np.uint8).copy()
    d_src = torch.from_numpy(src).cuda(0)
    t = table(members)
    oo, st = np.zeros(n + 1, np.uint64), np.full(max(n, 1), 0xEE, np.uint32)
    if cap is None:
        ctx.check(ctx.L.kc_zip_read_bound(ctx.h, src.ctypes.data, len(data), C.addressof(t), n, oo.ctypes.data, st.ctypes.data))
        cap = int(oo[-1])
    d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    rc = ctx.L.kc_zip_read_dev(ctx.h, d_src.data_ptr(), len(data), C.addressof(t), n, d_all.data_ptr() + GUARD, cap, oo.ctypes.data, st.ctypes.data)
    torch.cuda.synchronize()
    host = d_all.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + cap:] == 0xA5), "written outside dst"
    return rc, oo, st[:n], host


def read_host(ctx, data, members):
    """kc_zip_read_bound, then kc_zip_read into exactly that -> per member (bytes, status), total"""
    n = len(members)
    src = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, dtype=np.uint8)
    t = table(members)
    oo0, st0 = np.zeros(n + 1, np.uint64), np.full(max(n, 1), 0xEE, np.uint32)
    ctx.check(ctx.L.kc_zip_read_bound(ctx.h, src.ctypes.data, len(data), C.addressof(t), n, oo0.ctypes.data, st0.ctypes.data))
    cap = int(oo0[-1])
    dst = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    oo, st = np.zeros(n + 1, np.uint64), np.full(max(n, 1), 0xEE, np.uint32)
    ctx.check(ctx.L.kc_zip_read(ctx.h, src.ctypes.data, len(data), C.addressof(t), n, dst.ctypes.data + GUARD, cap, oo.ctypes.data, st.ctypes.data))
    assert np.all(dst[:GUARD] == 0xA5) and np.all(dst[GUARD + cap:] == 0xA5) and np.array_equal(oo, oo0)
    return [(dst[GUARD + int(oo[i]):GUARD + int(oo[i + 1])].tobytes(), int(st[i])) for i in range(n)], cap


def check_set(ctx, cases):
    # one device-resident batch over the merged buffers
    data, members = ZC.merged(cases)
    want, total = Z.read_all(data, members)
    rc, oo, st, host = read_device(ctx, data, members)
    assert rc == 0 and int(oo[-1]) == total
    got = [(host[GUARD + int(oo[i]):GUARD + int(oo[i + 1])].tobytes(), int(st[i])) for i in range(len(members))]
    bad = [(i, Z.NAMES.get(g[1], g[1]), len(g[0]), Z.NAMES[w[1]], len(w[0])) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:10])
    # case by case through the host-buffer form: every buffer ends where its case says
    bad = []
    for c in cases:
        ms = ZC.members_of(c)
        w, total = Z.read_all(c.data, ms)
        g, cap = read_host(ctx, c.data, ms)
        if g != w or cap != total:
            bad.append((c.name, cap, total, [(Z.NAMES.get(x[1], x[1]), len(x[0])) for x in g][:4], [(Z.NAMES[x[1]], len(x[0])) for x in w][:4]))
    assert not bad, (len(bad), bad[:10])


def test_reference_fixtures(ctx):
    check_set(ctx, ZC.fixture_cases())


def test_directed_cases_and_stored_sweep(ctx):
    check_set(ctx, ZC.directed() + [ZC.stored_cases(True)])


def test_mutations(ctx):
    cs = ZC.mutations()
    assert len(cs) == 480
    check_set(ctx, cs)


def test_dst_too_small_writes_nothing(ctx):
    c = {c.name: c for c in ZC.directed()}["merged/two-archives"]
    ms = ZC.members_of(c)
    rc, oo, _, host = read_device(ctx, c.data, ms, cap=699)
    assert rc == -2 and np.all(host == 0xA5) and [int(x) for x in oo] == [0, 300, 400, 700, 700]
    rc, oo, st, host = read_device(ctx, c.data, ms, cap=700)
    assert rc == 0 and [int(s) for s in st] == [0, 0, 0, 0]


def test_python_objects():
    from compress_amd import zip as kzip
    data = open(ZC.GOLDEN + "/test.zip", "rb").read()
    png = open(ZC.GOLDEN + "/gophercolor16x16.png", "rb").read()
    for r in (kzip.NewReader(data), kzip.NewReader(io.BytesIO(data)), kzip.NewReader(np.frombuffer(data, dtype=np.uint8)), kzip.OpenReader(ZC.GOLDEN + "/test.zip")):
        assert r.Comment == "This is a zipfile comment." and [f.Name for f in r.File] == ["test.txt", "gophercolor16x16.png"]
        f0, f1 = r.File
        assert (f0.Method, f0.UncompressedSize64, f1.Method, f1.CRC32) == (kzip.Deflate, 26, kzip.Store, host_zlib.crc32(png))
        rc = f0.Open()
        p = bytearray(10)
        got = b""
        while True:
            n = rc.Read(p)
            if n == 0:
                break
            got += bytes(p[:n])
        rc.Close()
        assert got == b"This is a test text file.\n"
        w = io.BytesIO()
        assert f1.Open().WriteTo(w) == 785 and w.getvalue() == png
        at = f1.DataOffset()
        assert data[at:at + 785] == png and f1.OpenRaw().read() == png
        assert host_zlib.decompress(f0.OpenRaw().read(), -15) == got
        assert r.ReadAll() == [got, png] and r.ReadAll([f1]) == [png] and r.ReadAll([]) == []
        r.Close()
    bad = {c.name: c for c in ZC.directed()}
    r = kzip.NewReader(bad["crc/wrong"].data)
    with pytest.raises(kzip.ErrChecksum, match="zip: checksum error"):
        r.File[0].Open().Read(bytearray(4))
    res = kzip.NewReader(bad["method/93"].data).ReadAll() + kzip.NewReader(bad["size/deflated-one-too-small"].data).ReadAll() + \
        kzip.NewReader(bad["csize/one-short"].data).ReadAll() + kzip.NewReader(bad["bomb/corrupt"].data).ReadAll()
    assert [type(x) for x in res] == [kzip.ErrAlgorithm, kzip.ErrFormat, kzip.ErrUnexpectedEOF, kzip.CorruptInputError]
    assert str(res[0]) == "zip: unsupported compression algorithm" and str(res[1]) == "zip: not a valid zip file"
    with pytest.raises(kzip.ErrFormat):
        kzip.NewReader(bad["end/none"].data)


def test_read_all_device_2048_members_of_cpython_levels():
    import torch
    from compress_amd import zip as kzip
    data, contents = ZC.many_small()
    r = kzip.NewReader(data)
    assert len(r.File) == 2048
    total = sum(len(t) for t in contents)
    d_src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda(0)
    d_dst = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    oo, st = r.ReadAllDevice(d_src.data_ptr(), d_dst.data_ptr() + GUARD, total)
    host = d_dst.cpu().numpy()
    assert not st.any() and int(oo[-1]) == total and host[GUARD:GUARD + total].tobytes() == b"".join(contents)
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + total:] == 0xA5)
    assert r.ReadAll(r.File[5:8]) == contents[5:8]
    r.Close()
