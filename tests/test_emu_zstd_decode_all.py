"""The DecodeAll kernels (kc_zstd_plan.hip, kc_zstd_decode_all.hip) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_zstd_decode_all — plan, decode, XXH64, verdict, compaction as one batch) against the reference's decoder fixtures and the
reference's own DecodeAll (translated: oracle_goref.zstd_decode_all)."""
import ctypes as C
import os
import zipfile

import numpy as np
import pytest

import emu_lib

HERE = os.path.dirname(os.path.abspath(__file__))
REFIN = os.path.join(HERE, "golden", "ref_inputs")
NAMES = {0: "OK", 1: "MAGIC", 2: "EOF", 3: "UNKNOWN_DICT", 4: "WINDOW_EXCEEDED", 5: "SIZE_EXCEEDED", 6: "CRC", 7: "CORRUPT"}


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference decoder) is not built")
    return oracle_goref


def _members(name, suffix=None):
    z = zipfile.ZipFile(os.path.join(REFIN, name))
    return [(m, z.read(m)) for m in z.namelist() if not m.endswith("/") and (suffix is None or m.endswith(suffix))]


def decode_all(inputs, cap, dicts=(), max_memory=64 << 30, max_window=1 << 29, ignore_checksum=False):
    """(list of bytes, status[n]) of kcemu_zstd_decode_all; GUARD bytes around dst are checked."""
    L = emu_lib.lib()
    L.kcemu_zstd_decode_all.restype = C.c_int
    L.kcemu_zstd_decode_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    n = len(inputs)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs])
    src = np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy()
    doff = np.zeros(len(dicts) + 1, dtype=np.uint64)
    doff[1:] = np.cumsum([len(d) for d in dicts])
    dblob = np.frombuffer(b"".join(dicts) + b"\0", dtype=np.uint8).copy()
    guard = 64
    dst = np.full(cap + 2 * guard, 0xA5, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    r = L.kcemu_zstd_decode_all(src.ctypes.data, off.ctypes.data, n, max_memory, max_window, int(ignore_checksum), dblob.ctypes.data, doff.ctypes.data,
                                len(dicts), dst.ctypes.data + guard, cap, out_off.ctypes.data, status.ctypes.data)
    assert r == 0, r
    assert np.all(dst[:guard] == 0xA5) and np.all(dst[guard + cap:] == 0xA5), "written outside dst"
    body = dst[guard:guard + cap]
    return [body[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)], status


def test_good_frames(G):
    """good.zip + z000028.zst: the plaintexts of the archive and the reference decoder's output (several frames per input and
    skippable frames included)."""
    good = _members("good.zip", ".zst")
    plain = dict(_members("good.zip"))
    frames = [d for _, d in good] + [open(os.path.join(REFIN, "z000028.zst"), "rb").read()]
    want = [G.zstd_decode_all(z, 1 << 20) for z in frames]
    outs, status = decode_all(frames, sum(len(w) for w in want))
    assert [NAMES[int(s)] for s in status] == ["OK"] * len(frames)
    assert outs == want
    assert outs[-1] == open(os.path.join(REFIN, "z000028"), "rb").read()
    n = 0
    for (m, _), o in zip(good, outs):
        if m[:-4] in plain:
            assert o == plain[m[:-4]], m
            n += 1
    assert n >= 10


def test_dictionary_frames(G):
    """The 41 frames of dict-tests-small.zip with all three dictionaries registered at once."""
    ms = _members("dict-tests-small.zip")
    dicts = {int.from_bytes(d[4:8], "little"): d for m, d in ms if m.endswith(".dict")}
    frames = [(m, d) for m, d in ms if m.endswith(".zst")]
    assert len(dicts) == 3 and len(frames) == 41
    want = []
    for m, z in frames:
        fhd = z[4]
        p = 5 + (0 if (fhd >> 5) & 1 else 1)
        want.append(G.zstd_decode_all(z, 1 << 20, dict_blob=dicts[int.from_bytes(z[p:p + [0, 1, 2, 4][fhd & 3]], "little")]))
    outs, status = decode_all([z for _, z in frames], sum(len(w) for w in want), dicts=list(dicts.values()))
    assert [NAMES[int(s)] for s in status] == ["OK"] * 41
    assert outs == want
    outs, status = decode_all([z for _, z in frames], 64)
    assert [NAMES[int(s)] for s in status] == ["UNKNOWN_DICT"] * 41 and outs == [b""] * 41


def test_bad_frames_are_refused(G):
    """bad.zip: all 44 members get a status (the reference refuses all of them) and leave nothing in dst."""
    bad = _members("bad.zip")
    assert len(bad) == 44
    for _, z in bad:
        with pytest.raises(ValueError):
            G.zstd_decode_all(z, 1 << 20)
    outs, status = decode_all([z for _, z in bad], 1 << 16)
    assert all(int(s) != 0 for s in status), [NAMES[int(s)] for s in status]
    assert outs == [b""] * 44
