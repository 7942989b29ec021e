"""The verifier (kc_zstd_decode.hip behind kc_zstd_decode_units_dev / _dict_dev: one frame per unit, every frame's decoded length
given) on the CPU wave emulator (tools/hipemu/kcemu.cpp: kcemu_zstd_decode_units — decode kernel, XXH64, checksum verdict), judged by
the builder's plaintexts and by the reference's own DecodeAll (translated: oracle_goref.zstd_decode_all)."""
import ctypes as C

import numpy as np
import pytest

import zstd_dstream_cases as K
import zstd_frame_cases as zc

GUARD = 64


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference decoder) is not built")
    return oracle_goref


def decode_units(frames, sizes, dict_content=b""):
    """(status per frame, bytes per frame) of kcemu_zstd_decode_units: frame i decodes into a range of sizes[i] bytes; the GUARD bytes
    around dst are checked.  dict_content: a raw dictionary's content in front of every frame."""
    import emu_lib
    L = emu_lib.lib()
    L.kcemu_zstd_decode_units.restype = C.c_int
    L.kcemu_zstd_decode_units.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    n = len(frames)
    eoff = np.zeros(n + 1, dtype=np.uint64)
    eoff[1:] = np.cumsum([len(f) for f in frames])
    enc = np.frombuffer(b"".join(frames) + b"\0", dtype=np.uint8).copy()
    doff = np.zeros(n + 1, dtype=np.uint64)
    doff[1:] = np.cumsum(sizes)
    total = int(doff[n])
    dst = np.full(total + 2 * GUARD, 0xA5, dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint32)
    d = np.frombuffer(dict_content + b"\0", dtype=np.uint8).copy()
    r = L.kcemu_zstd_decode_units(enc.ctypes.data, eoff.ctypes.data, n, dst.ctypes.data + GUARD, doff.ctypes.data, d.ctypes.data, len(dict_content),
                                  status.ctypes.data)
    assert r == 0, r
    assert np.all(dst[:GUARD] == 0xA5) and np.all(dst[GUARD + total:] == 0xA5), "written outside dst"
    body = dst[GUARD:GUARD + total]
    return [int(s) for s in status], [body[int(doff[i]):int(doff[i + 1])].tobytes() for i in range(n)]


def test_verifier_on_the_valid_frames():
    """Every valid single-frame case through the verifier, with the builder's sizes and the raw dictionaries: status 0 and the
    builder's bytes (the emulator twin of test_gpu_zstd_decode_shapes.py::test_verifier_on_the_valid_frames)."""
    seen = 0
    for did in (None,) + tuple(zc.DICTS):
        cs = [c for c in zc.cases() if c.expect == "valid" and not c.name.startswith("two frames") and c.dicts == (() if did is None else (did,))]
        assert cs
        seen += len(cs)
        status, outs = decode_units([c.data for c in cs], [len(c.plain) for c in cs], b"" if did is None else zc.DICTS[did])
        bad = [(c.name, s) for c, s in zip(cs, status) if s]
        assert not bad, bad
        for c, o in zip(cs, outs):
            assert o == c.plain, c.name
    assert seen >= 100


def test_bad_frames_are_refused():
    """bad.zip: all 44 members get a status, given the length their header promises (4096 where it promises none)."""
    bad = K.members("bad.zip")
    assert len(bad) == 44
    sizes = []
    for _, z in bad:
        h = K.first_header(z)
        sizes.append(h[2] if h is not None and h[2] is not None and h[2] <= 1 << 20 else 4096)
    status, _ = decode_units([z for _, z in bad], sizes)
    assert all(status), [m for (m, _), s in zip(bad, status) if not s]


def test_differential_on_mutations(G):
    """The 480 seeded mutations, each given the reference's decoded length where the reference decodes it and the unmutated frame's
    length where it does not: status 0 implies the reference decodes exactly those bytes, and the reference decoding (the checksum,
    where one is stored, matching) implies status 0."""
    cases = K.mutation_cases(G)
    original = [n for n in (1, 300, 5000, 70000, 140000) for _ in range(6 * 16)]  # (the frames of mutation_cases, in its order)
    assert len(original) == len(cases) == 480
    refs = [K.ref(G, z)[0] for z in cases]
    status, outs = decode_units(cases, [len(r) if r is not None else n for r, n in zip(refs, original)])
    wrong = []
    for i, (r, s, o) in enumerate(zip(refs, status, outs)):
        if s == 0 and (r is None or o != r):
            wrong.append("mutation %d: status 0 with %d bytes, the reference %s" % (i, len(o), "refuses" if r is None else "returns others"))
        if r is not None and s != 0:
            wrong.append("mutation %d: the reference returns %d bytes, status %d" % (i, len(r), s))
    assert not wrong, "\n".join(wrong)
    assert 0 < sum(r is not None for r in refs) < len(cases)
