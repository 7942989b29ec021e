"""The DecodeAll kernels (kc_zstd_plan.hip, kc_zstd_decode_all.hip) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_zstd_decode_all — plan, decode, XXH64, verdict, compaction as one batch) against the reference's decoder fixtures and the
reference's own DecodeAll (translated: oracle_goref.zstd_decode_all)."""
import os
import zipfile

import pytest

from zstd_frame_cases import emu_decode_all as decode_all

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
