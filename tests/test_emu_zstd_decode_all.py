"""The DecodeAll kernels (kc_zstd_plan.hip, kc_zstd_decode_all.hip) on the CPU wave emulator (tools/hipemu/kcemu.cpp:
kcemu_zstd_decode_all — plan, decode, XXH64, verdict, compaction as one batch) against the reference's decoder fixtures and the
reference's own DecodeAll (translated: oracle_goref.zstd_decode_all)."""
import os
import zipfile

import pytest

import emu_lib
import zstd_frame_cases as zc
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


def test_budget_cuts_change_nothing_and_refuse_what_cannot_fit(G):
    """The hand-built frames (tests/zstd_frame_cases.py) as one device batch, then under the least scratch budget that refuses no input
    — the largest input's staging and per-frame scratch plus the 1/8 allowance, as the sequence reports it: at least three batches,
    the same bytes, layout and statuses.  One byte less: exactly that input is KC_ZD_SIZE_EXCEEDED with an empty range, every other
    input as before."""
    cs = [c for c in zc.cases() if not c.big]
    inputs = [c.data for c in cs]
    dicts = [zc.raw_dict_blob(i, d) for i, d in zc.DICTS.items()]
    refs = [zc.reference(G, c) for c in cs]
    cap = sum(len(r) for r, _ in refs if r is not None)
    outs, status = decode_all(inputs, cap, dicts=dicts)
    assert emu_lib.last_batches() == 1 and not zc.judge(cs, refs, outs, status)
    need = emu_lib.last_max_need()
    k = max(range(len(cs)), key=lambda i: len(outs[i]))  # the input that needs it: the one with the most decoded bytes
    decode_all([inputs[k]], cap, dicts=dicts)
    assert emu_lib.last_max_need() == need and 0 < need < (16 << 20) and int(status[k]) == 0
    with emu_lib.scratch_budget(need):
        outs2, status2 = decode_all(inputs, cap, dicts=dicts)
        assert emu_lib.last_batches() >= 3, emu_lib.last_batches()
    assert outs2 == outs and list(status2) == list(status)
    with emu_lib.scratch_budget(need - 1):
        outs3, status3 = decode_all(inputs, cap, dicts=dicts)
        assert emu_lib.last_batches() >= 3
    assert NAMES[int(status3[k])] == "SIZE_EXCEEDED" and outs3[k] == b""
    assert [o for i, o in enumerate(outs3) if i != k] == [o for i, o in enumerate(outs) if i != k]
    assert [int(s) for i, s in enumerate(status3) if i != k] == [int(s) for i, s in enumerate(status) if i != k]
