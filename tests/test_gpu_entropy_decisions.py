"""The directed entropy-stage inputs (tests/entropy_cases.py) on the device: the frames the HIP entropy stage writes for them
(kc_huf_dev.h's rank sort / depth relaxation / setMaxHeight on LDS, kc_fse_dev.h's normalizeCount / normalizeCount2 / writeCount,
kc_zstd_entropy.hip) are byte-identical to the oracle's, and the device decoder's table builders read the oracle's frames of the
same cases back.  tests/test_entropy_decisions.py (CPU) shows which decisions of the reference each case takes; nothing here reads
the reference or oracle/_ref."""
import functools

import numpy as np
import pytest

import corpora
import entropy_cases as ec
from test_gpu_zstd import LEVELS_B, _li, _lo, _path_ran, _torch

pytestmark = pytest.mark.gpu


def _batches(level):
    """The cases in batches of one option set each: (encoder keywords of the oracle, cases)."""
    groups = {}
    for c in ec.CASES:
        kw = ec.oracle_kw(c, level)
        groups.setdefault((bool(kw.get("all_lit_entropy")), ec.uses_dict(c)), []).append(c)
    return sorted(groups.items())


@functools.lru_cache(maxsize=None)
def _reference(level, ale, with_dict):
    """The oracle's frames of one batch, computed once (levels 1 and "1L" share them) and left unchanged."""
    import oracle_lib
    cases = dict(_batches(level))[ale, with_dict]
    buf, off = corpora.pack_units([ec.unit(c) for c in cases])
    kw = {"level": level}
    if ale:
        kw["all_lit_entropy"] = True
    if with_dict:
        kw.update(dict_id=ec.DICT_ID, dict_content=ec.pool())
    ref, ref_off = oracle_lib.zstd_encode_units(buf, off, threads=8, **kw)
    return cases, buf, off, ref, ref_off


def _options(level, ale, with_dict):
    from compress_amd import zstd
    ops = list(_lo(level))
    if ale:
        ops.append(zstd.WithAllLitEntropyCompression(True))
    if with_dict:
        ops.append(zstd.WithEncoderDictRaw(ec.DICT_ID, ec.pool()))
    return ops


@pytest.mark.parametrize("with_dict", [False, True], ids=["plain", "dict"])
@pytest.mark.parametrize("level", LEVELS_B)
def test_directed_cases_bit_exact(oracle, kclib, level, with_dict):
    """One EncodeUnits batch per level and option set (the dictionary cases in batches of their own): frames and offsets are the
    oracle's."""
    _torch()
    from compress_amd import zstd
    ran = 0
    for (ale, wd), _ in _batches(_li(level)):
        if wd != with_dict:
            continue
        cases, buf, off, ref, ref_off = _reference(_li(level), ale, wd)
        enc = zstd.NewWriter(None, *_options(level, ale, wd))
        out, out_off = enc.EncodeUnits(buf, off)
        _path_ran(enc, level)
        enc.Close()
        bad = []
        for i, c in enumerate(cases):
            a = out[int(out_off[i]):int(out_off[i + 1])].tobytes()
            b = ref[int(ref_off[i]):int(ref_off[i + 1])].tobytes()
            if a != b:
                bad.append((c[0], int(off[i + 1] - off[i]), len(a), len(b)))
        assert not bad, "cases differing from the oracle (name, in_len, gpu_len, oracle_len): %r" % bad
        assert np.array_equal(out_off, ref_off)
        ran += len(cases)
    assert ran >= 10


@pytest.mark.parametrize("with_dict", [False, True], ids=["plain", "dict"])
def test_device_decoder_reads_the_oracles_frames(oracle, kclib, with_dict):
    """The ORACLE's frames of all cases at all four levels through the device DecodeAll: its table builders see the same rare tables
    (a height-limited tree at every table log, raw 4-bit weights with odd counts, FSE tables full of -1 symbols)."""
    _torch()
    from compress_amd import zstd
    from test_gpu_zstd_decode_all import _decode_dev
    frames, want = [], []
    for level in ec.LEVELS:
        for (ale, wd), _ in _batches(level):
            if wd != with_dict:
                continue
            cases, buf, off, ref, ref_off = _reference(level, ale, wd)
            for i in range(len(cases)):
                frames.append(ref[int(ref_off[i]):int(ref_off[i + 1])].tobytes())
                want.append(buf[int(off[i]):int(off[i + 1])].tobytes())
    assert len(frames) >= 40
    dec = zstd.NewReader(None, *([zstd.WithDecoderDictRaw(ec.DICT_ID, ec.pool())] if with_dict else []))
    outs, _, status, guards = _decode_dev(dec, frames)
    dec.Close()
    assert guards
    bad = [(i, int(s)) for i, s in enumerate(status) if s != 0]
    assert not bad, "frames the device decoder refuses (index, status): %r" % bad[:10]
    assert outs == want
