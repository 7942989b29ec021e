"""The hand-built frames of tests/zstd_frame_cases.py through zstd.Decoder on the device: DecodeAllDevice (device-resident, dst sized by
DecodeBoundsDevice, guard bytes on both sides) and DecodeUnits (host buffers), judged by the reference's own DecodeAll (translated:
oracle_goref.zstd_decode_all) — its bytes with status 0, or a status and an empty range; for the directed refusals the status class
is the class of the reference's message.  The valid single frames also go through the verifier (kc_zstd_decode_units_dev /
_dict_dev), which shares kc_zdec_dev.h with the product path."""
import numpy as np
import pytest

import corpora
import zstd_frame_cases as zc

pytestmark = pytest.mark.gpu

GUARD = 64
SECTIONS = ("header", "blocks", "literals", "sequences", "offsets", "group")


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own DecodeAll, translated) is the judge of these tests"
    return oracle_goref


@pytest.fixture(scope="module")
def dec(kclib):
    from compress_amd import zstd
    d = zstd.NewReader(None, *[zstd.WithDecoderDictRaw(i, c) for i, c in zc.DICTS.items()])
    yield d
    d.Close()


def _decode_dev(dec, inputs):
    """One device-resident batch: inputs on the device, dst sized by the plan (DecodeBoundsDevice), GUARD bytes of 0xA5 in front of and
    behind dst.  Returns (list of bytes per input, out_off, status, guards intact)."""
    import torch
    buf, off = corpora.pack_units([bytes(x) for x in inputs])
    d_src = torch.from_numpy(buf).cuda(0)
    bound, st0 = dec.DecodeBoundsDevice(d_src.data_ptr(), off)
    cap = int(sum(int(b) for b, s in zip(bound, st0) if s == 0))
    d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out_off, status = dec.DecodeAllDevice(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap)
    host = d_all.cpu().numpy()
    guards = bool(np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + cap:] == 0xA5))
    body = host[GUARD:GUARD + cap]
    assert out_off[0] == 0 and int(out_off[-1]) <= cap and np.all(np.diff(out_off.astype(np.int64)) >= 0)
    return [body[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(len(inputs))], out_off, status, guards


@pytest.mark.parametrize("section", SECTIONS)
def test_device_judged_by_the_reference(kclib, G, dec, section):
    cs = [c for c in zc.cases() if c.section == section]
    assert cs
    refs = [zc.reference(G, c) for c in cs]
    inputs = [c.data for c in cs]
    outs, out_off, status, guards = _decode_dev(dec, inputs)
    assert guards, "written outside dst"
    wrong = zc.judge(cs, refs, outs, status)
    assert not wrong, "\n".join(wrong)
    # the host entry point gives the same
    buf, off = corpora.pack_units(inputs)
    hout, hoff, hstatus = dec.DecodeUnits(buf, off)
    assert np.array_equal(hoff, out_off) and np.array_equal(hstatus, status) and hout.tobytes() == b"".join(outs)
    # the directed refusals: the class of the status is the class of the reference's message
    for c, (_, err), s in zip(cs, refs, status):
        if c.cls is not None:
            assert zc.NAMES[int(s)] == c.cls == zc.message_class(err), (c.name, zc.NAMES[int(s)], err)


def test_directed_refusals_name_every_class():
    """WINDOW_EXCEEDED, SIZE_EXCEEDED, CRC, UNKNOWN_DICT and EOF have a hand-built case each, whose class the test above compares."""
    assert {c.cls for c in zc.cases() if c.cls} == {"WINDOW_EXCEEDED", "SIZE_EXCEEDED", "CRC", "UNKNOWN_DICT", "EOF"}


def test_verifier_on_the_valid_frames(kclib):
    """Every valid single-frame case through the verifier, with the builder's sizes: status 0 and the builder's bytes."""
    import torch
    from compress_amd import zstd
    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(1))
    seen = 0
    for did in (None,) + tuple(zc.DICTS):
        cs = [c for c in zc.cases() if c.expect == "valid" and not c.name.startswith("two frames") and c.dicts == (() if did is None else (did,))]
        assert cs
        seen += len(cs)
        buf, eoff = corpora.pack_units([c.data for c in cs])
        plain = b"".join(c.plain for c in cs)
        doff = np.zeros(len(cs) + 1, dtype=np.uint64)
        doff[1:] = np.cumsum([len(c.plain) for c in cs])
        d_enc = torch.from_numpy(buf).cuda(0)
        d_out = torch.full((len(plain) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        st = enc.DecodeUnitsDevice(d_enc.data_ptr(), eoff, d_out.data_ptr() + GUARD, doff, dict_content=None if did is None else zc.DICTS[did])
        bad = [(c.name, int(s)) for c, s in zip(cs, st) if s]
        assert not bad, bad
        host = d_out.cpu().numpy()
        assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + len(plain):] == 0xA5), "written outside dst"
        got = host[GUARD:GUARD + len(plain)].tobytes()
        for i, c in enumerate(cs):
            assert got[int(doff[i]):int(doff[i + 1])] == c.plain, c.name
    enc.Close()
    assert seen >= 100
