"""zstd.Decoder.DecodeAll on the device as a product (kc_zstd_decode_all[_dev], compress_amd.zstd.Decoder): batches of independent
inputs, no decoded size supplied, judged by the reference's own DecodeAll (translated: oracle_goref.zstd_decode_all) on the
reference's decoder fixtures (tests/golden/ref_inputs/), on frames of the oracle and of the device encoder, and on seeded mutations."""
import os
import random
import zipfile

import numpy as np
import pytest

import corpora

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REFIN = os.path.join(HERE, "golden", "ref_inputs")
GUARD = 64
KC_ERR_DST_TOO_SMALL = -2


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    assert oracle_goref.available(), "oracle/_ref/libzstdref.so (the reference's own DecodeAll, translated) is the judge of these tests"
    return oracle_goref


def _members(name, suffix=None):
    z = zipfile.ZipFile(os.path.join(REFIN, name))
    return [(m, z.read(m)) for m in z.namelist() if not m.endswith("/") and (suffix is None or m.endswith(suffix))]


def _twain():
    return open(os.path.join(REFIN, "Mark.Twain-Tom.Sawyer.txt"), "rb").read()


_ref_cache = {}


def _ref(G, z, cap=8 << 20, **kw):
    """The reference's DecodeAll: (bytes, None) or (None, error text).  Computed once per input and left unchanged."""
    key = (bytes(z), cap, tuple(sorted((k, bytes(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in kw.items())))
    if key not in _ref_cache:
        try:
            _ref_cache[key] = (G.zstd_decode_all(z, cap, **kw), None)
        except ValueError as e:
            _ref_cache[key] = (None, str(e))
    return _ref_cache[key]


def _decode_dev(dec, inputs, cap=None):
    """One device-resident batch: inputs on the device, dst sized by the plan (DecodeBoundsDevice) unless `cap` is given, GUARD bytes of
    0xA5 in front of and behind dst.  Returns (list of bytes per input, out_off, status, guards intact)."""
    import torch
    buf, off = corpora.pack_units([bytes(x) for x in inputs])
    d_src = torch.from_numpy(buf if len(buf) else np.zeros(1, dtype=np.uint8)).cuda(0)
    if cap is None:
        bound, st0 = dec.DecodeBoundsDevice(d_src.data_ptr(), off)
        cap = int(sum(int(b) for b, s in zip(bound, st0) if s == 0))
    d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out_off, status = dec.DecodeAllDevice(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap)
    host = d_all.cpu().numpy()
    guards = bool(np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + cap:] == 0xA5))
    body = host[GUARD:GUARD + cap]
    assert out_off[0] == 0 and int(out_off[-1]) <= cap and np.all(np.diff(out_off.astype(np.int64)) >= 0)
    return [body[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(len(inputs))], out_off, status, guards


def _fixture_batch():
    good = _members("good.zip", ".zst")
    assert len(good) == 12
    bench = _members("benchdecoder.zip")
    assert len(bench) == 12
    return [d for _, d in good] + [open(os.path.join(REFIN, "z000028.zst"), "rb").read()] + [d for _, d in bench]


def _name(status):
    from compress_amd import _lib
    return _lib.ZD_NAMES[int(status)]


def test_fixtures_one_batch(kclib, G):
    """good.zip (12), z000028.zst and benchdecoder.zip (12) in one batch, no decoded size supplied: out_off and bytes are the reference's."""
    from compress_amd import zstd
    frames = _fixture_batch()
    dec = zstd.NewReader(None)
    outs, out_off, status, guards = _decode_dev(dec, frames)
    dec.Close()
    want = [_ref(G, z)[0] for z in frames]
    assert all(w is not None for w in want)
    assert [int(s) for s in status] == [0] * len(frames)
    assert [len(o) for o in outs] == [len(w) for w in want]
    assert outs == want and guards
    assert int(out_off[-1]) == sum(len(w) for w in want)
    # the plaintexts beside the frames in good.zip
    plain = dict(_members("good.zip"))
    for (m, _), o in zip(_members("good.zip", ".zst"), outs):
        if m[:-4] in plain:
            assert o == plain[m[:-4]], m


def test_refusals_between_good_neighbours(kclib, G):
    """The 44 members of bad.zip interleaved with the good.zip frames: every bad one gets a status and an empty range, every good
    neighbour its bytes; nothing is written outside the output."""
    from compress_amd import zstd
    bad = _members("bad.zip")
    good = [d for _, d in _members("good.zip", ".zst")]
    assert len(bad) == 44
    inputs, is_bad = [], []
    for i, (_, d) in enumerate(bad):
        inputs.append(d); is_bad.append(True)
        inputs.append(good[i % len(good)]); is_bad.append(False)
    dec = zstd.NewReader(None)
    outs, out_off, status, guards = _decode_dev(dec, inputs)
    dec.Close()
    assert guards
    for i, z in enumerate(inputs):
        ref, err = _ref(G, z)
        if is_bad[i]:
            assert err is not None, "the reference refuses every member of bad.zip"
            assert status[i] != 0 and outs[i] == b"", (i, _name(status[i]), err)
        else:
            assert status[i] == 0 and outs[i] == ref, (i, _name(status[i]))


def _dict_frames():
    ms = _members("dict-tests-small.zip")
    dicts = {int.from_bytes(d[4:8], "little"): d for m, d in ms if m.endswith(".dict")}
    frames = [(m, d) for m, d in ms if m.endswith(".zst")]
    assert len(dicts) == 3 and len(frames) == 41
    return dicts, frames


def _frame_dict_id(z):
    fhd = z[4]
    p = 5 + (0 if (fhd >> 5) & 1 else 1)
    return int.from_bytes(z[p:p + [0, 1, 2, 4][fhd & 3]], "little")


def test_dictionaries_chosen_by_id(kclib, G):
    """dict-tests-small.zip: 41 frames, the three dictionaries registered at once and chosen by the frame's id (24 of the frames need
    the dictionary's entropy tables or repeat offsets); without a dictionary all 41 report KC_ZD_UNKNOWN_DICT, as the reference does."""
    from compress_amd import zstd, _lib
    dicts, frames = _dict_frames()
    dec = zstd.NewReader(None, zstd.WithDecoderDicts(*dicts.values()))
    outs, _, status, guards = _decode_dev(dec, [d for _, d in frames])
    dec.Close()
    assert guards
    for (m, z), o, s in zip(frames, outs, status):
        ref, err = _ref(G, z, 1 << 20, dict_blob=dicts[_frame_dict_id(z)])
        assert err is None and s == 0 and o == ref, (m, _name(s), err)
    dec = zstd.NewReader(None)
    outs, _, status, _ = _decode_dev(dec, [d for _, d in frames])
    dec.Close()
    for (m, z), o, s in zip(frames, outs, status):
        assert "unknown dictionary" in _ref(G, z, 1 << 20)[1]
        assert _lib.ZD_NAMES[int(s)] == "KC_ZD_UNKNOWN_DICT" and o == b"", m


@pytest.mark.parametrize("level", [1, 2, 3])
def test_device_encoder_dictionary_frames_decode_back(kclib, level):
    """Frames the device encoder wrote with tests/golden/dict/d0.dict (full format) and with a raw dictionary decode back to their sources."""
    from compress_amd import zstd
    blob = open(os.path.join(HERE, "golden", "dict", "d0.dict"), "rb").read()
    tw = _twain()
    units = [tw[20000:20000 + n] for n in (0, 1, 700, 9000, 70000)] + [blob[5000:9000] + tw[:3000]]
    buf, off = corpora.pack_units(units)
    raw = tw[100000:130000]
    for eopt, dopt in ((zstd.WithEncoderDict(blob), zstd.WithDecoderDicts(blob)), (zstd.WithEncoderDictRaw(77, raw), zstd.WithDecoderDictRaw(77, raw))):
        enc = zstd.NewWriter(None, zstd.WithEncoderLevel(level), eopt)
        frames, foff = enc.EncodeUnits(buf, off)
        enc.Close()
        dec = zstd.NewReader(None, dopt)
        outs, _, status, guards = _decode_dev(dec, [frames[int(foff[i]):int(foff[i + 1])].tobytes() for i in range(len(units))])
        dec.Close()
        assert guards and [int(s) for s in status] == [0] * len(units) and outs == units


def test_unknown_sizes_and_several_frames_per_input(kclib, G):
    """Stream frames of the oracle (no content size) at levels 1-3; one input made of frame + skippable frame + stream frame + empty
    frame + skippable frame; the padded output of zstd.pad_frames; stray bytes behind the input (KC_ZD_MAGIC) and an input cut
    short (KC_ZD_EOF), with the reference's own verdicts checked beside them."""
    from compress_amd import zstd
    tw = _twain()
    inputs, want = [], []
    for level in (1, 2, 3):
        for n in (0, 1, 1000, 65536, 131072, 300000):
            src = tw[3000:3000 + n]
            inputs.append(G.zstd_encode_stream(src, level=level))
            want.append(src)
    a, b = tw[:5000], tw[50000:50000 + 200000]
    skip = lambda k: zstd.skippable_frame(8 + k, rand=lambda m: bytes(range(m)))
    composite = G.zstd_encode_all(a, level=1) + skip(17) + G.zstd_encode_stream(b, level=2) + G.zstd_encode_all(b"", level=1) + skip(0)
    assert _ref(G, composite) == (a + b, None)
    inputs.append(composite); want.append(a + b)
    fr, foff = corpora.pack_units([G.zstd_encode_all(tw[k * 1000:k * 1000 + 777 * k], level=1) for k in range(4)])
    padded, poff = zstd.pad_frames(fr, foff, 64, rand=lambda m: b"\x5a" * m)
    for i in range(4):
        inputs.append(padded[int(poff[i]):int(poff[i + 1])].tobytes()); want.append(tw[i * 1000:i * 1000 + 777 * i])
    n_ok = len(inputs)
    inputs.append(composite + b"\x01\x02\x03\x04\x05")
    assert "magic number mismatch" in _ref(G, inputs[-1])[1]
    inputs.append(composite[:-2])
    assert "unexpected EOF" in _ref(G, inputs[-1])[1]
    dec = zstd.NewReader(None)
    outs, _, status, guards = _decode_dev(dec, inputs)
    dec.Close()
    assert guards
    assert [int(s) for s in status[:n_ok]] == [0] * n_ok and outs[:n_ok] == want
    assert (_name(status[n_ok]), _name(status[n_ok + 1])) == ("KC_ZD_MAGIC", "KC_ZD_EOF") and outs[n_ok:] == [b"", b""]


def test_differential_on_mutations(kclib, G):
    """30 frames (Tom Sawyer at five lengths, levels 1-3, EncodeAll and stream form, no checksum), 16 seeded mutations each — a bit
    flip, a truncation or a byte overwrite: where the reference returns bytes (at most 1 MiB) the device returns the same bytes,
    where it refuses (or returns more) the device reports a status.  No case is left out."""
    from compress_amd import zstd
    tw = _twain()
    frames = []
    for n in (1, 300, 5000, 70000, 140000):
        src = tw[1000:1000 + n]
        for level in (1, 2, 3):
            frames.append(G.zstd_encode_all(src, level=level, crc=False))
            frames.append(G.zstd_encode_stream(src, level=level, crc=False))
    assert len(frames) == 30
    rng = random.Random(0x5EED0001)
    cases = []
    for f in frames:
        for _ in range(16):
            kind = rng.randrange(3)
            m = bytearray(f)
            if kind == 0:
                p = rng.randrange(len(m) * 8)
                m[p >> 3] ^= 1 << (p & 7)
            elif kind == 1:
                m = m[:rng.randrange(len(m))]
            else:
                m[rng.randrange(len(m))] = rng.randrange(256)
            cases.append(bytes(m))
    assert len(cases) == 480
    cap = 1 << 20
    refs = [_ref(G, c, cap) for c in cases]
    accepted = sum(1 for r, _ in refs if r is not None)
    changed = sum(1 for i, (r, _) in enumerate(refs) if r is not None and r != _ref(G, frames[i // 16], cap)[0])
    print("reference: %d accepted (%d of them with other bytes than the original), %d refused" % (accepted, changed, len(cases) - accepted))
    assert accepted * 5 >= len(cases) and (len(cases) - accepted) * 5 >= len(cases)  # the reference's side alone: neither verdict is rare
    dec = zstd.NewReader(None, zstd.WithDecoderMaxMemory(cap))
    outs, _, status, guards = _decode_dev(dec, cases)
    dec.Close()
    assert guards
    wrong = []
    for i, ((ref, err), o, s) in enumerate(zip(refs, outs, status)):
        if ref is not None:
            if s != 0 or o != ref:
                wrong.append((i, "reference returns %d bytes" % len(ref), _name(s), len(o)))
        elif s == 0:
            wrong.append((i, err, "KC_ZD_OK", len(o)))
    assert not wrong, wrong[:10]


def test_limits_and_classes(kclib, G):
    """One directed case per class, beside the reference's own error text."""
    from compress_amd import zstd, _lib
    tw = _twain()
    src = tw[:100000]
    sized = G.zstd_encode_all(src, level=1)
    stream = G.zstd_encode_stream(tw[:300000], level=1)  # window 4 MiB, no content size
    # WithDecoderMaxMemory below a frame's content size
    dec = zstd.NewReader(None, zstd.WithDecoderMaxMemory(len(src) - 1))
    outs, _, status, _ = _decode_dev(dec, [sized])
    dec.Close()
    assert _name(status[0]) == "KC_ZD_SIZE_EXCEEDED" and outs == [b""]
    # WithDecoderMaxWindow below a stream frame's window
    dec = zstd.NewReader(None, zstd.WithDecoderMaxWindow(1 << 20))
    outs, _, status, _ = _decode_dev(dec, [stream])
    dec.Close()
    assert _name(status[0]) == "KC_ZD_WINDOW_EXCEEDED" and outs == [b""]
    # the last checksum byte flipped
    badsum = sized[:-1] + bytes([sized[-1] ^ 0x10])
    assert "CRC check failed" in _ref(G, badsum)[1]
    dec = zstd.NewReader(None)
    outs, _, status, _ = _decode_dev(dec, [badsum, sized])
    dec.Close()
    assert _name(status[0]) == "KC_ZD_CRC" and outs == [b"", src] and status[1] == 0
    dec = zstd.NewReader(None, zstd.IgnoreChecksum(True))
    outs, _, status, _ = _decode_dev(dec, [badsum])
    dec.Close()
    assert status[0] == 0 and outs == [src]
    # dst_cap one byte short
    dec = zstd.NewReader(None)
    with pytest.raises(_lib.KcError) as ei:
        _decode_dev_guarded_short(dec, [sized, stream], len(src) + 300000 - 1)
    dec.Close()
    assert ei.value.status == KC_ERR_DST_TOO_SMALL


def _decode_dev_guarded_short(dec, inputs, cap):
    import torch
    buf, off = corpora.pack_units(inputs)
    d_src = torch.from_numpy(buf).cuda(0)
    d_all = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    try:
        dec.DecodeAllDevice(d_src.data_ptr(), off, d_all.data_ptr() + GUARD, cap)
    finally:
        host = d_all.cpu().numpy()
        assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + cap:] == 0xA5), "written past dst_cap"


def test_host_and_device_entry_points_agree(kclib, G):
    """kc_zstd_decode_all (host buffers) and kc_zstd_decode_all_dev give the same out_off, status and bytes; DecodeAll appends to dst."""
    from compress_amd import zstd
    frames = _fixture_batch() + [b"\x28\xb5\x2f\xfd\x00"]
    dec = zstd.NewReader(None)
    outs, out_off, status, _ = _decode_dev(dec, frames)
    buf, off = corpora.pack_units(frames)
    hout, hoff, hstatus = dec.DecodeUnits(buf, off)
    assert np.array_equal(hoff, out_off) and np.array_equal(hstatus, status) and hout.tobytes() == b"".join(outs)
    assert status[-1] != 0 and sum(int(s) for s in status[:-1]) == 0
    assert dec.DecodeAll(frames[0], b"abc") == b"abc" + outs[0]
    with pytest.raises(zstd.DecodeError) as ei:
        dec.DecodeAll(frames[-1])
    assert ei.value.name == "KC_ZD_EOF"
    with pytest.raises(NotImplementedError):
        dec.Read(bytearray(4))
    dec.Close()


def test_batches_cut_to_the_scratch_budget(kclib, G):
    """With the scratch ceiling at 4 MiB the fixture batch is decoded in several device batches with the same result; at 1 MiB an
    input that cannot fit even alone gets KC_ZD_SIZE_EXCEEDED and its neighbours decode."""
    from compress_amd import zstd, _lib
    frames = _fixture_batch()
    want = [_ref(G, z)[0] for z in frames]
    dec = zstd.NewReader(None)
    dec.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 4)
    outs, _, status, guards = _decode_dev(dec, frames)
    assert guards and not status.any() and outs == want
    assert dec.ctx().get_option(_lib.OPT_LAST_BATCHES) > 1
    dec.ctx().set_option(_lib.OPT_MAX_SCRATCH_MIB, 1)
    tw = _twain()
    big = G.zstd_encode_all((tw * 4)[:1200000], level=1)  # its staging slot alone is above the ceiling
    outs, _, status, guards = _decode_dev(dec, frames[:6] + [big] + frames[6:])
    dec.Close()
    assert guards
    assert _name(status[6]) == "KC_ZD_SIZE_EXCEEDED" and outs[6] == b""
    assert not np.delete(status, 6).any() and outs[:6] + outs[7:] == want


@pytest.mark.parametrize("level", [1, "1L", 2, 3])
def test_round_trip(kclib, level):
    """16 units of 128 KiB of corpus T through the device encoder and back, no sizes supplied."""
    import torch
    from compress_amd import zstd
    n, usz = 16, 128 << 10
    host = corpora.corpus("T", n, usz)
    off = np.arange(n + 1, dtype=np.uint64) * usz
    opts = [zstd.WithEncoderLevel(1), zstd.WithMatchPath("lds")] if level == "1L" else [zstd.WithEncoderLevel(level)] + ([zstd.WithMatchPath("hbm")] if level == 1 else [])
    enc = zstd.NewWriter(None, *opts)
    d_src = torch.from_numpy(host).cuda(0)
    cap = n * ((enc.MaxEncodedSize(usz) + 15) & ~15) + 64
    d_enc = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    eoff = enc.EncodeUnitsDevice(d_src.data_ptr(), off, d_enc.data_ptr(), cap)
    enc.Close()
    dec = zstd.NewReader(None)
    bound, st0 = dec.DecodeBoundsDevice(d_enc.data_ptr(), eoff)
    assert [int(b) for b in bound] == [usz] * n and not st0.any()
    d_out = torch.empty(n * usz, dtype=torch.uint8, device="cuda:0")
    out_off, status = dec.DecodeAllDevice(d_enc.data_ptr(), eoff, d_out.data_ptr(), n * usz)
    dec.Close()
    assert not status.any() and np.array_equal(out_off, off)
    assert torch.equal(d_out, d_src)
