"""Shared by tests/test_emu_zstd_dstream.py (the stream reader's kernels and state machine on the CPU wave emulator) and
tests/test_gpu_zstd_dstream.py (kc_zstd_dstream_feed on the device): a driver that feeds a stream in pieces with guard bytes around
dst, the reference's verdict restated for the stream form, and the inputs both files decode.

The judge is the reference's own DecodeAll (oracle_goref.zstd_decode_all): the bytes of a valid stream are the same whichever way it
is read.  Where it refuses, the stream reader reports the class of its message, with the substitutions the stream form of the
reference makes (include/kcgpu.h, kc_zdstream_host.h):
  * a window descriptor above WithDecoderMaxWindow: KC_ZD_SIZE_EXCEEDED instead of KC_ZD_WINDOW_EXCEEDED;
  * a Frame_Content_Size above WithDecoderMaxMemory behind a window descriptor: the limit does not bound a stream's total, so the
    frame is decoded and fails where its content falls short of what it promised: KC_ZD_CORRUPT (ErrFrameSizeMismatch), or KC_ZD_EOF."""
import ctypes as C
import os
import random
import zipfile

import numpy as np

import zstd_frame_cases as zc

HERE = os.path.dirname(os.path.abspath(__file__))
REFIN = os.path.join(HERE, "golden", "ref_inputs")
GUARD = 64
NAMES = zc.NAMES
FEED_ARGS = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]


def members(name, suffix=None):
    z = zipfile.ZipFile(os.path.join(REFIN, name))
    return [(m, z.read(m)) for m in z.namelist() if not m.endswith("/") and (suffix is None or m.endswith(suffix))]


def twain():
    return open(os.path.join(REFIN, "Mark.Twain-Tom.Sawyer.txt"), "rb").read()


class Stream:
    """new() -> handle, feed and free as kc_zstd_dstream_feed / _free take them behind the handle."""

    def __init__(self, new, feed, free):
        self.new, self.feed, self.free = new, feed, free


def run(S, data, piece=None, cuts=None, dst_cap=256 << 10):
    """Feeds `data` whole (piece None), in pieces of `piece` bytes, or cut at the positions `cuts`.  Every call gets a dst of dst_cap
    bytes with GUARD bytes of 0xA5 on both sides, checked after the call.  Returns (delivered bytes, status, kc_status)."""
    data = bytes(data)
    if cuts is None:
        cuts = list(range(piece, len(data), piece)) if piece else []
    bounds = sorted(set(int(x) for x in cuts if 0 < x < len(data))) + [len(data)]
    buf = np.full(dst_cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    consumed, produced, status = C.c_uint64(), C.c_uint64(), C.c_uint32()
    h = S.new()
    assert h
    out = bytearray()
    pend, pos = b"", 0
    try:
        for b in bounds:
            pend += data[pos:b]
            pos = b
            eof = int(b == len(data))
            while True:
                rc = S.feed(h, pend, len(pend), eof, buf.ctypes.data + GUARD, dst_cap, C.byref(consumed), C.byref(produced), C.byref(status))
                assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + dst_cap:] == 0xA5), "written outside dst"
                if rc != 0:
                    return bytes(out), int(status.value), rc
                assert consumed.value <= len(pend) and produced.value <= dst_cap
                out += buf[GUARD:GUARD + produced.value].tobytes()
                pend = pend[consumed.value:]
                if status.value:
                    return bytes(out), int(status.value), 0
                if not (consumed.value or produced.value):
                    break
        assert pend == b"", "a clean end leaves nothing unconsumed"
        return bytes(out), 0, 0
    finally:
        S.free(h)


def first_header(z):
    """(window from the descriptor or None, single segment, content size or None) of the first frame behind any skippable ones."""
    p = 0
    while len(z) - p >= 8 and z[p + 1:p + 4] == b"\x2a\x4d\x18" and (z[p] & 0xF0) == 0x50:
        p += 8 + int.from_bytes(z[p + 4:p + 8], "little")
    if len(z) - p < 6 or z[p:p + 4] != b"\x28\xb5\x2f\xfd":
        return None
    fhd = z[p + 4]
    q = p + 5
    single = bool((fhd >> 5) & 1)
    window = None
    if not single:
        wd = z[q]
        q += 1
        base = 1 << (10 + (wd >> 3))
        window = base + (base // 8) * (wd & 7)
    q += [0, 1, 2, 4][fhd & 3]
    fsz = [1 if single else 0, 2, 4, 8][fhd >> 6]
    if len(z) - q < fsz:
        return None
    fcs = None
    if fsz:
        fcs = int.from_bytes(z[q:q + fsz], "little") + (256 if fsz == 2 else 0)
    return window, single, fcs


def expected_classes(z, err, max_window=1 << 29, max_memory=64 << 30):
    """The classes the stream reader may report where the reference's DecodeAll says `err`."""
    cls = zc.message_class(err)
    h = first_header(z)
    if h is not None:
        window, single, fcs = h
        if cls == "WINDOW_EXCEEDED" and window is not None and window > max_window:
            return {"SIZE_EXCEEDED"}
        if cls == "SIZE_EXCEEDED" and window is not None and window <= min(max_window, max_memory) and fcs is not None and fcs > max_memory:
            return {"CORRUPT", "EOF"}
    return {cls}


def mutation_cases(G):
    """The 30 frames x 16 seeded mutations of tests/test_gpu_zstd_decode_all.py::test_differential_on_mutations, built the same way."""
    tw = twain()
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
    return cases


_refs = {}


def ref(G, z, cap=1 << 20, **kw):
    """The reference's DecodeAll: (bytes, None) or (None, message).  Computed once per input and left unchanged."""
    key = (bytes(z), cap, tuple(sorted((k, bytes(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in kw.items())))
    if key not in _refs:
        try:
            _refs[key] = (G.zstd_decode_all(z, cap, **kw), None)
        except ValueError as e:
            _refs[key] = (None, str(e))
    return _refs[key]


def judge_one(name, z, want, err, out, status, rc, plain=None, loose_eof=False):
    """What is wrong with one stream's outcome (None: nothing).  loose_eof: KC_ZD_EOF and KC_ZD_CORRUPT count as one class."""
    if rc != 0:
        return "%s: kc_status %d" % (name, rc)
    if want is not None:
        if status != 0 or out != want:
            return "%s: reference returns %d bytes, stream status %s with %d bytes" % (name, len(want), NAMES.get(status, status), len(out))
        return None
    if status == 0:
        return "%s: reference refuses (%s), stream returns %d bytes without an error" % (name, err, len(out))
    exp = expected_classes(z, err)
    got = NAMES.get(status, str(status))
    if loose_eof and got in ("EOF", "CORRUPT") and exp & {"EOF", "CORRUPT"}:
        got = next(iter(exp & {"EOF", "CORRUPT"}))
    if got not in exp:
        return "%s: reference refuses (%s), class %s, stream status %s" % (name, err, "/".join(sorted(exp)), NAMES.get(status, status))
    if plain is not None and plain[:len(out)] != out:
        return "%s: the bytes in front of the error are no prefix of the plaintext" % name
    return None


def dict_frames():
    ms = members("dict-tests-small.zip")
    dicts = {int.from_bytes(d[4:8], "little"): d for m, d in ms if m.endswith(".dict")}
    frames = [(m, d) for m, d in ms if m.endswith(".zst")]
    assert len(dicts) == 3 and len(frames) == 41
    return dicts, frames


def frame_dict_id(z):
    fhd = z[4]
    p = 5 + (0 if (fhd >> 5) & 1 else 1)
    return int.from_bytes(z[p:p + [0, 1, 2, 4][fhd & 3]], "little")


def composite(G):
    """frame + skippable frame + stream frame + empty frame + skippable(0), its plaintext, and cut points inside the magic, the frame
    header, a block header, the skippable payload and the checksum."""
    import zstd_frame_builder as zb
    tw = twain()
    f1, p1 = zc.frame([zc.raw(tw[:500]), zc.seqblock([(4, 9, 3 + 2)], 3)], checksum=True, xxh64=zc._xxh64)
    sk = zb.skippable(b"x" * 300, 3)
    f2 = G.zstd_encode_stream(tw[1000:200000], level=1, crc=True)
    f3 = zc.frame([zc.raw(b"")])[0]  # an empty frame
    data = f1 + sk + f2 + f3 + zb.skippable(b"")
    a, b = len(f1), len(f1) + len(sk)
    hdr2 = 4 + 1 + 1  # magic, descriptor, window descriptor of the stream frame (no content size, no dictionary)
    cuts = [2, 5, a - 2, a + 3, a + 6, a + 150, b + 2, b + 5, b + hdr2 + 1, b + len(f2) - 2, len(data) - 3]
    return data, p1 + tw[1000:200000], cuts
