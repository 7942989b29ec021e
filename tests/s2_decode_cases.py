"""Inputs and the judging of the s2.Reader / s2.Decode product path, shared by tests/test_emu_s2_decode_all.py (the kernels on the CPU wave
emulator) and tests/test_gpu_s2_decode_all.py (the library on the device).  Every case is judged by the reference's own Reader / Decode
(translated: oracle_goref.s2_read_stream / s2_decode): where it returns bytes the status is 0 and the bytes are equal; where it raises,
the status class equals its message's class and the input's range in dst is all zero.

A runner is a function run(inputs, blocks=False, max_block=4 << 20, ignore_crc=False, ignore_id=False, cap=None) that returns a Result;
it puts 64 guard bytes of 0xA5 on both sides of dst and checks them itself."""
import os
import random
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
S2IN = os.path.join(HERE, "golden", "ref_inputs", "s2")
OK, CORRUPT, CRC, UNSUPPORTED, SIZE_EXCEEDED = 0, 1, 2, 3, 4
NAMES = {0: "OK", 1: "CORRUPT", 2: "CRC", 3: "UNSUPPORTED", 4: "SIZE_EXCEEDED"}
DST_TOO_SMALL = -2
GUARD = 64
MAGIC = b"\xff\x06\x00\x00S2sTwO"
SEED = 0x52D0001


class Result:
    def __init__(self, rc, dst, out_off, status, bound):
        self.rc, self.dst, self.out_off, self.status, self.bound = rc, dst, out_off, status, bound

    def out(self, i):
        return self.dst[int(self.out_off[i]):int(self.out_off[i + 1])].tobytes()


def pack(inputs):
    off = np.zeros(len(inputs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in inputs], dtype=np.uint64)
    return np.frombuffer(b"".join(inputs) + b"\0", dtype=np.uint8).copy(), off


def tom():
    """Tom Sawyer x 2 (28 KiB)."""
    return open(os.path.join(S2IN, "Mark.Twain-Tom.Sawyer.txt"), "rb").read() * 2


def item1_streams(G):
    """The batch of everything: (name, stream, decoded bytes or None when only the judge knows).  The first eight are the mutation bases."""
    t = tom()
    out = []
    for level in (0, 1, 3):
        for bs in (4 << 10, 16 << 10):
            out.append(("writer level %d block %d" % (level, bs), G.s2_stream(t, level=level, block_size=bs), t))
    out.append(("snappy 8 KiB", G.s2_stream(t, snappy=True, block_size=8 << 10), t))
    out.append(("index + padding", G.s2_stream(t, add_index=True, padding=1024, block_size=4 << 10), t))
    out.append(("empty", b"", b""))
    out.append(("identifier only", MAGIC, b""))
    out.append(("two streams, the second Snappy", G.s2_stream(t[:9000], block_size=4 << 10) + G.s2_stream(t[9000:], snappy=True, block_size=4 << 10), t))
    cuts = [1, 2, 4097, 4098, 10000, 10001, len(t) - 1]
    out.append(("flushes that leave 1-byte chunks", G.s2_stream(t, flush_at=cuts, block_size=4 << 10), t))
    return out


def headers(stream):
    """Positions of the 4-byte chunk headers of a well-formed stream."""
    pos, out = 0, []
    while pos + 4 <= len(stream):
        out.append(pos)
        pos += 4 + (stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16)
    return out


def data_chunks(stream):
    """(header position, type, length) of the data chunks (types 0 and 1) of a well-formed stream."""
    return [(p, stream[p], stream[p + 1] | stream[p + 2] << 8 | stream[p + 3] << 16) for p in headers(stream) if stream[p] <= 1]


def mutations(bases, n=480, seed=SEED):
    """Case k mutates base k mod 8; kinds by k mod 6: a bit flip anywhere, a truncation, a bit flip in some chunk's 4-byte header, a bit flip
    in the first 16 bytes behind a header, a one-byte insertion, a one-byte deletion."""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        b = bytearray(bases[k % 8])
        kind = k % 6
        if kind == 0:
            b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        elif kind == 1:
            b = b[:rnd.randrange(len(b))]
        elif kind == 2:
            h = rnd.choice(headers(bytes(b)))
            b[h + rnd.randrange(4)] ^= 1 << rnd.randrange(8)
        elif kind == 3:
            h = rnd.choice(headers(bytes(b)))
            p = min(h + 4 + rnd.randrange(16), len(b) - 1)
            b[p] ^= 1 << rnd.randrange(8)
        elif kind == 4:
            b.insert(rnd.randrange(len(b) + 1), rnd.getrandbits(8))
        else:
            del b[rnd.randrange(len(b))]
        out.append(bytes(b))
    return out


def judge_stream(G, stream, max_out, max_block=0, ignore_crc=False):
    """('ok', bytes) or ('err', class) from the reference's own Reader."""
    try:
        return "ok", G.s2_read_stream(stream, max_out, max_block=max_block, ignore_crc=ignore_crc)
    except ValueError as e:
        m = str(e)
        assert m.endswith("(-5)"), m  # the Reader's own error, not a failure of the harness
        if "crc mismatch" in m:
            return "err", CRC
        if "corrupt input" in m:
            return "err", CORRUPT
        assert "unsupported input" in m, m
        return "err", UNSUPPORTED


def judge_block(G, block, max_out):
    try:
        return "ok", G.s2_decode(block, max_out)
    except ValueError:
        return "err", CORRUPT  # (s2.Decode has one error on a 64-bit build: ErrCorrupt)


def check(res, verdicts, what=""):
    """Every input against its verdict; the layout against the bounds.  Returns (n decoded, {class: count})."""
    n = len(verdicts)
    assert res.rc == 0, res.rc
    assert int(res.out_off[0]) == 0
    assert [int(x) for x in res.out_off[1:]] == [int(x) for x in np.cumsum(res.bound[:n], dtype=np.uint64)], "out_off is not the prefix sum of bound"
    ok, classes = 0, {}
    for i, (kind, v) in enumerate(verdicts):
        got = res.out(i)
        if kind == "ok":
            assert int(res.status[i]) == OK, (what, i, NAMES[int(res.status[i])])
            assert got == v, (what, i, len(got), len(v))
            assert int(res.bound[i]) == len(v), (what, i)
            ok += 1
        else:
            assert int(res.status[i]) == v, (what, i, NAMES[int(res.status[i])], NAMES[v])
            assert got == b"\0" * len(got), (what, i, "bytes of a refused input left in dst")
            classes[v] = classes.get(v, 0) + 1
    return ok, classes


# ---- hand-built blocks through the reference's own emitters ----
def uvarint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def expand(ops):
    """The bytes a list of operations decodes to: ('lit', bytes) | ('copy' | 'repeat' | 'copy_norepeat', offset, length)."""
    out = bytearray()
    for op in ops:
        if op[0] == "lit":
            out += op[1]
        else:
            off, ln = op[1], op[2]
            if off >= ln:
                out += out[len(out) - off:len(out) - off + ln]
            else:
                pat = bytes(out[len(out) - off:])
                out += (pat * (ln // off + 1))[:ln]
    return bytes(out)


def block_of(G, ops):
    body = bytearray()
    for op in ops:
        body += G.s2_emit("literal", 0, 0, op[1]) if op[0] == "lit" else G.s2_emit(op[0], op[1], op[2])
    return uvarint(len(expand(ops))) + bytes(body)


def chunk_of(block, decoded):
    """The block as a compressed chunk with the CRC of its decoded bytes."""
    c = crc32c_masked(decoded)
    n = len(block) + 4
    return bytes([0, n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF]) + c.to_bytes(4, "little") + block


_CRC_T = None


def crc32c_masked(b):
    global _CRC_T
    if _CRC_T is None:
        _CRC_T = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            _CRC_T.append(c)
    c = 0xFFFFFFFF
    for x in b:
        c = _CRC_T[(c ^ x) & 0xFF] ^ (c >> 8)
    c ^= 0xFFFFFFFF
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def hand_blocks(G):
    """(name, block) without the 16 MiB one: copies at offsets 1-17 x the lengths around a lane's word and the wave, repeats in all four
    length forms, the four short literal forms, blocks of exactly 63 / 64 / 65 / 128 / 129 operations, a literal across a 64-byte
    window, a last tag inside the last 5 bytes."""
    rnd = random.Random(7)
    seed = bytes(rnd.getrandbits(8) for _ in range(40))
    out = []
    for off in range(1, 18):
        ops = [("lit", seed)]
        for ln in (4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129, 1000):
            ops.append(("copy", off, ln))
            ops.append(("lit", bytes([rnd.getrandbits(8)])))
        out.append(("copies at offset %d" % off, block_of(G, ops)))
    ops = [("lit", seed), ("copy", 7, 9)]
    for ln in (4, 8, 11, 12, 259, 260, 300, 65791, 65792, 70000):  # repeat lengths: in the tag, + 1, + 2, + 3 bytes
        ops.append(("repeat", 7, ln))
        ops.append(("lit", b"x"))
        ops.append(("copy", 7, 5))  # (a repeat takes the offset of the copy before it)
    out.append(("repeats", block_of(G, ops)))
    ops = []
    for ln in (1, 60, 61, 256, 257, 65536, 65537):  # literal tags of 1, 2, 3 and 4 bytes
        ops.append(("lit", bytes(rnd.getrandbits(8) for _ in range(ln))))
        ops.append(("copy", 1, 4))
    out.append(("literal forms", block_of(G, ops)))
    for nops in (63, 64, 65, 128, 129):
        ops = [("lit", seed)]
        while len(ops) < nops:
            ops.append(("copy", 1 + rnd.randrange(30), 4 + rnd.randrange(20)) if len(ops) % 2 else ("lit", bytes(rnd.getrandbits(8) for _ in range(1 + rnd.randrange(5)))))
        out.append(("%d operations" % nops, block_of(G, ops)))
    # a literal that starts in one 64-byte window of the tag stream and ends past it
    out.append(("literal across a window", block_of(G, [("lit", seed[:30]), ("copy", 3, 10), ("copy", 20, 8), ("lit", bytes(range(200))), ("copy", 100, 50)])))
    # the last tag starts in the last 5 bytes: copy2 (3 bytes), copy1 (2 bytes), a 1-byte literal, a repeat with one length byte
    for tail in ([("copy", 3000, 20)], [("copy", 5, 6)], [("lit", b"z")], [("copy", 9, 5), ("repeat", 9, 100)]):
        out.append(("short tail %s" % tail[-1][0], block_of(G, [("lit", bytes(rnd.getrandbits(8) for _ in range(4000)))] + tail)))
    return out


def regression_blocks():
    z = zipfile.ZipFile(os.path.join(S2IN, "dec-block-regressions.zip"))
    return [(m, z.read(m)) for m in z.namelist() if not m.endswith("/")]


def first_error_cases(G):
    """(name, stream): two faults each; the first in stream order decides.  Built on a stream of 4 KiB chunks (chunk 0 is the first
    data chunk)."""
    t = tom()
    s = G.s2_stream(t, block_size=4 << 10)
    dc = data_chunks(s)
    assert len(dc) >= 6 and all(ty == 0 for _, ty, _ in dc[:6])

    def crc_flip(b, k):
        b[dc[k][0] + 4] ^= 0x40

    def break_body(b, k):  # the block's uvarint says one byte more than the tags produce: decode error, not a header-level one
        p = dc[k][0] + 8
        v, sh, i = 0, 0, 0
        while True:
            v |= (b[p + i] & 0x7F) << sh
            sh += 7
            i += 1
            if not b[p + i - 1] & 0x80:
                break
        enc = uvarint(v + 1)
        assert len(enc) == i
        b[p:p + i] = enc

    def bad_type(b, k):
        b[dc[k][0]] = 0x02

    out = []
    b = bytearray(s)
    crc_flip(b, 1)
    cut = dc[3][0] + 4 + dc[3][2] // 2
    out.append(("CRC in chunk 1, truncation inside chunk 3", bytes(b[:cut]), CRC))
    b = bytearray(s)
    bad_type(b, 2)
    break_body(b, 4)
    out.append(("type 0x02 at chunk 2, broken body in chunk 4", bytes(b), UNSUPPORTED))
    b = bytearray(s)
    break_body(b, 1)
    bad_type(b, 2)
    out.append(("broken body in chunk 1, type 0x02 at chunk 2", bytes(b), CORRUPT))
    return out
