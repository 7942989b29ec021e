"""Inputs, requests and the judging of ranged reads (s2.ReadSeeker.ReadAt as a batch: kc_s2_read_ranges[_dev]) and of the index behind
them, shared by tests/test_emu_s2_ranges.py (the kernels on the CPU wave emulator) and tests/test_gpu_s2_ranges.py (the library on the
device).  Every request is judged by the reference's own Reader (translated: oracle_goref.s2_read_stream): the bytes of request (stream,
off, len) are s2_read_stream(stream)[off:off + len].

A runner is a function run(streams, indexes, requests, cap=None, **reader options) -> RResult; indexes holds per stream None or the
bytes of an index; it puts 64 guard bytes of 0xA5 on both sides of dst and checks them itself."""
import random

import numpy as np

import s2_decode_cases as K

OK, CORRUPT, CRC, UNSUPPORTED = K.OK, K.CORRUPT, K.CRC, K.UNSUPPORTED
EOF, UNEXPECTED_EOF = 5, 6
NAMES = dict(K.NAMES)
NAMES.update({EOF: "EOF", UNEXPECTED_EOF: "UNEXPECTED_EOF"})
BAD_ARG, DST_TOO_SMALL = -1, K.DST_TOO_SMALL
GUARD = K.GUARD
SEED = 0x52D0002
_memo = {}


class RResult:
    def __init__(self, rc, dst, out_off, got, status):
        self.rc, self.dst, self.out_off, self.got, self.status = rc, dst, out_off, got, status

    def range(self, j):
        return self.dst[int(self.out_off[j]):int(self.out_off[j + 1])].tobytes()


def max_buf(max_block):
    """MaxEncodedLen(max_block) + 4 (s2/encode.go:389-418, s2/reader.go:42): the largest chunk the Reader buffers."""
    n = int(max_block)
    n += (n.bit_length() + 7) // 7
    n += 0 if max_block == 0 else 1 if max_block < 60 else 2 if max_block < 1 << 8 else 3 if max_block < 1 << 16 else 4 if max_block < 1 << 24 else 5
    return n + 4


def varint(x):
    """binary.PutVarint: zigzag, then a uvarint."""
    ux = ((x << 1) ^ (x >> 63)) & ((1 << 64) - 1)
    return K.uvarint(ux)


def chunk_table(stream):
    """(header position, end position, decoded length) of every data chunk of a well-formed stream, from its headers alone."""
    out = []
    for p, ty, ln in K.data_chunks(stream):
        if ty == 1:
            dl = ln - 4
        else:
            dl, sh, i = 0, 0, p + 8
            while True:
                dl |= (stream[i] & 0x7F) << sh
                sh += 7
                i += 1
                if not stream[i - 1] & 0x80:
                    break
        out.append((p, p + 4 + ln, dl))
    return out


def bounds_of(stream):
    """Decoded offsets of the chunk boundaries: [0, ..., total]."""
    b = [0]
    for _, _, dl in chunk_table(stream):
        b.append(b[-1] + dl)
    return b


def dense_index(stream):
    """A hand-built index with one entry per data chunk: the entries of the Python Index set directly, then append_to.  (The format
    allows any spacing; only Index.add enforces 1 MiB.)"""
    from compress_amd import s2
    tab = chunk_table(stream)
    ix = s2.Index(tab[0][2])
    u = 0
    for p, _, dl in tab:
        ix.info.append([p, u])
        u += dl
    return ix.append_to(u, len(stream))


def small_streams(G):
    """(name, stream): the 28 KiB text through the reference's Writer in 4 KiB blocks (7 chunks) at levels 0 / 1 / 3, a stream of
    uncompressed chunks out of the compressing Writer (random bytes), a Snappy-framed one, one with flushes that leave 1-byte chunks,
    one with the Writer's own index and 1 024 bytes of padding."""
    if "small" not in _memo:
        t = K.tom()
        out = [("writer level %d" % lv, G.s2_stream(t, level=lv, block_size=4 << 10)) for lv in (0, 1, 3)]
        rnd = np.random.default_rng(11).integers(0, 256, 20000, dtype=np.uint8).tobytes()
        out.append(("uncompressed chunks", G.s2_stream(rnd, block_size=4 << 10)))
        out.append(("snappy", G.s2_stream(t, snappy=True, block_size=4 << 10)))
        cuts = [1, 2, 4097, 4098, 10000, 10001, len(t) - 1]
        out.append(("flushes that leave 1-byte chunks", G.s2_stream(t, flush_at=cuts, block_size=4 << 10)))
        out.append(("index + padding", G.s2_stream(t, add_index=True, padding=1024, block_size=4 << 10)))
        assert all(ty == 1 for _, ty, _ in K.data_chunks(out[3][1]))
        _memo["small"] = out
    return _memo["small"]


def big_stream(G):
    """3 MiB (the text repeated) in 64 KiB blocks with the reference Writer's own index: three entries, 1 MiB apart."""
    if "big" not in _memo:
        t = K.tom()
        data = (t * ((3 << 20) // len(t) + 1))[:3 << 20]
        _memo["big"] = G.s2_stream(data, add_index=True, block_size=64 << 10)
    return _memo["big"]


def decoded(G, stream):
    """The reference Reader's bytes of a stream, computed once and left unchanged."""
    if stream not in _memo:
        _memo[stream] = G.s2_read_stream(stream, 4 << 20)
    return _memo[stream]


def ranges_for(bounds):
    """(off, len) at the smallest shapes at which the clip can go wrong, for a stream with the chunk boundaries `bounds`."""
    total = bounds[-1]
    k = max(range(len(bounds) - 1), key=lambda i: (bounds[i + 1] - bounds[i] >= 16, -abs(i - 2)))  # a chunk of >= 16 bytes near the third
    a, b = bounds[k], bounds[k + 1]
    k3 = min(1, len(bounds) - 4)
    out = [(0, 0), (a + 5, 0), (total, 0),                    # len 0: at offset 0, inside a chunk, at the end
           (a, 1), (b - 1, 1),                                 # 1 byte at the first and the last byte of a chunk
           (a + 3, b - a - 3), (a, 7),                         # ending exactly at a chunk end, starting exactly at one
           (a, b - a),                                         # one chunk exactly
           (b - 1, 2) if b < total else (a - 1, 2),            # 1 byte on each side of a boundary
           (bounds[k3] + 1, bounds[k3 + 3] - bounds[k3] - 2),  # three chunks, both edges clipped
           (0, total),                                         # the whole stream
           (total, 10),                                        # off == total: EOF, got 0
           (total - 5, 100),                                   # a short read
           (total + 1, 10), (total + 1, 0),                    # off > total: unexpected EOF (Find with an index, Skip without)
           (b, 0)]                                             # len 0 at a chunk's end: nothing is decoded
    for i in range(len(bounds) - 1):                           # every chunk of one byte, alone and with its neighbours
        if bounds[i + 1] - bounds[i] == 1:
            out += [(bounds[i], 1), (max(bounds[i] - 1, 0), 3)]
    return out


def expect(dec, off, ln):
    """(status, bytes) a request must come back with."""
    if off > len(dec):
        return UNEXPECTED_EOF, b""
    got = dec[off:off + ln]
    return (OK if len(got) == ln else EOF), got


def check(res, requests, want, what=""):
    """Every request against (status, bytes): the layout, got, the bytes, the zero-filled rest.  Returns {status: count}."""
    assert res.rc == 0, res.rc
    assert [int(x) for x in res.out_off] == [0] + [int(x) for x in np.cumsum([r[2] for r in requests], dtype=np.uint64)], "out_off is not the prefix sum of the lengths"
    classes = {}
    for j, ((st, data), r) in enumerate(zip(want, requests)):
        assert int(res.status[j]) == st, (what, j, r, NAMES[int(res.status[j])], NAMES[st])
        assert int(res.got[j]) == len(data), (what, j, r, int(res.got[j]), len(data))
        rng = res.range(j)
        assert rng[:len(data)] == data, (what, j, r, "bytes differ")
        assert rng[len(data):] == b"\0" * (len(rng) - len(data)), (what, j, r, "the rest of the range is not zero")
        classes[st] = classes.get(st, 0) + 1
    return classes


def everything(G):
    """The batch that mixes all streams and requests: (streams, indexes, requests, want).  Every small stream stands there twice —
    without an index and with its dense one — beside the stream that carries the Writer's index, and the 3 MiB stream with and
    without the Writer's index."""
    streams, indexes, requests, want = [], [], [], []

    def add(stream, index, ranges):
        dec = decoded(G, stream)
        streams.append(stream)
        indexes.append(index)
        for off, ln in ranges:
            requests.append((len(streams) - 1, off, ln))
            want.append(expect(dec, off, ln))

    for _, s in small_streams(G):
        r = ranges_for(bounds_of(s))
        add(s, None, r)
        add(s, dense_index(s), r)
    s = small_streams(G)[-1][1]
    add(s, writer_index(s), ranges_for(bounds_of(s)))
    big = big_stream(G)
    M = 1 << 20
    br = [(M + 100, 4096), (M - 10, 20), (2 * M + 5 * 65536 + 5, 3000), (3 * M - 100, 200), (M + 3 * 65536 + 5, 70000), (2 * M, 1), (3 * M, 0), (3 * M + 1, 1),
          (65536 * 7 - 1, 2), (0, 100)]
    add(big, writer_index(big), br)
    add(big, None, [(2 * M + 7, 1000), (65536 * 9 + 1, 65536)])
    return streams, indexes, requests, want


def writer_index(stream):
    """The bytes of the index chunk at the end of a stream the reference's Writer closed with WriterAddIndex."""
    assert stream[-6:] == b"\x00xdi2s"
    sz = int.from_bytes(stream[-10:-6], "little")
    return stream[-sz:]


# ---- Index.Load: one case per return statement of s2/index.go:238-374 ----
def _wrap(body, header=b"s2idx\x00", trailer=b"\x00xdi2s", chunk_type=0x99, tail=True):
    b = bytearray([chunk_type, 0, 0, 0]) + header + body
    if tail:
        b += (len(b) + 10).to_bytes(4, "little") + trailer
    n = len(b) - 4
    b[1:4] = bytes([n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF])
    return bytes(b)


def load_cases():
    """(name with the index.go line of the return it reaches, index bytes, expected status, rest).  Hand-built from reading Index.Load:
    no translated Load exists to judge them."""
    v = varint
    bad = b"\xff" * 9 + b"\x7f"  # binary.Varint: overflow, n < 0
    big = 1 << 40               # a six-byte varint: keeps short bodies above the 16 bytes of the first check
    good = _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x00" + v(10) + v(0))
    return [
        ("index.go:240 sixteen bytes or fewer", good[:16], UNEXPECTED_EOF, None),
        ("index.go:243 not an index chunk", _wrap(v(8192) + v(5000) + v(4096) + v(0) + b"\x00", chunk_type=0x98), CORRUPT, None),
        ("index.go:250 shorter than its chunk length", good[:-1], UNEXPECTED_EOF, None),
        ("index.go:253 another header", _wrap(v(8192) + v(5000) + v(4096) + v(0) + b"\x00", header=b"s2idy\x00"), UNSUPPORTED, None),
        ("index.go:259 total uncompressed negative", _wrap(v(-1) + v(5000) + v(4096) + v(0) + b"\x00"), CORRUPT, None),
        ("index.go:259 total uncompressed overflows", _wrap(bad + v(5000) + v(4096) + v(0) + b"\x00"), CORRUPT, None),
        ("index.go:267 total compressed overflows", _wrap(v(8192) + bad + v(4096) + v(0) + b"\x00"), CORRUPT, None),
        ("index.go:275 block estimate overflows", _wrap(v(8192) + v(5000) + bad + v(0) + b"\x00"), CORRUPT, None),
        ("index.go:278 block estimate negative", _wrap(v(8192) + v(5000) + v(-4096) + v(0) + b"\x00"), CORRUPT, None),
        ("index.go:286 entry count overflows", _wrap(v(8192) + v(5000) + v(4096) + bad + b"\x00"), CORRUPT, None),
        ("index.go:289 more than 65536 entries", _wrap(v(8192) + v(5000) + v(4096) + v(65537) + b"\x00"), CORRUPT, None),
        ("index.go:289 negative entry count", _wrap(v(8192) + v(5000) + v(4096) + v(-1) + b"\x00"), CORRUPT, None),
        ("index.go:300 ends behind the entry count", _wrap(v(big) + v(big) + v(4096) + v(0), tail=False), UNEXPECTED_EOF, None),
        ("index.go:305 hasUncompressed is 2", _wrap(v(8192) + v(5000) + v(4096) + v(0) + b"\x02"), CORRUPT, None),
        ("index.go:314 an uncompressed delta overflows", _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x01" + v(0) + bad + v(10) + v(0)), CORRUPT, None),
        ("index.go:325 uncompressed offsets do not ascend", _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x01" + v(0) + v(-4096) + v(10) + v(0)), CORRUPT, None),
        ("index.go:329 first uncompressed offset negative", _wrap(v(8192) + v(5000) + v(4096) + v(1) + b"\x01" + v(-5) + v(10)), CORRUPT, None),
        ("index.go:341 a compressed delta overflows", _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x00" + v(10) + bad), CORRUPT, None),
        ("index.go:341 the compressed deltas are missing", _wrap(v(big) + v(big) + v(4096) + v(2) + b"\x00", tail=False), CORRUPT, None),
        ("index.go:354 compressed offsets do not ascend", _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x00" + v(10) + v(-2048)), CORRUPT, None),
        ("index.go:359 first compressed offset negative", _wrap(v(8192) + v(5000) + v(4096) + v(1) + b"\x00" + v(-3)), CORRUPT, None),
        ("index.go:364 no room for size and trailer", _wrap(v(big) + v(big) + v(4096) + v(1) + b"\x00" + v(10) + b"\0" * 9, tail=False), UNEXPECTED_EOF, None),
        ("index.go:371 another trailer", _wrap(v(8192) + v(5000) + v(4096) + v(2) + b"\x00" + v(10) + v(0), trailer=b"\x00xdi2t"), CORRUPT, None),
        ("index.go:373 loaded, the rest returned", good + b"rest", OK, b"rest"),
    ]


# ---- corrupt input under a dense index ----
def covered_span(stream, off, ln):
    """(first covered header, end of the last covered chunk, decoded offset of the first covered chunk, [(header, end)] of the covered
    chunks) of request (off, ln), 0 < ln, off + ln <= total, in a well-formed stream read through its dense index."""
    tab, u, cov, u0 = chunk_table(stream), 0, [], None
    for p, e, dl in tab:
        if u + dl > off and u < off + ln:
            if u0 is None:
                u0 = u
            cov.append((p, e))
        u += dl
    return cov[0][0], cov[-1][1], u0, cov


def _chunk_at(mut, pos):
    """(type, chunk length, decoded length) of the chunk whose header stands at pos, by the header and the uvarint alone; None where
    they do not parse (short, a reserved type, a stored chunk shorter than its CRC, a uvarint that does not end)."""
    if pos + 4 > len(mut):
        return None
    ty, ln = mut[pos], mut[pos + 1] | mut[pos + 2] << 8 | mut[pos + 3] << 16
    if pos + 4 + ln > len(mut) or 2 <= ty < 0x80:
        return None
    if ty == 1:
        return (ty, ln, ln - 4) if ln >= 4 else None
    if ty != 0:
        return ty, ln, 0
    dl, sh, i = 0, 0, pos + 8
    while True:
        if i >= pos + 4 + ln or sh > 28:
            return None
        dl |= (mut[i] & 0x7F) << sh
        sh += 7
        i += 1
        if not mut[i - 1] & 0x80:
            return ty, ln, dl


def walk_cut(mut, c, need):
    """The end of the chunk at which a walk of the mutated bytes from header position c has passed `need` decoded bytes, by the headers
    and uvarints alone; the stream's end where that walk cannot finish."""
    pos, have = c, 0
    while have < need:
        h = _chunk_at(mut, pos)
        if h is None:
            return len(mut)
        have += h[2]
        pos += 4 + h[1]
    return pos


def skipped_front(mut, c, u0, off):
    """Where Reader.Skip stands when it has passed, by their headers alone, the data chunks from header position c (decoded offset u0)
    that end at or before off (reader.go:761-766): (header position, decoded offset).  In a pristine stream read through its dense
    index that is (c, u0) itself; a mutation that shrinks the first covered chunk's stated length to off - u0 or less makes the
    reference skip that chunk instead of decoding it, and the judge — the sequential Reader — has to start behind it to make the
    reads ReadAt makes."""
    pos, u = c, u0
    while u < off:
        h = _chunk_at(mut, pos)
        if h is None or h[0] > 1 or u + h[2] > off:
            break
        pos += 4 + h[1]
        u += h[2]
    return pos, u


def corrupt_cases(G, n=480, seed=SEED):
    """Case k: base k mod 7 of the small streams read through its dense index, a seeded request inside it and one flipped bit; kinds by
    k mod 3: (a) anywhere inside the covered span, (b) in a covered chunk's header or the 16 bytes behind it, (c) outside the covered
    span — before the first covered header (behind the stream identifier, which a ranged read does read: it sets the reader's state)
    or behind the last covered chunk.  Returns (mutated stream, index bytes, (off, len), kind, judge input, offset in the judge's
    output) per case.  The judge reads the stream's own identifier followed by mutated[first covered header : cut] — the first
    covered header by the mutated headers: see skipped_front."""
    rnd = random.Random(seed)
    bases = [s for _, s in small_streams(G)]
    dense = [dense_index(s) for s in bases]
    out = []
    for k in range(n):
        s = bases[k % len(bases)]
        total = bounds_of(s)[-1]
        kind = "abc"[k % 3]
        while True:
            off = rnd.randrange(total - 1)
            ln = rnd.randrange(1, min(total - off, 9000) + 1)
            c, e, u0, cov = covered_span(s, off, ln)
            if kind != "c" or c > 10 or e < len(s):
                break
        b = bytearray(s)
        if kind == "a":
            p = rnd.randrange(c, e)
        elif kind == "b":
            h, he = rnd.choice(cov)
            p = min(h + rnd.randrange(20), he - 1)
        else:
            outside = list(range(10, c)) + list(range(e, len(s)))
            p = rnd.choice(outside)
        b[p] ^= 1 << rnd.randrange(8)
        mut = bytes(b)
        c1, u1 = skipped_front(mut, c, u0, off)
        cut = walk_cut(mut, c1, (off - u1) + ln)
        out.append((mut, dense[k % len(bases)], (off, ln), kind, s[:10] + mut[c1:cut], off - u1))
    return out


def judge_range(G, judge_input, rel, ln):
    """(status, bytes) from the reference's sequential Reader over the judge's input."""
    kind, v = K.judge_stream(G, judge_input, 1 << 20)
    if kind == "err":
        return v, b""
    if rel > len(v):
        return UNEXPECTED_EOF, b""
    got = v[rel:rel + ln]
    return (OK if len(got) == ln else EOF), got
