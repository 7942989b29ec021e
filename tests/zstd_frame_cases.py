"""Hand-built zstd frames for the DecodeAll path, shared by tests/test_zstd_decode_shapes.py (the builder against the reference, the
oracle and the kernels on the CPU wave emulator) and tests/test_gpu_zstd_decode_shapes.py (the library on the device).  The frames come
from tests/zstd_frame_builder.py and reach the shapes of the format that neither the reference's fixture archives nor any encoder here
emits: RLE blocks and RLE literals, directly coded Huffman weights, weight table logs other than 5, the 3-byte sequence count, repeat
codes 2 and 3, small windows, offset codes above 24, and the edges of the 64-sequence group executor.

A case is (name, input bytes, decoder options, dictionaries, expectation) with the section it belongs to, the builder's plaintext and,
for a directed refusal, its status class.  The decoder options are the defaults for every case (the reference's judge takes none); the
dictionaries are raw ones, chosen by id.  expectation: "valid" (the builder's plaintext), "refused" (wrong by one named field) or
"judge" (the reference's DecodeAll decides)."""
import collections
import ctypes as C
import os
import random

import numpy as np

import zstd_frame_builder as zb
from zstd_frame_builder import Block, Lits, frame, RLE, FSE, REPEAT

Case = collections.namedtuple("Case", "name section data opts dicts expect plain cls big")
NAMES = {0: "OK", 1: "MAGIC", 2: "EOF", 3: "UNKNOWN_DICT", 4: "WINDOW_EXCEEDED", 5: "SIZE_EXCEEDED", 6: "CRC", 7: "CORRUPT"}
GUARD = 64
W1K, W8M, W64M, W1G = 0x00, 0x68, 0x80, 0xA0  # Window_Descriptor bytes: exponent << 3 | mantissa, window = 2^(10 + exponent) * (1 + mantissa / 8)
BLOCK = 128 << 10


def rnd(n, seed=1, alphabet=256):
    r = random.Random(0x2D5EED00 + seed)
    return bytes(r.randrange(alphabet) for _ in range(n))


DICTS = {5: rnd(300, 5), 300: rnd(700, 300), 70000: rnd(1500, 70000)}


def comp(lits, seqs=(), **kw):
    return Block("compressed", lits=lits if isinstance(lits, Lits) else Lits("raw", lits), seqs=seqs, **kw)


def raw(data, **kw):
    return Block("raw", data, **kw)


def rle(byte, n, **kw):
    return Block("rle", bytes([byte]), n=n, **kw)


def seqblock(seqs, trailing=0, seed=7, **kw):
    """A compressed block with raw random literals: as many as the sequences consume, plus `trailing`."""
    return comp(rnd(sum(s[0] for s in seqs) + trailing, seed), seqs, **kw)


def _xxh64(b):
    import oracle_lib
    return int(oracle_lib.lib().kco_xxh64(b, len(b)))


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def _build():
    out = []
    section = [None]

    def add(name, expect, fr, dict_id=None, cls=None, big=False):
        if isinstance(fr, tuple) and len(fr) == 3:
            dict_id = fr[2]
        data, plain = fr[:2] if isinstance(fr, tuple) else (fr, b"")
        assert expect in ("valid", "refused", "judge")
        out.append(Case(name, section[0], bytes(data), {}, (dict_id,) if dict_id is not None else (), expect, plain if expect == "valid" else None, cls, big))

    def fd(blocks, dict_id, **kw):
        return frame(blocks, dict_id=dict_id, dict_content=DICTS[dict_id], **kw) + (dict_id,)

    # ---- frame header and plan ------------------------------------------------------------------------------------------------
    section[0] = "header"
    t = rnd(40, 2, 26)
    add("fcs 0 bytes, window descriptor", "valid", frame([raw(t)], window_desc=0x50))
    add("fcs 1 byte", "valid", frame([raw(t)], fcs_bytes=1))
    add("fcs 2 bytes, 256", "valid", frame([rle(0x41, 256)], fcs_bytes=2))
    add("fcs 2 bytes, 65791", "valid", frame([rle(0x42, 65791)], fcs_bytes=2))
    add("fcs 4 bytes", "valid", frame([raw(t)], fcs_bytes=4))
    add("fcs 8 bytes", "valid", frame([raw(t)], fcs_bytes=8))
    add("fcs 8 bytes says 2^40", "refused", frame([raw(t)], fcs_bytes=8, content_size=1 << 40))
    add("fcs 8 bytes says 2^37 behind a window descriptor", "refused", frame([raw(t)], window_desc=W1K, single=False, fcs_bytes=8, content_size=1 << 37), cls="SIZE_EXCEEDED")
    add("single segment, content 1000: window 1024", "valid", frame([rle(0x43, 1000)]))
    add("window descriptor 0x00", "valid", frame([raw(t)], window_desc=W1K))
    add("window descriptor with mantissa 3: block of 2816", "valid", frame([rle(0x44, 2816)], window_desc=0x0B))
    add("window descriptor with mantissa 3: block of 2817", "judge", frame([rle(0x44, 2817)], window_desc=0x0B))
    add("window above the decoder's maximum", "refused", frame([raw(t)], window_desc=W1G), cls="WINDOW_EXCEEDED")
    for did in (5, 300, 70000):
        d = DICTS[did]
        add("dictionary id %d" % did, "valid", fd([seqblock([(3, 20, 3 + 40), (2, 5, 3 + len(d))], 1, did)], did))
    add("dictionary id field of one byte, value 0", "judge", frame([raw(t)], dict_id=0, did_bytes=1))
    add("dictionary id 9 is not registered", "refused", frame([raw(t)], dict_id=9), cls="UNKNOWN_DICT")
    add("reserved bit of the frame header", "refused", frame([raw(t)], reserved_bit=1))
    add("content size one too many", "refused", frame([raw(t)], content_size=len(t) + 1))
    add("content size one too few", "refused", frame([raw(t)], content_size=len(t) - 1))
    add("checksum right", "valid", frame([raw(t), seqblock([(4, 9, 3 + 2)], 0)], checksum=True, xxh64=_xxh64))
    add("checksum wrong", "refused", frame([raw(t)], checksum=True, checksum_value=(_xxh64(t) & 0xFFFFFFFF) ^ 0x100), cls="CRC")
    f1, p1 = frame([raw(t)], checksum=True, xxh64=_xxh64)
    f2, p2 = frame([seqblock([(6, 30, 3 + 1)], 2, 3)], window_desc=W1K)
    add("two frames around a skippable frame", "valid", (f1 + zb.skippable(b"skip me", 7) + f2 + zb.skippable(b""), p1 + p2))
    add("frame cut short in its last block", "refused", f1[:-6], cls="EOF")
    add("skippable frame cut short", "refused", f1 + zb.skippable(b"abc", size=9), cls="EOF")

    # ---- blocks ---------------------------------------------------------------------------------------------------------------
    section[0] = "blocks"
    add("rle block of 1", "valid", frame([rle(0x61, 1)]))
    add("rle block of 131072", "valid", frame([rle(0x62, BLOCK)]))
    add("rle block of 131073", "refused", frame([rle(0x62, BLOCK + 1)], window_desc=W8M))
    add("raw block of 0, last", "valid", frame([raw(t), raw(b"")]))
    add("raw block of 0, in the middle", "valid", frame([raw(t), raw(b""), rle(0x63, 3)]))
    add("compressed block of the minimum size", "valid", frame([raw(t), comp(b"")]))
    add("compressed block of one byte", "refused", frame([raw(t), comp(b"", body=b"\0")]))
    add("block type 3", "refused", frame([raw(t), Block("reserved", b"abc")]))
    k = rnd(1025, 4)
    add("1 KiB window: raw block of 1024", "valid", frame([raw(k[:1024])], window_desc=W1K))
    add("1 KiB window: raw block of 1025", "refused", frame([raw(k)], window_desc=W1K))
    add("1 KiB window: compressed block regenerates 1024", "valid", frame([seqblock([(500, 500, 3 + 100)], 24)], window_desc=W1K))
    add("1 KiB window: compressed block regenerates 1025", "refused", frame([seqblock([(500, 500, 3 + 100)], 25)], window_desc=W1K))
    add("1 KiB window: literals regenerate 1025", "refused", frame([comp(Lits("rle", b"z" * 1025))], window_desc=W1K))
    add("8 MiB window: compressed block regenerates 131072", "valid", frame([seqblock([(8, 65539, 3 + 1), (0, 65525, 3 + 5)])], window_desc=W8M))
    add("8 MiB window: compressed block regenerates 131073", "refused", frame([seqblock([(8, 65539, 3 + 1), (0, 65526, 3 + 5)])], window_desc=W8M))

    # ---- literals -------------------------------------------------------------------------------------------------------------
    section[0] = "literals"
    for kind in ("raw", "rle"):
        for sf, limit in ((0, 31), (1, 4095), (3, 4096)):
            for n in (0, 31, 32, 4095, 4096):
                if n <= limit:
                    data = rnd(n, n) if kind == "raw" else b"\x5a" * n
                    add("%s literals, size format %d, %d bytes" % (kind, sf, n), "valid", frame([comp(Lits(kind, data, sf=sf))], window_desc=W8M))
    h5 = rnd(203, 11, 5)   # symbols 0..4: four explicit weights
    h6 = rnd(203, 12, 6)   # symbols 0..5: five explicit weights
    for sf in (0, 1, 2, 3):
        add("huffman literals, size format %d" % sf, "valid", frame([comp(Lits("huf", h5, sf=sf), [(200, 5, 3 + 9)])]))
    for n in (41, 42, 43):
        add("four streams, %d literals" % n, "valid", frame([comp(Lits("huf", h5[:n], sf=1))]))
    add("four streams, 6 literals: the last stream holds no symbol", "judge", frame([comp(Lits("huf", h5[:6], sf=1))]))
    add("direct weights, even count", "valid", frame([comp(Lits("huf", h5, sf=0))]))
    add("direct weights, odd count", "valid", frame([comp(Lits("huf", h6, sf=0))]))
    a20 = bytes(97 + b for b in rnd(300, 13, 20))  # 20 letters: weights 0 (97 times), 1 and 2 -> an FSE alphabet of three symbols
    for log in (5, 6, 7):
        add("fse weights, table log %d" % log, "valid", frame([comp(Lits("huf", a20, sf=1, wcoding=("fse", log)))]))
    for log in (8, 9, 12, 15):  # the format stops at 6; the reference's fse package reads up to 15
        add("fse weights, table log %d" % log, "judge", frame([comp(Lits("huf", a20, sf=1, wcoding=("fse", log)))]))
    add("fse weights, table log 15, then treeless and a match", "judge",
        frame([comp(Lits("huf", a20, sf=1, wcoding=("fse", 15)), [(250, 30, 3 + 100)]), comp(Lits("treeless", a20[:77], sf=0), [(70, 9, 3 + 3)])]))
    add("fse weights, description of 3 bytes", "judge", frame([comp(Lits("huf", h5, sf=0, weights=[2, 1, 1, 2, 2], wcoding=("fse", 5), tree_kw={"cut": 3}))]))
    add("fse weights, whole description 5 bytes", "judge", frame([comp(Lits("huf", bytes([0, 1, 2] * 9), sf=0, weights=[2, 1, 1], wcoding=("fse", 5, [0, 16, 16])))]))
    add("fse weights, whole description 4 bytes", "judge", frame([comp(Lits("huf", bytes([1, 2] * 9), sf=0, weights=[0, 1, 1], wcoding=("fse", 5, [16, 16])))]))
    add("fse weights, description of 2 bytes and a stream of 1", "judge",
        frame([comp(Lits("huf", bytes([1, 2] * 9), sf=0, weights=[0, 1, 1], tree=b"\x03" + zb.fse_description([16, 16], 5) + b"\xd5"))]))
    far = [10, 10, 10] + [0] * 67 + [-1, -1]  # weights 70 and 71 have a cell each and are never coded: a zero run of 3, 3, ... flags
    add("fse weights, a table with unused symbols 70 and 71", "judge", frame([comp(Lits("huf", a20, sf=1, wcoding=("fse", 5, far)))]))
    add("fse weights, table log 15 and one count of 32768", "judge",
        frame([comp(Lits("huf", bytes([1, 2] * 9), sf=0, weights=[0, 1, 1], tree=b"\x07" + zb.fse_description([0, 32768], 15) + b"\x01\x80"))]))
    add("two symbols, weights 1 and 1", "valid", frame([comp(Lits("huf", rnd(50, 14, 2), sf=0))]))
    w255 = [2, 2, 0, 0] + [1] * 252
    d255 = bytes([255, 0, 1, 4, 254]) + bytes(b for b in rnd(120, 15) if b not in (2, 3)) + b"\xff"
    add("symbol 255 in use, 255 weights", "valid", frame([comp(Lits("huf", d255, sf=0, weights=w255, wcoding=("fse", 6)))]))
    w11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    add("code of 11 bits, table log 11", "valid", frame([comp(Lits("huf", bytes(range(12)) * 3 + rnd(60, 16, 12), sf=0, weights=w11))]))
    add("weights sum to table log 12", "refused", frame([comp(Lits("huf", rnd(40, 17, 4), sf=0, weights=[11, 11, 11, 11]))]))
    add("a weight of 12", "refused", frame([comp(Lits("huf", rnd(40, 18, 2), sf=0, weights=[12, 12]))]))
    two = [comp(Lits("huf", h5, sf=1)), comp(Lits("treeless", h5[50:150], sf=0))]
    add("treeless right after a huffman block", "valid", frame(two))
    add("treeless after a block with raw literals", "valid", frame([two[0], comp(rnd(9, 19)), comp(Lits("treeless", h5[20:190], sf=1))]))
    for sf in (2, 3):
        add("treeless, size format %d" % sf, "valid", frame([two[0], comp(Lits("treeless", h5[3:160], sf=sf), [(100, 9, 3 + 5)])]))
    add("treeless in the first block", "refused", frame([comp(Lits("treeless", h5, sf=1, assume_weights=zb.flat_weights(h5)))]))
    s0 = zb.huf_stream(h5, zb.huf_codes(zb.flat_weights(h5))[1])
    add("huffman stream with a last byte of 0", "refused", frame([comp(Lits("huf", h5, sf=0, streams=[s0 + b"\0"]))]))
    add("huffman stream that leaves 8 bits unread", "refused", frame([comp(Lits("huf", h5, sf=0, stream_kw={"pad_bits": 8}))]))
    add("huffman stream one symbol short", "refused", frame([comp(Lits("huf", h5, sf=0, regen=len(h5) + 1))]))

    # ---- sequence section -----------------------------------------------------------------------------------------------------
    section[0] = "sequences"
    for n in (1, 63, 64, 65, 127, 128, 129, 0x7EFF, 0x7F00, 0x7F00 + 5):
        seqs = [(8, 3, 3 + 5)] + [(0, 3, 3 + 1 + (i * 7) % 8) for i in range(1, n)]
        add("nSeq %d" % n, "valid", frame([seqblock(seqs, n & 1, n)], window_desc=W8M))
    varied = [(i % 5, 3 + (i * 3) % 7, 3 + 1 + i % 6) for i in range(40)]
    varied[0] = (9, 4, 3 + 7)
    same = [(2, 4, 3 + 2)] * 5
    add("all tables predefined", "valid", frame([seqblock(varied, 3)]))
    add("all tables rle", "valid", frame([seqblock(same, 0)]))
    add("all tables fse", "valid", frame([seqblock(varied, 3, modes={"ll": (FSE, 5), "of": (FSE, 5), "ml": (FSE, 5)})]))
    for kind in ("ll", "of", "ml"):
        add("%s rle, the others predefined" % kind, "valid", frame([seqblock(same, 1, modes={kind: RLE})]))
        add("%s fse, the others predefined" % kind, "valid", frame([seqblock(varied, 1, modes={kind: (FSE, 6)})]))
        add("%s repeats an fse table" % kind, "valid", frame([seqblock(varied, 1, modes={kind: (FSE, 6)}), seqblock(varied[:17], 2, 8, modes={kind: REPEAT})]))
        add("%s repeat in the first block" % kind, "refused", frame([seqblock(varied, 1, modes={kind: REPEAT})]))
    rep3 = {"ll": REPEAT, "of": REPEAT, "ml": REPEAT}
    add("repeat after rle", "valid", frame([seqblock(same, 0, modes={"ll": RLE, "of": RLE, "ml": RLE}), seqblock(same[:3], 1, 9, modes=rep3)]))
    add("repeat after predefined", "valid", frame([seqblock(varied, 0), seqblock(varied[:11], 1, 9, modes=rep3)]))
    add("repeat after fse, across a raw block", "valid", frame([seqblock(varied, 0, modes={"ll": (FSE, 6), "of": (FSE, 5), "ml": (FSE, 7)}), raw(t), seqblock(varied[:9], 1, 9, modes=rep3)]))
    add("fse tables at logs 9, 8, 9", "valid", frame([seqblock(varied, 2, modes={"ll": (FSE, 9), "of": (FSE, 8), "ml": (FSE, 9)})]))
    for kind, log in (("ll", 10), ("of", 9), ("of", 10), ("ml", 10)):
        add("%s fse table log %d" % (kind, log), "refused" if kind != "of" else "judge", frame([seqblock(varied, 2, modes={kind: (FSE, log)})]))
    low = [(i % 4, 3, 3 + 3) for i in range(30)]
    low[0] = (3, 3, 3 + 3)
    add("ll table with -1 counts", "valid", frame([seqblock(low, 0, modes={"ll": (FSE, 5, [16, 14, -1, -1])})]))
    add("of table with -1 counts and a zero run", "valid", frame([rle(0x20, 5000), seqblock(varied, 0, modes={"of": (FSE, 5, [0, 0, 22, 8, -1, 0, 0, 0, 0, 0, 0, 0, -1])}),
                                                              seqblock([(8, 3, 3 + 4093)], 0, 5, modes={"of": REPEAT})]))
    short = [(3, i, 3 + 2) for i in (3, 4, 4, 3)]
    add("ml description with 3 bytes behind it", "judge", frame([seqblock(short[:1], 0, modes={"ll": RLE, "of": RLE, "ml": (FSE, 5, [16, 16])})]))
    add("ml description with 4 bytes behind it", "judge", frame([seqblock(short, 0, modes={"ll": RLE, "of": RLE, "ml": (FSE, 5, [16, 16])})]))
    add("reserved bits of the mode byte", "refused", frame([seqblock(varied, 1, mode_reserved=1)]))
    add("ll codes 0 to 25 at both ends of their extra bits", "valid",
        frame([raw(t), seqblock([(n, 3, 3 + 1) for n in (0, 15, 16, 17, 48, 63, 64, 127)], 0)]))
    add("ll code 35, least and greatest that fit a block", "valid",
        frame([raw(t), comp(Lits("rle", b"q" * 65536), [(65536, 3, 3 + 2)]), comp(Lits("rle", b"r" * (BLOCK - 3)), [(BLOCK - 3, 3, 3 + 2)])], window_desc=W8M))
    add("ll code 35, one more than fits a block", "refused", frame([raw(t), comp(Lits("rle", b"r" * (BLOCK - 2)), [(BLOCK - 2, 3, 3 + 2)])], window_desc=W8M))
    add("ml codes 0 to 43 at both ends of their extra bits", "valid", frame([seqblock([(1, n, 3 + 1) for n in (3, 34, 35, 36, 99, 130, 131, 258)], 0)]))
    add("ml code 52, least and greatest that fit a block", "valid",
        frame([raw(t), seqblock([(1, 65539, 3 + 3)], 1), seqblock([(1, BLOCK - 1, 3 + 30)], 0)], window_desc=W8M))
    add("ml code 52, one more than fits a block", "refused", frame([raw(t), seqblock([(1, BLOCK, 3 + 30)], 0)], window_desc=W8M))
    add("of code 31", "refused", frame([raw(t), seqblock([(1, 3, 3 + 4)], 0, modes={"of": (RLE, 31)}, of_codes=[31])]))

    # ---- offsets and repeat codes ---------------------------------------------------------------------------------------------
    section[0] = "offsets"
    reps = [(10, 4, 3 + 7), (2, 3, 1), (2, 3, 2), (2, 3, 3), (0, 3, 1), (0, 3, 2), (0, 3, 3), (3, 5, 2), (0, 4, 3), (1, 3, 3)]
    add("repeat codes 1, 2, 3 with and without literals", "valid", frame([seqblock(reps, 2)]))
    add("repeat 1 minus one byte while repeat 1 is 1", "judge", frame([seqblock([(5, 3, 3 + 1), (0, 3, 3)], 1)], window_desc=W1K))
    start = [(1, 3, 1), (1, 3, 2), (1, 3, 3)]
    add("start values 1, 4, 8 behind a raw block", "valid", frame([raw(t), seqblock(start, 0)]))
    add("start values 1, 4, 8 behind a dictionary", "valid", fd([seqblock(start, 0)], 5))
    add("start value 8 without history", "refused", frame([seqblock([(7, 3, 3)], 0)]))
    setrep = seqblock([(9, 4, 3 + 7), (1, 3, 3 + 12)], 1)
    userep = seqblock([(2, 5, 2), (3, 4, 1), (0, 3, 2)], 1, 8)
    add("repeat history across a raw block", "valid", frame([setrep, raw(t), userep]))
    add("repeat history across an rle block", "valid", frame([setrep, rle(0x55, 50), userep]))
    add("offset codes 2 to 17 in one block", "valid",
        frame([rle(0x30, BLOCK), raw(rnd(300, 21)), rle(0x31, BLOCK), seqblock([(1, 4, 1 << c) for c in range(2, 18)] + [(0, 5, (1 << 18) - 1)], 1)], window_desc=W8M))
    add("offset code 20", "valid", frame([rle(0x32 + i, BLOCK) for i in range(8)] + [seqblock([(0, 40, (1 << 20) + 3)], 1)], window_desc=W8M))
    # 33 MiB of history whose first 128 KiB change every 1 KiB, so that a wrong bit of the offset's upper part shows in the bytes copied
    far_hist = [raw(b"first")] + [rle(i, 1024) for i in range(128)] + [rle(i & 255, BLOCK) for i in range(256)]
    add("offset code 25", "valid", frame(far_hist + [seqblock([(2, 9, (1 << 25) + 100003), (1, 5, (1 << 25) + 70003), (0, 4, (1 << 25) + 3)], 1)], window_desc=W64M), big=True)
    add("offset equal to all history", "valid", frame([raw(t), seqblock([(5, 6, 3 + len(t) + 5)], 0)]))
    add("offset one beyond all history", "refused", frame([raw(t), seqblock([(5, 6, 3 + len(t) + 6)], 0)]))
    add("offset equal to dictionary and history", "valid", fd([raw(t), seqblock([(5, 6, 3 + 300 + len(t) + 5)], 0)], 5))
    add("offset one beyond dictionary and history", "refused", fd([raw(t), seqblock([(5, 6, 3 + 300 + len(t) + 6)], 0)], 5))
    two_k = [raw(k[:1024]), raw(k[:1024][::-1])]
    add("1 KiB window, 2 KiB produced: offset 1024", "valid", frame(two_k + [seqblock([(1, 8, 3 + 1024)], 0)], window_desc=W1K))
    add("1 KiB window, 2 KiB produced: offset 1025", "refused", frame(two_k + [seqblock([(1, 8, 3 + 1025)], 0)], window_desc=W1K))
    add("1 KiB window: offset into the dictionary beyond the window", "judge", fd([raw(k[:1024]), seqblock([(1, 8, 3 + 1100)], 0)], 5, window_desc=W1K))

    # ---- the 64-sequence group executor ---------------------------------------------------------------------------------------
    section[0] = "group"
    add("ll and ml of 32 and 33", "valid", frame([raw(rnd(100, 22)), seqblock([(32, 32, 3 + 90), (33, 33, 3 + 95), (32, 33, 3 + 200), (33, 32, 3 + 64), (31, 31, 3 + 33)], 3)]))
    over = [(70, 300, 3 + 1), (1, 299, 3 + 2), (2, 100, 3 + 3), (64, 300, 3 + 63), (3, 65, 3 + 64), (0, 300, 3 + 65), (1, 33, 3 + 32), (1, 34, 3 + 33), (0, 64, 3 + 1), (0, 65, 3 + 2)]
    add("overlapping matches", "valid", frame([seqblock(over, 1)]))
    filler = [(1, 3, 3 + 1 + i % 9) for i in range(64)]
    filler[0] = (12, 3, 3 + 4)
    for name, off in (("ends at the group's first byte", 12), ("ends one byte into the group", 11), ("ends at the group's last literal", 8), ("starts in the group", 3)):
        add("second group: a match whose source %s" % name, "valid", frame([seqblock(filler + [(4, 8, 3 + off), (2, 40, 3 + 50)], 1)]))
        add("first group behind a raw block: a match whose source %s" % name, "valid", frame([raw(t), seqblock([(4, 8, 3 + off), (2, 40, 3 + 30)], 1)]))
    r100 = rnd(100, 25)
    for ml in (5, 32, 33, 40):  # the copy by the sequence's own lane up to 32 bytes, by the whole wave above
        for name, end in (("ends at the group's first byte", 0), ("ends one byte into the group", 1)):
            for ll in (4, 40):  # the literals in front of it by their own lane, or by the whole wave in a later step
                two = [(ll, 8, 3 + 12), (2, ml, 3 + ll + 10 + ml - end), (1, 3, 3 + 2)]
                add("first group: %d literals, then a match of %d whose source %s" % (ll, ml, name), "valid", frame([raw(r100), seqblock(two, 1)]))
                add("second group: %d literals, then a match of %d whose source %s" % (ll, ml, name), "valid", frame([raw(r100), seqblock(filler + two, 1)]))
    add("matches that copy from earlier sequences of the group", "valid",
        frame([seqblock([(20, 10, 3 + 15), (0, 12, 3 + 10), (1, 40, 3 + 22), (0, 35, 3 + 75), (5, 100, 3 + 5), (0, 50, 3 + 100)], 4)]))
    for name, seq in (("short", (10, 12, 3 + 15)), ("short, source ends at the first byte", (10, 5, 3 + 15)), ("long", (40, 60, 3 + 70)), ("long, 300 bytes", (10, 300, 3 + 305)),
                      ("overlapping", (10, 100, 3 + 20)), ("overlapping, offset 11", (10, 40, 3 + 11)), ("the whole dictionary", (0, 300, 3 + 300))):
        add("a match from the dictionary into the output: %s" % name, "valid", fd([seqblock([seq, (1, 4, 3 + 2)], 1)], 5))
    add("a match from the dictionary in the second group", "valid", fd([seqblock(filler + [(4, 90, 3 + 215 + 70)], 1)], 5))
    add("literals overrun by one byte", "refused", frame([comp(rnd(20, 23), [(10, 4, 3 + 3), (11, 3, 3 + 1)])]))
    add("literals overrun by one byte in the second group", "refused", frame([comp(rnd(12 + 63 + 3, 24), filler + [(4, 3, 3 + 1)])]))
    add("no trailing literals", "valid", frame([seqblock([(10, 4, 3 + 3), (10, 3, 3 + 1)], 0)]))
    add("one trailing literal", "valid", frame([seqblock([(10, 4, 3 + 3), (10, 3, 3 + 1)], 1)]))
    return out


# ---- the judge and the emulator's runner ---------------------------------------------------------------------------------------
def dict_args(c):
    """Keyword arguments of oracle_goref.zstd_decode_all for a case's dictionary."""
    return {"dict_id": c.dicts[0], "dict_content": DICTS[c.dicts[0]]} if c.dicts else {}


_ref = {}


def reference(G, c):
    """The reference's DecodeAll on a case: (bytes, None) or (None, message).  Computed once per case and left unchanged."""
    if c.name not in _ref:
        cap = (len(c.plain) if c.plain is not None else 1 << 20) + 64
        try:
            _ref[c.name] = (G.zstd_decode_all(c.data, cap, **dict_args(c)), None)
        except ValueError as e:
            _ref[c.name] = (None, str(e))
    return _ref[c.name]


def message_class(msg):
    """The status class of one of the reference's error messages, for the directed refusals."""
    for text, cls in (("window size exceeded", "WINDOW_EXCEEDED"), ("decompressed size exceeds", "SIZE_EXCEEDED"), ("CRC check failed", "CRC"),
                      ("unknown dictionary", "UNKNOWN_DICT"), ("unexpected EOF", "EOF"), ("magic number mismatch", "MAGIC")):
        if text in msg:
            return cls
    return "CORRUPT"


def judge(cs, refs, outs, status):
    """The lines of what is wrong: where the reference returns bytes the status is 0 and the bytes are equal; where it refuses the
    status is non-zero, of the class of the reference's message, and the range is empty; a valid case's bytes are the builder's, a refused case is refused by the reference."""
    wrong = []
    for c, (ref, err), o, s in zip(cs, refs, outs, status):
        s = int(s)
        if c.expect == "valid" and ref != c.plain:
            wrong.append("%s: the builder and the reference disagree (%s)" % (c.name, err))
        if c.expect == "refused" and ref is not None:
            wrong.append("%s: the reference accepts it" % c.name)
        if ref is not None:
            if s != 0 or o != ref:
                wrong.append("%s: reference returns %d bytes, device status %s with %d bytes%s" % (c.name, len(ref), NAMES.get(s, s), len(o), "" if len(o) != len(ref) else
                             ", first difference at %d" % next((i for i in range(len(o)) if o[i] != ref[i]), -1)))
        elif s == 0 or o != b"":
            wrong.append("%s: reference refuses (%s), device status %s with %d bytes" % (c.name, err, NAMES.get(s, s), len(o)))
        elif NAMES.get(s) != message_class(err):
            wrong.append("%s: reference refuses (%s), class %s, device status %s" % (c.name, err, message_class(err), NAMES.get(s, s)))
    return wrong


def raw_dict_blob(did, content):
    """A raw dictionary as the emulator's entry point takes it."""
    return b"KCRD" + did.to_bytes(4, "little") + content


def emu_decode_all(inputs, cap, dicts=(), max_memory=64 << 30, max_window=1 << 29, ignore_checksum=False):
    """(list of bytes, status[n]) of kcemu_zstd_decode_all (plan, decode, XXH64, verdict and compaction as one batch); the GUARD bytes
    around dst are checked.  dicts: full-format dictionaries, or raw ones wrapped by raw_dict_blob."""
    import emu_lib
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
    dst = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    r = L.kcemu_zstd_decode_all(src.ctypes.data, off.ctypes.data, n, max_memory, max_window, int(ignore_checksum), dblob.ctypes.data, doff.ctypes.data,
                                len(dicts), dst.ctypes.data + GUARD, cap, out_off.ctypes.data, status.ctypes.data)
    assert r == 0, r
    assert np.all(dst[:GUARD] == 0xA5) and np.all(dst[GUARD + cap:] == 0xA5), "written outside dst"
    body = dst[GUARD:GUARD + cap]
    return [body[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)], status


def full():
    return os.environ.get("KC_TEST_FULL", "") == "1"
