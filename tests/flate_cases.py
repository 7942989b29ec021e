"""Inputs of the inflate tests, shared by the emulator suite (test_emu_flate.py) and the GPU suite (test_gpu_flate.py): hand-built
DEFLATE and gzip streams at the smallest shapes at which the device code can go wrong, streams zlib writes, and seeded mutations.
Every case is judged by tests/flate_model.py; nothing here knows what the device answers.

A case is a Case(name, fmt, data, dict, multistream); cases() lists the directed ones, mutations() the 2 x 480 mutated ones,
sized(text, noise) the large ones.  verdict(case) is the model's (bytes, class, consumed), computed once per case.

Not covered: ISIZE wrapping at 4 GiB (a member that large is above this library's 1 GiB limit per input)."""
import collections
import random
import struct
import zlib

import flate_model as M

Case = collections.namedtuple("Case", "name fmt data dict multistream")
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def C(name, data, fmt="flate", dict=b"", multistream=True):
    return Case(name, fmt, bytes(data), bytes(dict), multistream)


_verdicts = {}


def verdict(c):
    k = (c.fmt, c.data, c.dict, c.multistream)
    if k not in _verdicts:
        _verdicts[k] = M.gunzip(c.data, c.multistream) if c.fmt == "gzip" else M.inflate(c.data, c.dict)
    return _verdicts[k]


class BW:
    """DEFLATE's bit order: fields LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, cl):
        c, n = cl
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)
        return self

    def raw(self, b):
        assert self.n == 0
        self.out += b
        return self

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canon(lens):
    """symbol -> (code, length) of the canonical code over lens (also for sets that are not complete)."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for i in range(1, 16):
        code = (code + count[i - 1]) << 1
        nxt[i] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


FIXED = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]


def put_len(bw, lit, length, sym=None):
    if sym is None:
        sym = max(i for i in range(29) if _LBASE[i] <= length and (i != 28 or length == 258)) + 257
    bw.code(lit[sym])
    i = sym - 257
    bw.put(length - _LBASE[i], _LEXTRA[i])


def put_dist(bw, dcode, dist):
    """dcode None: a fixed block's five bits."""
    i = max(k for k in range(30) if _DBASE[k] <= dist)
    if dcode is None:
        bw.code((i, 5))
    else:
        bw.code(dcode[i])
    bw.put(dist - _DBASE[i], _DEXTRA[i])


def fixed_block(bw, items, final=True, eob=True):
    """items: ints (literals), (length, dist) or (length, dist, length symbol) matches, or ("sym", s) / ("dsym", d) raw symbols."""
    bw.put(1 if final else 0, 1).put(1, 2)
    for it in items:
        if isinstance(it, int):
            bw.code(FIXED[it])
        elif it[0] == "sym":
            bw.code(FIXED[it[1]])
        elif it[0] == "dsym":
            bw.code((it[1], 5))
        else:
            put_len(bw, FIXED, it[0], it[2] if len(it) > 2 else None)
            put_dist(bw, None, it[1])
    if eob:
        bw.code(FIXED[256])
    return bw


def stored_block(bw, data, final=True, nlen=None):
    bw.put(1 if final else 0, 1).put(0, 2).align()
    bw.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
    bw.raw(data)
    return bw


def dyn_header(bw, lit_lens, dist_lens, final=True, cl_lens=None, cl_syms=None, hlit=None, hdist=None, nclen=19):
    """A dynamic block's header.  lit_lens / dist_lens: the code lengths to transmit; cl_syms: the code-length symbols to send, as
    (symbol, extra value) — default one plain symbol per length; cl_lens: the 19 lengths of the code-length code — default 5 bits
    for 0..15 and 16 / 17 / 18 ... a complete code."""
    if cl_syms is None:
        cl_syms = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
    if cl_lens is None:
        cl_lens = [5] * 16 + [3, 3, 2]   # 16/32 + 1/8 + 1/8 + 1/4 = 1
    bw.put(1 if final else 0, 1).put(2, 2)
    bw.put((len(lit_lens) - 257) if hlit is None else hlit, 5)
    bw.put((len(dist_lens) - 1) if hdist is None else hdist, 5)
    bw.put(nclen - 4, 4)
    for i in range(nclen):
        bw.put(cl_lens[_ORDER[i]], 3)
    cc = canon(cl_lens)
    for s, extra in cl_syms:
        bw.code(cc[s])
        if s >= 16:
            bw.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return bw


def lit_lens_with(used, n=257):
    """Literal/length code lengths: a complete code over the symbols `used` (a power of two of them, equal lengths)."""
    k = len(used)
    assert k & (k - 1) == 0 and k >= 2
    lens = [0] * n
    for s in used:
        lens[s] = k.bit_length() - 1
    return lens


def _stored():
    out = [C("stored/empty-final", stored_block(BW(), b"").bytes()),
           C("stored/1", stored_block(BW(), b"Z").bytes()),
           C("stored/65535", stored_block(BW(), bytes(i * 7 & 255 for i in range(65535))).bytes()),
           C("stored/len-nlen-mismatch", stored_block(BW(), b"abc", nlen=0x1234).bytes())]
    for j in range(8):  # 13 + 9 j bits in front of the length field: every count of bits to discard
        bw = fixed_block(BW(), [200] * j, final=False)
        out.append(C("stored/discard-%d" % ((-(13 + 9 * j)) % 8), stored_block(bw, b"stored after %d" % j).bytes()))
    full = stored_block(BW(), b"0123456789").bytes()
    out += [C("stored/cut-in-length", full[:3]), C("stored/cut-in-nlen", full[:4]), C("stored/cut-in-data", full[:9]), C("stored/cut-no-data", full[:5])]
    return out


def _fixed():
    lits = [ord(c) for c in "abcdefgh"]
    out = [C("fixed/eob-only", fixed_block(BW(), []).bytes()),
           C("fixed/one-literal", fixed_block(BW(), [65]).bytes()),
           C("fixed/len3", fixed_block(BW(), lits + [(3, 8)]).bytes()),
           C("fixed/len258-sym285", fixed_block(BW(), lits + [(258, 8)]).bytes()),
           C("fixed/len258-sym284+31", fixed_block(BW(), lits + [(258, 8, 284)]).bytes()),
           C("fixed/dist1-len258", fixed_block(BW(), [120, (258, 1)]).bytes()),
           C("fixed/dist-produced+1", fixed_block(BW(), lits + [(3, 9)]).bytes()),
           C("fixed/dist-at-0", fixed_block(BW(), [(3, 1)]).bytes())]
    for d in (30, 31):
        bw = BW()
        bw.put(1, 1).put(1, 2)
        for x in lits:
            bw.code(FIXED[x])
        bw.code(FIXED[257]).code((d, 5)).code(FIXED[256])
        out.append(C("fixed/dist-code-%d" % d, bw.bytes()))
    for s in (286, 287):
        out.append(C("fixed/len-sym-%d" % s, fixed_block(BW(), lits + [("sym", s), ("dsym", 0)]).bytes()))
    body = bytes((i * i + (i >> 3)) & 255 for i in range(32768))
    bw = stored_block(BW(), body, final=False)
    out.append(C("fixed/dist32768-at-32768", fixed_block(bw, [(3, 32768)]).bytes()))
    bw = stored_block(BW(), body[:32767], final=False)
    out.append(C("fixed/dist32768-at-32767", fixed_block(bw, [(3, 32768)]).bytes()))
    full = fixed_block(BW(), lits + [(258, 8, 284), (100, 3000)]).bytes()
    out += [C("fixed/cut-%d" % k, full[:k]) for k in range(len(full))]  # every truncation: in a code, in extra bits (R3), in the distance
    return out


def _dynamic():
    out = []
    # lengths 1 .. 15 (and a second 15): codes on both sides of the primary table's width and at the limit
    syms = list(range(97, 111)) + [256, 111]   # 97..110 get lengths 1..14, the end-of-block symbol and 111 get 15
    lens = [0] * 257
    for k, s in enumerate(syms):
        lens[s] = min(k + 1, 15)
    lc = canon(lens)
    for final_first in (True, False):
        bw = dyn_header(BW(), lens, [0], final=final_first)
        for s in syms[:14] + [111] + syms[13::-1]:
            bw.code(lc[s])
        bw.code(lc[256])
        if not final_first:
            fixed_block(bw, [33])
        out.append(C("dynamic/lengths-1-to-15%s" % ("" if final_first else "+fixed"), bw.bytes()))
    # one distance code of length 1: used, and its missing twin used
    l4 = lit_lens_with([97, 98, 256, 257], 258)
    c4 = canon(l4)
    for name, bit in (("single-dist-code", 0), ("single-dist-code-missing-used", 1)):
        bw = dyn_header(BW(), l4, [1])
        bw.code(c4[97]).code(c4[98]).code(c4[257]).put(bit, 1).code(c4[256])
        out.append(C("dynamic/" + name, bw.bytes()))
    # distance codes of 1 .. 15 bits (and a second of 15): both sides of the distance table's primary width, every one used
    dl = [min(k + 1, 15) for k in range(16)]
    dc = canon(dl)
    bw = stored_block(BW(), bytes((i * 11 + 3) & 255 for i in range(300)), final=False)
    dyn_header(bw, l4, dl)
    for k in list(range(16)) + [15, 9, 8, 10]:
        bw.code(c4[257])
        put_dist(bw, dc, _DBASE[k] + (k & 1 if k >= 4 else 0))
    out.append(C("dynamic/dist-lengths-1-to-15", bw.code(c4[256]).bytes()))
    # no distance code at all: literals only stand, a match does not
    bw = dyn_header(BW(), l4, [0])
    bw.code(c4[97]).code(c4[98]).code(c4[256])
    out.append(C("dynamic/empty-dist-literals-only", bw.bytes()))
    bw = dyn_header(BW(), l4, [0])
    bw.code(c4[97]).code(c4[98]).code(c4[257]).put(0, 1).code(c4[256])
    out.append(C("dynamic/empty-dist-match", bw.bytes()))
    # the repeats
    plain = [(n, 0) for n in l4]
    out.append(C("dynamic/repeat16-at-0", dyn_header(BW(), l4, [1], cl_syms=[(16, 0)] + plain[3:] + [(1, 0)]).code(c4[256]).bytes()))
    # 258 lengths + 2 distance lengths: "2" for symbol 257 repeated across the boundary gives distance lengths 2, 2 ... four of them is complete
    l5 = list(l4)
    span = [(n, 0) for n in l5] + [(16, 1)]   # 4 more copies of the last length (2): the four distance codes
    bw = dyn_header(BW(), l5, [2] * 4, cl_syms=span)
    bw.code(c4[97]).code(c4[98]).code(c4[257]).code((1, 2)).code(c4[256])
    out.append(C("dynamic/repeat-across-hlit-hdist", bw.bytes()))
    out.append(C("dynamic/repeat-past-n", dyn_header(BW(), l5, [2] * 4, cl_syms=[(n, 0) for n in l5] + [(16, 2)]).code(c4[256]).bytes()))
    out.append(C("dynamic/repeat18-past-n", dyn_header(BW(), l5, [2] * 4, cl_syms=[(n, 0) for n in l5[:200]] + [(18, 127)]).bytes()))
    for h in (30, 31):
        out.append(C("dynamic/hlit-%d" % (257 + h), dyn_header(BW(), l4, [1], hlit=h).put(0, 64).bytes()))
        out.append(C("dynamic/hdist-%d" % (1 + h), dyn_header(BW(), l4, [1], hdist=h).put(0, 64).bytes()))
    # over-subscribed and incomplete sets in each table
    over_cl, inc_cl = [5] * 16 + [3, 3, 1], [5] * 16 + [3, 3, 3]
    for name, cl in (("oversubscribed-clen", over_cl), ("incomplete-clen", inc_cl)):
        bw = BW()
        bw.put(1, 1).put(2, 2).put(1, 5).put(0, 5).put(15, 4)
        for i in range(19):
            bw.put(cl[_ORDER[i]], 3)
        out.append(C("dynamic/" + name, bw.put(0, 64).bytes()))
    l3 = [0] * 258
    l3[97], l3[98], l3[256] = 1, 1, 1
    out.append(C("dynamic/oversubscribed-lit", dyn_header(BW(), l3, [1]).put(0, 32).bytes()))
    l3 = [0] * 258
    l3[97], l3[256] = 2, 2
    out.append(C("dynamic/incomplete-lit", dyn_header(BW(), l3, [1]).put(0, 32).bytes()))
    l3 = [0] * 258
    l3[256] = 1
    out.append(C("dynamic/single-lit-code-eob", dyn_header(BW(), l3, [1]).put(0, 1).bytes()))
    out.append(C("dynamic/single-lit-code-missing-used", dyn_header(BW(), l3, [1]).put(1, 1).bytes()))
    out.append(C("dynamic/oversubscribed-dist", dyn_header(BW(), l4, [1, 1, 1]).code(c4[256]).bytes()))
    out.append(C("dynamic/incomplete-dist", dyn_header(BW(), l4, [2, 2]).code(c4[256]).bytes()))
    out.append(C("dynamic/no-eob-code", dyn_header(BW(), lit_lens_with([97, 98, 99, 100]), [1]).put(0x1B, 8).bytes()))  # R1: runs into the end
    out.append(C("block-type-3", BW().put(1, 1).put(3, 2).put(0, 13).bytes()))
    full = out[0].data
    out += [C("dynamic/cut-%d" % k, full[:k]) for k in range(0, len(full), 3)]
    return out


def _multi():
    a = bytes(range(64, 128))
    bw = fixed_block(BW(), list(a), final=False)
    stored_block(bw, b"-- stored in the middle --", final=False)
    three = fixed_block(bw, [(40, 64 + 26), 33]).bytes()
    nonfinal = fixed_block(BW(), list(b"never ends"), final=False).bytes()
    bw = fixed_block(BW(), list(b"fixed one "), final=False)   # the fixed code outlives the dynamic block between its two uses
    l4 = lit_lens_with([97, 98, 256, 257], 258)
    c4 = canon(l4)
    dyn_header(bw, l4, [1], final=False).code(c4[97]).code(c4[98]).code(c4[256])
    fdf = fixed_block(bw, list(b" fixed two") + [(10, 12)]).bytes()
    return [C("multi/fixed-dynamic-fixed", fdf),
            C("multi/three-blocks-match-into-first", three),
            C("multi/non-final-last", nonfinal),
            C("multi/trailing-bytes", three + b"behind the final block"),
            C("multi/empty-input", b"")]


def _granules():
    out = []
    for dist in range(1, 18):
        for length in range(3, 19):
            out.append(C("granule/d%d-l%d" % (dist, length), fixed_block(BW(), list(range(48, 48 + 17)) + [(length, dist), 46]).bytes()))
    for run in range(1, 131):
        out.append(C("granule/run%d" % run, fixed_block(BW(), [(i * 5 + run) & 127 for i in range(run)] + [(5, run), 10] + [66] * (run // 3)).bytes()))
    return out


def _dictionary():
    d = bytes((i * 13 + 5) & 255 for i in range(40000))   # longer than the window: its last 32 KiB count
    return [C("dict/match-at-0", fixed_block(BW(), [(258, 7), 65, (20, 270)]).bytes(), dict=b"dictionary tail"),
            C("dict/match-at-0-window-edge", fixed_block(BW(), [(10, 32768), 65, (5, 32768)]).bytes(), dict=d),
            C("dict/beyond-dict", fixed_block(BW(), [65, (3, 17)]).bytes(), dict=b"dictionary tail"),
            C("dict/zlib", _deflate(b"a preset dictionary pays for short inputs " * 3, 9, zdict=b"dictionary pays preset inputs short"), dict=b"dictionary pays preset inputs short")]


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    kw = {"zdict": zdict} if zdict else {}
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, **kw)
    return c.compress(data) + c.flush()


def gz_member(payload, flg=0, extra=b"xtra", name=b"name.txt", comment=b"a comment", bad_hcrc=False, deflated=None, crc=None, isize=None):
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", 1234567890) + b"\x00\x03")
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) ^ (0x0100 if bad_hcrc else 0))
    body = _deflate(payload) if deflated is None else deflated
    return bytes(h) + body + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, (len(payload) & 0xFFFFFFFF) if isize is None else isize)


def _gzip():
    G = lambda name, data, **kw: C("gzip/" + name, data, fmt="gzip", **kw)  # noqa: E731
    hello, world = gz_member(b"hello, "), gz_member(b"world" * 100, flg=8)
    out = [G("minimal", gz_member(b"", deflated=b"\x03\x00")), G("empty-input", b"")]
    for f in range(16):
        flg = (f & 1) * 4 | (f >> 1 & 1) * 8 | (f >> 2 & 1) * 16 | (f >> 3 & 1) * 2
        out.append(G("flg-%02x" % flg, gz_member(b"flags %d" % flg, flg=flg)))
        if flg & 2:
            out.append(G("flg-%02x-bad-hcrc" % flg, gz_member(b"flags %d" % flg, flg=flg, bad_hcrc=True)))
    out += [G("reserved-flg-%02x" % b, gz_member(b"x", flg=b)) for b in (0x20, 0x40, 0x80)]
    out += [G("wrong-magic", b"\x1f\x8c" + hello[2:]), G("wrong-method", hello[:2] + b"\x07" + hello[3:]),
            G("unterminated-name", gz_member(b"x", flg=8)[:14]), G("name-512", gz_member(b"x", flg=8, name=b"n" * 512)),
            G("name-511", gz_member(b"x", flg=8, name=b"n" * 511)),
            G("cut-in-extra", gz_member(b"x", flg=4)[:13]), G("cut-in-hcrc", gz_member(b"x", flg=2)[:11]),
            G("bad-crc32", gz_member(b"hello", crc=0x12345678)), G("bad-isize", gz_member(b"hello", isize=6)),
            G("two-members", hello + world), G("two-members-second-bad-crc", hello + gz_member(b"world", crc=1)),
            G("two-members-first-bad-crc-second-bad-header", gz_member(b"hello", crc=1) + b"\x1f\x8b\x09" + b"\0" * 20),
            G("second-member-corrupt", hello + world[:30] + b"\xff\xff" + world[32:]),
            G("second-member-unterminated-name", hello + gz_member(b"x", flg=8)[:14]),   # R5: the file ends there
            G("multistream-off-second-behind", hello + world, multistream=False),
            G("multistream-off-junk-behind", hello + b"junk", multistream=False)]
    out += [G("cut-trailer-%d" % k, hello[:len(hello) - k]) for k in range(1, 9)]
    out += [G("junk-%d" % k, hello + b"J" * k) for k in range(1, 12)]
    return out


def cases():
    return _stored() + _fixed() + _dynamic() + _multi() + _granules() + _dictionary() + _gzip()


def bases():
    """The six base streams of the mutations: 0.7 .. 4 KiB each."""
    rng = random.Random(0xF1A7E)
    vocab = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 10))) for _ in range(300)]
    text = b" ".join(rng.choice(vocab) for _ in range(1100))[:6000]
    noise = bytes(rng.randrange(256) for _ in range(1500))
    mixed = (text[:700] + noise[:300]) * 3
    out = [_deflate(text, 1), _deflate(text, 6), _deflate(text[:1800], 6, zlib.Z_FIXED), _deflate(text[:2600], 6, zlib.Z_HUFFMAN_ONLY),
           _deflate(noise, 6), _deflate(mixed, 9)]
    assert all(700 <= len(b) <= 4096 for b in out), [len(b) for b in out]
    return out, [text, text, text[:1800], text[:2600], noise, mixed]


def mutations():
    """480 seeded mutations of the six bases — one random bit, a truncation, one bit in the first 64 bytes, one random byte — and the
    same 480 wrapped as gzip members (header and trailer of the unmutated payload)."""
    rng = random.Random(0xDEF1A7E)
    bs, plain = bases()
    fl, gz = [], []
    for k in range(480):
        i = k % 6
        b = bytearray(bs[i])
        kind = (k // 6) % 4
        if kind == 0:
            p = rng.randrange(len(b) * 8)
            b[p >> 3] ^= 1 << (p & 7)
        elif kind == 1:
            b = b[:rng.randrange(len(b))]
        elif kind == 2:
            p = rng.randrange(64 * 8)
            b[p >> 3] ^= 1 << (p & 7)
        else:
            b[rng.randrange(len(b))] = rng.randrange(256)
        fl.append(C("mut/%d-base%d-kind%d" % (k, i, kind), b))
        gz.append(C("mutgz/%d-base%d-kind%d" % (k, i, kind), gz_member(plain[i], deflated=bytes(b)), fmt="gzip"))
    return fl, gz


def sized(text, noise):
    """text: corpus bytes, noise: random bytes — at zlib levels 1 and 9, and stored."""
    return [C("size/text-level1", _deflate(text, 1)), C("size/text-level9", _deflate(text, 9)), C("size/noise", _deflate(noise, 6)),
            C("size/text-gzip", gz_member(text[:1 << 20], flg=8), fmt="gzip")]


LIMIT = 1 << 30   # decoded bytes per input the library serves (KC_FL_SIZE_EXCEEDED beyond)


def at_the_limit(n_matches, n_literals):
    """One dynamic block of 1 + 258 * n_matches + n_literals bytes in about n_matches / 4 bytes: a literal, then matches of length
    258 at distance 1 — a one-bit length code and the single one-bit distance code, so every match is two zero bits — then literals.
    -> (stream, decoded size).  Too long for the model and the emulator; what it decodes to is arithmetic."""
    lens = [0] * 286
    lens[0], lens[256], lens[285] = 2, 2, 1
    lc = canon(lens)
    bw = dyn_header(BW(), lens, [1]).code(lc[0])
    bw.put(0, 2 * n_matches)
    for _ in range(n_literals):
        bw.code(lc[0])
    return bw.code(lc[256]).bytes(), 1 + 258 * n_matches + n_literals


def batches(cs):
    """cs grouped into batches that share their options: [(fmt, dict, multistream, [cases])]."""
    groups = collections.OrderedDict()
    for c in cs:
        groups.setdefault((c.fmt, c.dict, c.multistream), []).append(c)
    return [(k[0], k[1], k[2], v) for k, v in groups.items()]
