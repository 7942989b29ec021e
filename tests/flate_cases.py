"""Inputs of the inflate tests, shared by the emulator suite (test_emu_flate.py) and the GPU suite (test_gpu_flate.py): hand-built
DEFLATE and gzip streams at the smallest shapes at which the device code can go wrong, streams zlib writes, and seeded mutations.
Every case is judged by tests/flate_model.py; nothing here knows what the device answers.

A case is a Case(name, fmt, data, dict, multistream); cases() lists the directed ones, mutations() the 2 x 480 mutated ones,
generated(seed, n) / generated_gzip(seed, n) seeded structured streams (code-length sets, headers and bodies no encoder writes),
crc_sweep() and copy_sweep() the two device sweeps, sized(text, noise) the large ones.  verdict(case) is what the DEVICE is to answer:
the model's (bytes, class, consumed) with stale_tables=False, computed once per case; reference_verdict(case) the model as the
reference (stale_tables=True, rule R6), which tests/test_ref_flate.py holds against the reference's own code.

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


def verdict(c, stale_tables=False):
    k = (c.fmt, c.data, c.dict, c.multistream, stale_tables)
    if k not in _verdicts:
        if c.fmt == "gzip":
            _verdicts[k] = M.gunzip(c.data, c.multistream, stale_tables=stale_tables)
        else:
            _verdicts[k] = M.inflate(c.data, c.dict, stale_tables=stale_tables)
        _fired[k] = frozenset(M.fired)
    return _verdicts[k]


_fired = {}


def _warm_one(job):
    c, stale = job
    verdict(c, stale)
    k = (c.fmt, c.data, c.dict, c.multistream, stale)
    return _verdicts[k], _fired[k]


def warm(cases, stale_tables=False):
    """The verdicts of many cases, computed in forked children (wall-clock time of the CPU suite only: a process that has opened a GPU
    does not fork, it computes them as they are asked for)."""
    import multiprocessing as mp
    import os
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return
    todo = [c for c in cases if (c.fmt, c.data, c.dict, c.multistream, stale_tables) not in _verdicts]
    procs = min(8, os.cpu_count() or 1, int(os.environ.get("KC_EMU_PROCS", "8")))
    if procs <= 1 or len(todo) < 200:
        return
    with mp.get_context("fork").Pool(procs) as pool:
        for c, (v, f) in zip(todo, pool.map(_warm_one, [(c, stale_tables) for c in todo], chunksize=25)):
            k = (c.fmt, c.data, c.dict, c.multistream, stale_tables)
            _verdicts[k], _fired[k] = v, f


def reference_verdict(c):
    """-> ((bytes, class, consumed), the rules that fired) of the model as the reference."""
    v = verdict(c, True)
    return v, _fired[(c.fmt, c.data, c.dict, c.multistream, True)]


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
        # HLIT, HDIST and HCLEN are read together before either count is checked (inflate.go:466-470): an input that ends inside the
        # fourteen bits is io.ErrUnexpectedEOF whatever the counts say (the model once checked HLIT after its own five bits)
        for k in (1, 2):
            out.append(C("dynamic/hlit-%d-input-ends-at-%d" % (257 + h, k), dyn_header(BW(), l4, [1], hlit=h).bytes()[:k]))
            out.append(C("dynamic/hdist-%d-input-ends-at-%d" % (1 + h, k), dyn_header(BW(), l4, [1], hdist=h).bytes()[:k]))
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
            G("second-member-unterminated-name", hello + gz_member(b"x", flg=8)[:14]),   # R5: the file ends there, read to its end
            G("second-member-unterminated-comment", hello + gz_member(b"x", flg=24)[:22]),
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


# ---- seeded structured streams ----
GEN_SEED = 0x1F1A7E
_GEN_DICT = bytes((i * 131 + (i >> 7) * 17 + 7) & 255 for i in range(40000))
_GEN_DICT_LENS = (1, 257, 32767, 32768, 40000)   # (a few lengths only: a batch shares its dictionary)
PB_L, PB_D, PB_C = 10, 9, 7                      # the device's primary-table widths (KCFL_PB_* of kc_flate_dev.h)


def _split(rng, leaves, cap, exact=None):
    """A Kraft-exact multiset of code lengths, none above cap: random splits of a leaf into two; exact: the longest is exactly that."""
    if exact:
        depths, cap = list(range(1, exact)) + [exact, exact], exact
    else:
        depths = [1, 1]
    while len(depths) < leaves:
        cand = [i for i, d in enumerate(depths) if d < cap]
        if not cand:
            break
        d = depths.pop(rng.choice(cand))
        depths += [d + 1, d + 1]
    return depths


def _code(rng, nsym, must, cap, kind, width):
    """nsym code lengths.  kind: complete / near (longest one off the device's primary width) / deep (longest = cap, many codes) /
    single / empty / over / under (one code too many / too few); the symbols of `must` get codes where the kind has any."""
    lens = [0] * nsym
    must = sorted(must)
    if kind == "empty":
        return lens
    if kind == "single" or nsym < (3 if kind == "under" else 2):
        lens[rng.choice(must) if must else rng.randrange(nsym)] = 1
        return lens
    lo = max(len(must), 3 if kind == "under" else 2)
    leaves = rng.randint(lo, max(lo, min(nsym, lo + rng.choice((2, 8, 40, nsym)))))
    exact = None
    if kind == "near":
        exact = min(cap, rng.choice((width - 1, width + 1)))
    elif kind == "deep":
        exact, leaves = cap, rng.randint(max(lo, nsym // 2), nsym)
    elif rng.random() < 0.5:
        exact = rng.randint(1, cap)
    if exact:
        exact = min(exact, nsym - 1, cap)
        while (1 << exact) < leaves:
            exact += 1
    depths = _split(rng, leaves, cap, exact)
    if len(depths) > nsym:   # (cannot happen: leaves <= nsym and exact + 1 <= nsym)
        depths = _split(rng, nsym, cap)
    syms = must + rng.sample([x for x in range(nsym) if x not in set(must)], max(0, len(depths) - len(must)))
    syms = syms[:len(depths)]
    rng.shuffle(depths)
    for x, d in zip(syms, depths):
        lens[x] = d
    if kind == "over":
        free = [x for x in range(nsym) if not lens[x]]
        if free:
            lens[rng.choice(free)] = rng.randint(1, cap)
        else:
            x = rng.choice([x for x in range(nsym) if lens[x] > 1] or [0])
            lens[x] = max(1, lens[x] - 1)
    elif kind == "under":
        lens[rng.choice([x for x in range(nsym) if lens[x]])] = 0
    return lens


def _rle(rng, lens):
    """lens as code-length symbols (symbol, extra): plain ones and the repeats 16 / 17 / 18 where a run allows one."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        if v == 0 and r >= 3 and rng.random() < 0.8:
            if r >= 11 and rng.random() < 0.7:
                k = rng.randint(11, min(r, 138))
                out.append((18, k - 11))
            else:
                k = rng.randint(3, min(r, 10))
                out.append((17, k - 3))
            i += k
        elif i > 0 and lens[i - 1] == v and r >= 3 and rng.random() < 0.7:
            k = rng.randint(3, min(r, 6))
            out.append((16, k - 3))
            i += k
        else:
            out.append((v, 0))
            i += 1
    return out


def _header(bw, final, hlit, hdist, cl_lens, cl_syms, nclen=None, code=None):
    """A dynamic block's header from its fields: hlit / hdist as transmitted (count - 257, count - 1); code: what the code-length
    symbols are written with — default the canonical code of cl_lens, the stale shapes pass the code the reference will read them by."""
    if nclen is None:
        nclen = max([4] + [i + 1 for i in range(19) if cl_lens[_ORDER[i]]])
    bw.put(1 if final else 0, 1).put(2, 2).put(hlit, 5).put(hdist, 5).put(nclen - 4, 4)
    for i in range(nclen):
        bw.put(cl_lens[_ORDER[i]], 3)
    cc = canon(cl_lens) if code is None else code
    for x, extra in cl_syms:
        bw.code(cc[x])
        if x >= 16:
            bw.put(extra, {16: 2, 17: 3, 18: 7}[x])
    return bw


class _Gen:
    """One generated stream: the bit writer, how many bytes of history a distance may reach, the tags that go into the case's name."""

    def __init__(self, rng, hist, clean=False):
        self.rng, self.bw, self.hist, self.tags = rng, BW(), min(hist, 32768), []
        self.clean = clean   # nothing in this stream is damaged on purpose: what the reference is to accept
        self.prev = None   # the last dynamic block's (literal/length code, distance code) as canon() maps

    def tag(self, t):
        if t not in self.tags:
            self.tags.append(t)

    def grow(self, n):
        self.hist = min(32768, self.hist + n)

    def stored(self, final):
        rng = self.rng
        data = bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 1, 7, 64, 300))))
        stored_block(self.bw, data, final=final, nlen=0x1234 if rng.random() < 0.02 and not self.clean else None)
        self.grow(len(data))

    def fixed(self, final):
        rng, items = self.rng, []
        for _ in range(rng.randint(0, 40)):
            r = rng.random()
            if r < 0.6 or self.hist == 0:
                items.append(rng.getrandbits(8))
                self.grow(1)
            elif r < 0.97 or self.clean:
                length = rng.choice((3, 4, 10, 11, 66, 130, 227, 257, 258, rng.randint(3, 258)))
                dist = rng.choice((1, 2, self.hist, rng.randint(1, self.hist)))
                if length == 258 and rng.random() < 0.5:
                    items.append((258, dist, 284))   # symbol 284 with extra bits 31
                else:
                    items.append((length, dist))
                self.grow(length)
            elif r < 0.98:
                items += [("sym", rng.choice((286, 287))), ("dsym", rng.randrange(30))]
            elif r < 0.99:
                items += [("sym", 257), ("dsym", rng.choice((30, 31)))]
            elif self.hist < 32768:
                items.append((3, self.hist + 1))     # one beyond what stands
        fixed_block(self.bw, items, final=final, eob=self.clean or rng.random() >= 0.03)

    def body(self, lc, dc, eob=True, n=None):
        """A dynamic block's symbols from the codes lc / dc (canon() maps)."""
        rng, bw = self.rng, self.bw
        lits = [x for x in lc if x < 256]
        lsyms = [x for x in lc if 257 <= x <= 285]
        for _ in range(rng.randint(0, 40) if n is None else n):
            dsyms = [x for x in dc if x < 30 and _DBASE[x] <= self.hist]
            if lsyms and dsyms and (not lits or rng.random() < 0.4):
                ls = rng.choice(lsyms)
                i = ls - 257
                extra = 31 if ls == 284 and rng.random() < 0.4 else rng.getrandbits(_LEXTRA[i]) if _LEXTRA[i] else 0
                ds = rng.choice(dsyms)
                dist = min(_DBASE[ds] + (rng.getrandbits(_DEXTRA[ds]) if _DEXTRA[ds] else 0), self.hist)
                if rng.random() < 0.02 and self.hist < 32768 and not self.clean:   # one beyond what stands, where the code has that distance's symbol
                    far = max(k for k in range(30) if _DBASE[k] <= self.hist + 1)
                    if far in dc:
                        ds, dist = far, self.hist + 1
                bw.code(lc[ls]).put(extra, _LEXTRA[i])
                bw.code(dc[ds]).put(dist - _DBASE[ds], _DEXTRA[ds])
                if lc[ls][1] > PB_L:
                    self.tag("longL")
                if dc[ds][1] > PB_D:
                    self.tag("longD")
                self.grow(_LBASE[i] + extra)
            elif lits:
                x = rng.choice(lits)
                bw.code(lc[x])
                if lc[x][1] > PB_L:
                    self.tag("longL")
                self.grow(1)
            if len(lc) == 1 and rng.random() < 0.1 and not self.clean:
                bw.put(1, 1)   # the single one-bit code's missing twin
        if eob and 256 in lc:
            bw.code(lc[256])
            if lc[256][1] > PB_L:
                self.tag("longL")

    def tables(self, lit_kind=None, dist_kind=None):
        """(lit_lens, dist_lens) of a dynamic block, HLIT and HDIST at their limits among the counts."""
        rng = self.rng
        good = ("complete", "near", "deep") * 6
        kinds = good + ("single",) if self.clean else good + ("single", "over", "under")
        lk = lit_kind or rng.choice(kinds)
        dk = dist_kind or rng.choice(kinds + ("empty",))
        nlit = rng.choice((257, 258, 286, 286, rng.randint(258, 286)))
        ndist = rng.choice((1, 2, 30, 30, rng.randint(1, 30)))
        if dk in ("near", "deep"):
            ndist = max(ndist, 16)
        must = set(rng.sample(range(256), rng.choice((0, 1, 4, 30))))
        if self.clean or rng.random() >= 0.05:
            must.add(256)
        else:
            self.tag("no-eob")
        must |= set(rng.sample(range(257, nlit), min(nlit - 257, rng.choice((0, 1, 5, 29)))))
        if nlit > 284 and rng.random() < 0.5:
            must.add(284)
        if lk == "single":
            must = {256 if self.clean else rng.choice((256, 256, 65))}
        lit = _code(rng, nlit, must, 15, lk, PB_L)
        dist = _code(rng, ndist, set(range(min(ndist, rng.choice((1, 2, 4, 12))))), 15, dk, PB_D)
        return lit, dist

    def dynamic(self, final, lit=None, dist=None, n=None, clean=False):
        rng = self.rng
        clean = clean or self.clean
        if lit is None:
            lit, dist = self.tables()
        syms = _rle(rng, lit + dist)
        hlit, hdist = len(lit) - 257, len(dist) - 1
        r = 1.0 if clean else rng.random() * 2
        if r < 0.02:
            hlit = rng.choice((30, 31))           # HLIT 287 / 288
        elif r < 0.04:
            hdist = rng.choice((30, 31))          # HDIST 31 / 32
        elif r < 0.06:
            syms = [(16, rng.getrandbits(2))] + syms[1:]   # a repeat of the previous length at position 0
        elif r < 0.09:
            syms = syms + [rng.choice(((16, 0), (17, 0), (18, 0)))]   # a repeat that ends behind n
        elif r < 0.11 and syms[-1][0] >= 16 and syms[-1][1] < (3, 7, 127)[syms[-1][0] - 16]:
            syms = syms[:-1] + [(syms[-1][0], syms[-1][1] + 1)]       # ... one past n
        need = {x for x, _ in syms}
        ck = rng.choice(("complete", "near", "deep") * (6 if not clean else 1) + (() if clean else ("over", "under"))) if len(need) > 1 else "single"
        cl = _code(rng, 19, need, 7, ck, PB_C)
        nclen = 19 if rng.random() < 0.5 else None
        cc = canon(cl)
        _header(self.bw, final, hlit, hdist, cl, [(x, e) for x, e in syms if x in cc], nclen)
        lc, dc = canon(lit), canon(dist)
        self.body(lc, dc, n=n)
        self.prev = (lc, dc)

    def stale(self, table, final):
        """A non-final dynamic block with populated tables, then a dynamic block whose `table` is empty, with symbols that go through it.
        sync: those symbols are written with the code the reference will look them up in (rule R6 of flate_model), so that it reads on in
        step; else random bits."""
        rng, bw = self.rng, self.bw
        sync = rng.random() < 0.7
        self.tag("stale-" + table)
        self.tag("sync" if sync else "noise")
        junk = lambda: bw.put(rng.getrandbits(24), 24)  # noqa: E731
        # block A: literals 0 .. 18 have codes (what a stale literal/length table hands the code-length loop), a distance code with several
        # lengths (a long one among them, so that the reference's link tables are behind it)
        nlit = rng.choice((258, 270, 286))
        must = set(range(19)) | {256} | set(range(257, min(nlit, 262)))
        lit_a = _code(rng, nlit, must, 15, rng.choice(("complete", "near", "deep")), PB_L)
        dist_a = _code(rng, rng.choice((8, 16, 30)), {0, 1, 2, 3}, 15, rng.choice(("complete", "near", "deep", "single")), PB_D)
        if self.hist < 8:
            self.stored(False)
            stored_block(bw, bytes(rng.getrandbits(8) for _ in range(40)), final=False)
            self.grow(40)
        self.dynamic(False, lit_a, dist_a, n=rng.randint(1, 12), clean=True)
        lca, dca = self.prev
        if table == "dist":
            nlit = rng.choice((258, 286))
            lit = _code(rng, nlit, {65, 66, 256, 257}, 15, rng.choice(("complete", "near")), PB_L)
            dist = [0] * rng.choice((1, 2, 30))
            _header(bw, final, nlit - 257, len(dist) - 1, *self._cl(lit + dist))
            lc = canon(lit)
            self.body(lc, {}, eob=False, n=rng.randint(0, 5))
            lsym = rng.choice([x for x in lc if 257 <= x <= 285])
            bw.code(lc[lsym]).put(0, _LEXTRA[lsym - 257])
            if sync:
                ds = rng.choice([x for x in dca if x < 30 and _DBASE[x] <= self.hist] or [0])
                bw.code(dca[ds]).put(0, _DEXTRA[ds])
                self.grow(_LBASE[lsym - 257])
            else:
                junk()
            self.body(lc, {}, n=rng.randint(0, 5))
        elif table == "lit":
            nlit, ndist = rng.choice((257, 286)), rng.choice((1, 30))
            dist = _code(rng, ndist, {0}, 15, rng.choice(("empty", "single", "complete")), PB_D)
            cl, syms = self._cl([0] * nlit + dist, only_zero=rng.random() < 0.3 and not any(dist))
            _header(bw, final, nlit - 257, ndist - 1, cl, syms, nclen=4 if not any(cl[x] for x in range(1, 16)) and rng.random() < 0.5 else None)
            cc = canon(cl)
            for _ in range(rng.randint(1, 30)):   # the code-length code's symbols come out as literals; no end-of-block symbol exists
                if sync:
                    bw.code(cc[rng.choice(sorted(cc))])
                else:
                    bw.put(rng.getrandbits(8), 8)
        else:
            # the code-length code is empty: the lengths are read through block A's literal/length code
            nlit = rng.choice((257, 260))
            lit = _code(rng, nlit, {65, 256}, 7, "complete", PB_L)
            dist = _code(rng, rng.choice((1, 4)), {0}, 4, rng.choice(("empty", "single", "complete")), PB_D)
            syms = _rle(rng, lit + dist)
            if sync:
                _header(bw, final, nlit - 257, len(dist) - 1, [0] * 19, syms, nclen=rng.choice((4, 19)), code=lca)
                self.body(canon(lit), canon(dist), n=rng.randint(0, 6))
            else:
                _header(bw, final, nlit - 257, len(dist) - 1, [0] * 19, [], nclen=rng.choice((4, 19)))
                junk()
                junk()
        self.prev = None

    def _cl(self, lens, only_zero=False):
        """(cl_lens, cl_syms) for lens: a complete code-length code over the symbols the run-length form needs."""
        rng = self.rng
        if only_zero:   # symbol 18 alone, as the single one-bit code: 138 + 138 + ... zeroes
            syms, left = [], len(lens)
            while left:
                k = min(left, 138)
                if 0 < left - k < 11:   # (every repeat covers 11 .. 138 zeroes: leave the last one at least 11)
                    k = left - 11
                syms.append((18, k - 11))
                left -= k
            cl = [0] * 19
            cl[18] = 1
            return cl, syms
        syms = _rle(rng, lens)
        need = {x for x, _ in syms}
        if len(need) == 1:
            need.add(rng.choice([x for x in range(19) if x not in need]))
        return _code(rng, 19, need, 7, "complete", PB_C), syms


def _gen_stream(rng, hist, force_stale=None):
    """-> (bytes, tags) of one stream.  clean (three in ten): nothing is damaged on purpose."""
    clean = not force_stale and rng.random() < 0.3
    while True:
        g = _Gen(rng, hist, clean)
        if force_stale:
            for _ in range(rng.randint(0, 1)):
                rng.choice((g.stored, g.fixed))(False)
            last_final = rng.random() >= 0.05
            g.stale(force_stale, last_final)
        else:
            nb = rng.randint(1, 4)
            last_final = clean or rng.random() >= 0.05
            for b in range(nb):
                final = last_final and b == nb - 1
                r = rng.random()
                if r < 0.2:
                    g.stored(final)
                elif r < 0.45:
                    g.fixed(final)
                else:
                    g.dynamic(final)
        if not last_final:
            g.tag("non-final-last")
        data = g.bw.bytes()
        if len(data) <= 2048:
            break
    r = rng.random()
    if clean or force_stale:
        r = 0.1 + r * 0.9 if force_stale else 0.25 + r * 0.75   # a clean stream is not cut, a stale one rarely
    if r < 0.25 and len(data):
        bits = rng.randrange(len(data) * 8)
        data = data[:(bits + 7) >> 3]
        g.tag("cut")
    elif r < 0.35:
        data += bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 12)))
        g.tag("trailing")
    return data, g.tags


def _generated(seed, n):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        # the stale shapes: three of eight among the first 480 (the emulator's share: 60 per table), three of sixteen behind them
        stale = ("dist", "lit", "clen")[k % 8] if k % 8 < 3 and (k < 480 or k % 16 < 3) else None
        dl = rng.choice(_GEN_DICT_LENS) if rng.random() < 0.25 else 0
        data, tags = _gen_stream(rng, dl, stale)
        out.append((data, tags, _GEN_DICT[:dl]))
    return out


_gen_cache = {}


def generated(seed=GEN_SEED, n=2000):
    """n seeded structured streams as raw DEFLATE cases "gen/<k>/<tags>".  Tags: stale-dist / stale-lit / stale-clen (+ sync / noise),
    longL / longD (a symbol was written with a code longer than the device's primary table of that code), cut, trailing, no-eob,
    non-final-last.  All randomness comes from one random.Random(seed)."""
    if (seed, n) not in _gen_cache:
        _gen_cache[(seed, n)] = [C("gen/%d/%s" % (k, "+".join(t) or "plain"), d, dict=zd) for k, (d, t, zd) in enumerate(_generated(seed, n))]
    return _gen_cache[(seed, n)]


def generated_gzip(seed=GEN_SEED, n=2000):
    """The streams of generated(seed, n) as gzip members: case k wraps stream k and up to two of its successors, random FLG bits, the
    CRC-32 / ISIZE of what the stream decodes to without a dictionary (sometimes a wrong one), Multistream on or off."""
    if ("gz", seed, n) in _gen_cache:
        return _gen_cache[("gz", seed, n)]
    fl = generated(seed, n)
    rng = random.Random(seed ^ 0x677A)
    out = []
    decoded = [M.inflate(c.data, stale_tables=True) for c in fl]   # what the reference decodes, without the dictionary: gzip has none
    good = [i for i, v in enumerate(decoded) if v[1] == M.OK]
    for k in range(n):
        members = b""
        for j in range(rng.choice((1, 1, 1, 2, 2, 3))):
            # the first member is stream k; the ones behind it mostly streams that stand, so that the second and third get decoded
            i = k if j == 0 else rng.choice(good) if rng.random() < 0.85 else rng.randrange(n)
            payload = decoded[i][0]
            r = rng.random()
            kw = {"crc": zlib.crc32(payload) ^ (1 << rng.randrange(32))} if r < 0.05 else {"isize": (len(payload) + 1) & 0xFFFFFFFF} if r < 0.1 else {}
            flg = rng.choice((0, 0, 2, 4, 8, 16, 31, rng.randrange(32), 0x20 if rng.random() < 0.1 else 0))
            members += gz_member(payload, flg=flg, deflated=fl[i].data, bad_hcrc=rng.random() < 0.03, **kw)
        out.append(C("gengz/%d/%s" % (k, fl[k].name.split("/", 2)[2]), members, fmt="gzip", multistream=rng.random() < 0.7))
    _gen_cache[("gz", seed, n)] = out
    return out


CRC_SWEEP_LENGTHS = (list(range(0, 9)) + list(range(505, 521)) + list(range(764, 773)) + list(range(1020, 1029)) + list(range(4092, 4101)) + [65535])
CRC_SWEEP_TWINS = (511, 512, 513, 768, 769)


def crc_sweep():
    """gzip inputs of two members for the write pass's CRC-32 (s2_crc32c_wave of kc_s2_dev.h: serial below 512 bytes, from 512 on 64
    pieces of roundup4(ceil(len / 64)) bytes and a tail): a first member of 1, 2 or 3 bytes, so that the second one's bytes start at
    every residue mod 4 in dst, then a member of noise in one stored block at the lengths where the piece size steps (512 | 513,
    768 | 769) and around them.  The twins carry a trailer CRC with one bit flipped: CHECKSUM, and a zero-filled range."""
    out = []
    for n in CRC_SWEEP_LENGTHS:
        rng = random.Random(0xC4C32 + n)
        payload = rng.randbytes(n)
        body = stored_block(BW(), payload).bytes()
        for first in (1, 2, 3):
            head = rng.randbytes(first)
            m1 = gz_member(head, deflated=stored_block(BW(), head).bytes())
            out.append(C("crc/len%d-first%d" % (n, first), m1 + gz_member(payload, deflated=body), fmt="gzip"))
            if n in CRC_SWEEP_TWINS:
                bad = zlib.crc32(payload) ^ (1 << rng.randrange(32))
                out.append(C("crc/len%d-first%d-bad-crc" % (n, first), m1 + gz_member(payload, deflated=body, crc=bad), fmt="gzip"))
    return out


COPY_SWEEP_DICT = bytes((i * 29 + 11) & 255 for i in range(300))


def copy_sweep():
    """Self-overlapping matches that take several rounds of 64 lanes (the copy loop moves one byte per lane per round from
    d - dist + k % dist), in fixed blocks: from plain output, and beginning inside a preset dictionary and running over into the
    output (fewer bytes of output than the distance)."""
    out = []
    for dist in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        for length in (63, 64, 65, 127, 128, 129, 257, 258):
            lits = [(i * 7 + dist) & 255 for i in range(dist + 2)]
            out.append(C("copy/d%d-l%d" % (dist, length), fixed_block(BW(), lits + [(length, dist), 46]).bytes()))
            mine = dist // 2 if dist < length else dist - 1   # mine < dist, and the match crosses from the dictionary into the output
            out.append(C("copy/d%d-l%d-dict" % (dist, length), fixed_block(BW(), lits[:mine] + [(length, dist), 46]).bytes(), dict=COPY_SWEEP_DICT))
    return out


def families():
    """The case families whose reference verdicts are committed as digests (tests/golden/reference_go_flate_sha256.txt)."""
    fl, gz = mutations()
    return [("directed", cases()), ("mut", fl), ("mutgz", gz), ("generated", generated()), ("generated-gz", generated_gzip())]


def family_digest(cs, verdict_of):
    """SHA-256 over the records (name, class, consumed, len, sha256(bytes)) of a family's cases, verdict_of(case) -> (bytes, class, consumed)."""
    import hashlib
    h = hashlib.sha256()
    for c in cs:
        out, cls, used = verdict_of(c)
        h.update(c.name.encode() + b"\0" + struct.pack("<IQQ", cls, used, len(out)) + hashlib.sha256(out).digest())
    return h.hexdigest()


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
