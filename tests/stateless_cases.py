"""Inputs for the stateless writers: the smallest shapes at which each rule of StatelessDeflate can go wrong, directed and seeded, with
what the model (tests/stateless_model.py) writes for them.  Shared by the model's, the emulator's and the device's tests.

A case is (name, data, eof, dict).  The cuts are the reference's own (32767 - len(dict), then 24575), so a case that is to meet a rule
across blocks has at least 32768 bytes; everything about one block is met at a few hundred.
"""
import functools
import random

import deflate_cases as D
import stateless_model as M

FIRST, LATER = M.MAX_BLOCK, M.MAX_BLOCK - M.MAX_DICT
text = D.text


def other_text(n, at=0):
    """Text over another alphabet (0-9a-f): a table made for it lacks most of text()'s symbols, and the reverse."""
    return text((n + 1) // 2, at).hex().encode()[:n]


def rand(n, rng):
    return rng.randbytes(n)


def planted(n, rng, every, length):
    """Random bytes, and every `every` bytes a copy of `length` bytes from a little further back: few tokens fewer than bytes."""
    return bytes(_plant(bytearray(rng.randbytes(n)), rng, every, length))


def _plant(b, rng, every, length):
    at = every
    while at + length <= len(b):
        back = rng.randrange(length, min(at, 4000) + 1) if at > length else length
        b[at:at + length] = b[at - back:at - back + length]
        at += every
    return b


def tie_planted(seed):
    """Random bytes with planted matches of a seeded length, spacing and size: tools/find_deflate_ties.py walks the seeds for inputs
    whose token count lands on len - len>>4 (the last count that still goes to writeBlockDynamic) and on one more (writeBlockHuff)."""
    rng = random.Random(0x57A7 + seed)
    n = rng.randrange(40, 2500)
    return planted(n, rng, rng.choice((24, 32, 40, 48, 64)), rng.choice((5, 6, 7, 8)))


TOKEN_TIES = {0: (73, 174, 233, 235), 1: (32, 111, 320, 333)}   # tokens - (len - len>>4) -> seeds of tie_planted


# newSize - reuseSize of the second, open block of shifted_alphabet(seed)[:FIRST + m] -> (seed, m): reuse wins at 0 and 1, the new table at
# -1 and -2.  newSize is 2 * (lastHeader + EstimatedBits) + the EOB's length, so each of them is one bit of EstimatedBits from the other side.
DYN_TIES = {1: ((0, 506), (6, 491)), 0: ((0, 508), (2, 457)), -1: ((3, 592), (6, 492)), -2: ((2, 463), (4, 565))}
STORED_BY_SIZE = (0, 1, 2, 3, 5, 6, 7, 9)   # seeds of stored_by_size_planted at which the dynamic block would be larger than the bytes
NEW_TABLE_SEEDS = (5, 6, 7, 9, 10, 11, 13, 14)   # shifted_alphabet seeds whose second, open block takes the new table


def stored_by_size_planted(seed):
    rng = random.Random(0xD5B0 + seed)
    return planted(rng.randrange(200, 700), rng, 40, 6)


def shifted_alphabet(seed):
    """Block 1: 32 symbols at geometric frequencies (ratio 0.8), every one of them a literal somewhere, with planted matches; blocks 2
    and 3: the sixteen rarest at equal frequencies, matches planted the same way.  Block 2 can be written under block 1's table, at
    more than twice the doubled estimate of a table of its own: the new table with an owed EOB.  Block 3 goes on under block 2's."""
    rng = random.Random(seed)
    syms = list(range(0xC0, 0xE0))
    b1 = bytearray(rng.choices(syms, weights=[0.8 ** k for k in range(32)], k=FIRST))
    for k, v in enumerate(syms[16:]):
        b1[900 + 1900 * k] = v
    b1 = _plant(b1, rng, 100, 12)
    b2 = _plant(bytearray(rng.choices(syms[16:], k=LATER)), rng, 100, 12)
    return bytes(b1) + bytes(b2) + bytes(b2[:2000])


def huff_block(n, rng, history=b"", first=0x30):
    """A block that writeBlockHuff writes as a Huffman block: 24 symbols at geometric frequencies (ratio 0.75, about 3.3 bits a byte, so
    that even the DOUBLED estimate of this path stays below the stored size) in which statelessEnc finds one match, planted at byte 16,
    and no other.  Such bytes repeat their 4-byte strings all the time, so the model's own match finder is run over the block (behind
    `history`, the 8 KiB the reference keeps in front of a later block) and a byte inside every match it finds is drawn again, until
    none is left.  A prefix of the block has the same property."""
    syms = list(range(first, first + 24))
    wts = [0.75 ** i for i in range(24)]
    b = bytearray(rng.choices(syms, weights=wts, k=n))
    b[16:24] = b[0:8]
    h = len(history)
    for _ in range(1000):
        t = M.Tokens()
        M.stateless_enc(t, history + bytes(b), h)
        ev = [e for e in t.events if e[0] - h >= 32]
        if not ev:
            return bytes(b)
        for s, _, back, _, _ in ev:
            i = s - h + back + 1
            old = b[i]
            while b[i] == old:
                b[i] = rng.choices(syms, weights=wts)[0]
    raise AssertionError("huff_block: matches left")


# inputs whose LAST block is Huffman-only and goes on under the table in force: with eof the stream has no final block
NO_FINAL_BLOCK = ("huff-reuse-2-eof", "huff-reuse-2-short-tail-eof")


def pieces(spec, rng):
    out = b""
    for kind, n in spec:
        if kind == "text":
            out += text(n, rng.randrange(1 << 18))
        elif kind == "other":
            out += other_text(n, rng.randrange(1 << 18))
        elif kind == "random":
            out += rand(n, rng)
        elif kind == "planted":
            out += planted(n, rng, 40, 6)
        elif kind == "planted-dense":
            out += planted(n, rng, 100, 12)
        elif kind == "equal":
            out += bytes([rng.randrange(256)]) * n
        elif kind == "period":
            p = rng.randbytes(rng.randrange(1, 40))
            out += (p * (n // len(p) + 1))[:n]
        elif kind == "skew":
            out += D.skewed(n, rng, ord("a"))
        else:
            raise ValueError(kind)
    return out


@functools.lru_cache(maxsize=None)
def directed():
    rng = random.Random(0x57A7E1E5)
    c = []

    def add(name, data, eof=True, dic=b""):
        c.append((name, bytes(data), eof, bytes(dic)))

    # lengths around statelessEnc's 13-byte floor, both endings
    for n in (0, 1, 12, 13, 14):
        for eof in (True, False):
            add("len-%d-equal-%s" % (n, "eof" if eof else "open"), b"a" * n, eof)
            add("len-%d-text-%s" % (n, "eof" if eof else "open"), text(n, 321), eof)
    # the first cut and the second
    for n in (FIRST - 1, FIRST, FIRST + 1, FIRST + LATER, FIRST + LATER + 1):
        add("cut-%d-text" % n, text(n, 11))
        add("cut-%d-text-open" % n, text(n, 99000), False)
    add("cut-%d-random" % (FIRST + 1), rand(FIRST + 1, rng))
    # dictionaries: the first block's edge at 32767 - len(dict)
    for d in (1, 8191, 8192, 8193):
        dic = text(d, 50000)
        edge = FIRST - min(d, M.MAX_DICT)
        for n in (edge - 1, edge, edge + 1):
            add("dict-%d-len-%d" % (d, n), text(n, 52000), True, dic)
        add("dict-%d-len-20" % d, text(20, 50000 + max(0, d - 30)), True, dic)
        add("dict-%d-len-12-open" % d, dic[-12:], False, dic)
        add("dict-%d-len-13-open" % d, dic[-13:], False, dic)
    # all-equal bytes: a first match through the never-written slot at offset 0, AddMatchLong's split at 258 .. 264
    for run in range(258, 266):
        add("equal-%d" % (run + 1), b"z" * (run + 1))
        add("equal-%d-then-text" % (run + 1), b"z" * (run + 1) + text(40, 5), False)
    add("equal-32767", b"\0" * FIRST)
    add("equal-32768-open", b"\xff" * (FIRST + 1), False)
    add("equal-516", b"q" * 516)
    add("equal-517", b"q" * 517)
    # text, random (no match: stored), random with a few planted matches (more than 15/16 tokens: writeBlockHuff)
    for n in (100, 300, 1000, 5000, 20000):
        add("text-%d" % n, text(n, 1000 * n))
        add("other-%d" % n, other_text(n, 17 * n), n != 1000)
    for n in (13, 100, 2000, FIRST, 40000):
        add("random-%d" % n, rand(n, rng), n != 2000)
    for n in (200, 1500, 5000, FIRST, FIRST + LATER + 3000):
        add("planted-%d" % n, planted(n, rng, 40, 6), n != 1500)
        add("planted-dense-%d" % n, planted(n, rng, 100, 12), n != 5000)
    # short inputs with matches: fewer than 250 tokens, the fixed-table branches
    for n in (13, 16, 24, 40, 77, 150, 300):
        p = text(7, n)
        add("short-period-%d" % n, (p * 50)[:n])
        add("short-period-%d-open" % n, (p * 50)[:n], False)
        add("short-text-twice-%d" % n, (text(n // 2, 9 * n) * 3)[:n])
    # ... behind an open table (the fixed header owes its EOB), and a stored block behind one
    for tail in (13, 60, 200):
        add("text-then-short-%d" % tail, text(FIRST, 3) + (text(5, tail) * 50)[:tail])
        add("text-then-short-%d-open" % tail, text(FIRST, 3) + (text(5, tail) * 50)[:tail], False)
    add("text-then-random-tail", text(FIRST, 3) + rand(500, rng))
    add("text-then-one-byte", text(FIRST + 1, 3))
    add("text-then-12-bytes", text(FIRST + 12, 3), False)
    # blocks alternating: reuse, a new table with an owed EOB, cannot-reuse, stored and Huffman-only behind an open table
    alt = (("text", "text", "text"), ("text", "other", "text"), ("other", "text", "random", "text"), ("text", "random", "text", "other"),
           ("text", "planted", "text"), ("planted", "text", "planted", "other"), ("skew", "skew", "text"), ("text", "planted-dense", "other", "other"),
           ("other", "other", "equal", "other"), ("text", "equal", "text"), ("planted", "planted", "planted"), ("period", "text", "period"))
    for k, kinds in enumerate(alt):
        spec = [(kind, FIRST if j == 0 else LATER) for j, kind in enumerate(kinds)]
        spec[-1] = (spec[-1][0], 3000 + 500 * k)
        add("alt-%s" % "-".join(kinds), pieces(spec, rng), k % 3 != 1)
    for seed in (0, 1, 3):
        add("shifted-alphabet-%d" % seed, shifted_alphabet(seed), seed == 1)
    # a candidate at offset 0 through a slot never written (position 0 is never indexed without a dictionary)
    add("slot-0-hit", b"abcdWXYZ0123abcdefgh" + text(30, 4))
    add("slot-0-hit-later", text(200, 77) + text(200, 77)[:9] + rand(20, rng))
    # backward extension: to t == 0, and to nextEmit
    # (position 20 is not probed: the candidate is "abcd" at 1, and one byte back reaches t == 0)
    add("back-to-t0", b"Xabcdefgh-0123456789Xabcdefgh" + text(20, 8))
    # (a first match ends at 37; "bcde" is found at 38 against 15 and one byte back reaches nextEmit, though the byte in front of both is a 9)
    add("back-to-next-emit", bytes([0x80]) + b"0123456789" + bytes([0x90, 0x91]) + b"9abcdefghijkl" + bytes([0xA0]) + b"0123456789abcdefghijkl" + bytes(range(0xB0, 0xC0)))
    # a match from a block's first bytes into the last bytes of its history, and the same into a dictionary
    t2 = bytearray(text(FIRST + 4000, 60000))
    t2[FIRST:FIRST + 60] = t2[FIRST - 60:FIRST]
    add("match-into-history-tail", t2)
    t3 = bytearray(rand(FIRST + 300, rng))
    t3[FIRST:FIRST + 100] = t3[FIRST - 100:FIRST]
    add("match-into-history-tail-random", t3)
    t4 = bytearray(rand(FIRST + 300, rng))
    t4[FIRST:FIRST + 100] = t4[FIRST - M.MAX_DICT:FIRST - M.MAX_DICT + 100]  # 8192 back: the first byte of the history
    add("match-at-history-head-random", t4)
    dic = rand(5000, rng)
    add("match-into-dict-tail", dic[-80:] + rand(40, rng), True, dic)
    add("match-into-dict-head", dic[:80] + rand(40, rng), True, dic)
    add("match-into-dict-beyond-8192", text(8193, 123)[:60] + text(100, 9), True, text(8193, 123))
    add("dict-random-input", rand(3000, rng), False, text(4000, 5))
    add("dict-text-two-blocks", text(FIRST + 500, 70000), True, text(6000, 64000))
    # writeBlockHuff that WRITES a Huffman block, and the blocks behind it: under the table in force (with eof: no final block at all;
    # open: the EOB and the empty stored block), a third block that goes on to writeBlockDynamic (lastHuffMan: the owed EOB, a new
    # table), another alphabet (a symbol the table lacks: MaxInt32, a new table), random bytes (stored behind the owed EOB)
    rng = random.Random(0x4AFF0E0B)
    w1 = huff_block(FIRST, rng)
    w2 = huff_block(LATER, rng, w1[-M.MAX_DICT:])
    add("huff-reuse-2-eof", w1 + w2)
    add("huff-reuse-2-short-tail-eof", w1 + w2[:3000])
    add("huff-reuse-2-open", w1 + w2[:3500], False)
    add("huff-one-block-eof", w1[:20000])
    add("huff-one-block-open", w1[:1500], False)
    add("huff-huff-then-dynamic", w1 + w2 + text(3000, 41))
    add("huff-then-dynamic", w1 + text(3500, 43), False)
    add("huff-then-other-alphabet", w1 + huff_block(3800, rng, w1[-M.MAX_DICT:], first=0x80))
    add("huff-reuse-then-other-alphabet", w1 + w2 + huff_block(2600, rng, w2[-M.MAX_DICT:], first=0x80), False)
    add("huff-then-random", w1 + rand(3000, rng))
    add("huff-then-short-fixed", w1 + (text(5, 3) * 30)[:100])
    t1 = text(FIRST, 47)
    add("dynamic-then-huff", t1 + huff_block(3900, rng, t1[-M.MAX_DICT:]))
    # reuse of a dynamic table, the new table with its owed EOB, and stored-by-size, in two-block inputs the emulator runs too
    for k in range(4):
        add("text-text-reuse-%d" % k, text(FIRST + 2500 + 300 * k, 7000 * k + 13), k % 2 == 0)
    # (seeds found by `python tools/find_deflate_ties.py shapes`: the model decides for the new table in the second, open block; with eof the
    # last block never weighs reuse)
    for seed in NEW_TABLE_SEEDS:
        add("shifted-alphabet-two-blocks-%d" % seed, shifted_alphabet(seed)[:FIRST + 3900], False)
    for k in range(5):
        add("dense-then-dense-%d" % k, planted(FIRST + 1500 + 500 * k, rng, 100, 12), k % 2 == 1)
    # a few hundred random bytes with matches planted: just under 15/16 tokens, and the dynamic block would be larger than the bytes
    for seed in STORED_BY_SIZE:
        d = stored_by_size_planted(seed)
        add("planted-stored-by-size-%d" % len(d), d, seed % 2 == 0)
    # writeBlockDynamic's reuse against the doubled estimate of a new table, within two bits either way
    for m, pairs in DYN_TIES.items():
        for seed, extra in pairs:
            add("tie-dyn-new-reuse%+d-seed-%d" % (m, seed), shifted_alphabet(seed)[:FIRST + extra], False)
    # the token count on the threshold between writeBlockDynamic and writeBlockHuff, and one above it
    for m, seeds in TOKEN_TIES.items():
        for seed in seeds:
            add("tie-tokens-%d-seed-%d" % (m, seed), tie_planted(seed), seed % 2 == 0)
    names = [x[0] for x in c]
    assert len(set(names)) == len(names)
    return tuple(c)


SEED_KINDS = ("text", "other", "random", "planted", "planted-dense", "equal", "period", "skew")


@functools.lru_cache(maxsize=None)
def seeded(count=300):
    rng = random.Random(0x5EEDED)
    c = []
    for k in range(count):
        shape = k % 10
        if shape < 6:      # one small block
            spec = [(rng.choice(SEED_KINDS), rng.choice((rng.randrange(13, 400), rng.randrange(400, 6000)))) for _ in range(rng.randrange(1, 4))]
        elif shape < 8:    # the block's edge
            spec = [(rng.choice(SEED_KINDS), rng.randrange(1, 300)), (rng.choice(("text", "other", "planted")), FIRST - rng.randrange(0, 600))]
        else:              # several blocks
            spec = [(rng.choice(SEED_KINDS), FIRST)] + [(rng.choice(SEED_KINDS), LATER) for _ in range(rng.randrange(0, 3))]
            spec.append((rng.choice(SEED_KINDS), rng.randrange(1, 4000)))
        data = pieces(spec, rng)
        dic = b""
        if rng.random() < 0.3:
            d = rng.choice((1, 100, 3000, 8192, 9000))
            dic = data[:d] if rng.random() < 0.5 and len(data) >= d else text(d, rng.randrange(1 << 18))
            if shape >= 8:  # keep the later cuts where they are: the first block shrinks by the dictionary
                data = data[min(len(dic), M.MAX_DICT):]
        c.append(("seed-%03d-%s" % (k, "-".join(s[0] for s in spec)), data, rng.random() < 0.6, dic))
    return tuple(c)


def all_cases():
    return directed() + seeded()


@functools.lru_cache(maxsize=None)
def _model(index):
    name, data, eof, dic = all_cases()[index]
    return M.stateless_deflate_ex(data, eof, dic)


def model(case):
    """The model's Result for a case of all_cases(), computed once."""
    return _model(_index()[case[0]])


@functools.lru_cache(maxsize=None)
def _index():
    return {c[0]: k for k, c in enumerate(all_cases())}


@functools.lru_cache(maxsize=None)
def _model_gzip(index):
    return M.gzip_stateless(all_cases()[index][1])


def model_gzip(case):
    """gzip.NewWriterLevel(w, StatelessCompression); Write(data); Close() of the case's data (its eof and dict do not apply)."""
    return _model_gzip(_index()[case[0]])


def total_counts(cases=None):
    tot = dict.fromkeys(M.DECISIONS, 0)
    for c in (cases if cases is not None else all_cases()):
        for k in tot:
            tot[k] += model(c).counts[k]
    return tot


def emu_subset():
    """What the emulator runs: every directed case of at most two blocks, a few of more, and every sixth seeded one."""
    d = [c for c in directed() if len(c[1]) <= FIRST + 4000 or c[0].startswith(("alt-text-other", "alt-other-text", "shifted-alphabet-0", "alt-skew-skew", "alt-text-planted-", "huff-"))]
    return tuple(d) + seeded()[::6]


COUNT_NAMES = M.DECISIONS + ("quick-stored", "est-stored", "first-table", "reuse", "new-table-eob-owed", "not-reusable")  # KCSL_N_*


def emu_stateless(datas, gzip=False, eof=True, dic=b"", cap=None):
    """kcemu_flate_stateless over `datas`.  Returns (rc, list of outputs or None, out_off, counts by name); checks the guards on both sides
    of a dst that is not word-aligned, and the bound's closed form against the model's."""
    import ctypes as C
    import numpy as np
    import emu_lib
    L = emu_lib.lib()
    fn = L.kcemu_flate_stateless
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.kcemu_flate_stateless_bound.restype = C.c_uint64
    L.kcemu_flate_stateless_bound.argtypes = [C.c_uint64, C.c_uint64]
    src, off = D.pack(datas)
    n = len(datas)
    dl = 0 if gzip else len(dic)
    assert all(int(L.kcemu_flate_stateless_bound(len(d), dl)) == M.bound(len(d), dl) for d in datas)
    bound = sum(M.bound(len(d), dl) + (20 if gzip else 0) for d in datas)
    if cap is None:
        cap = bound
    buf = np.full(cap + 2 * D.GUARD, 0xA5, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    counts = np.zeros(16, dtype=np.uint32)
    rc = fn(int(gzip), src.ctypes.data if len(src) else buf.ctypes.data, off.ctypes.data, n, int(eof), bytes(dic), len(dic), buf.ctypes.data + D.GUARD, cap,
            out_off.ctypes.data, counts.ctypes.data)
    total = int(out_off[n])
    assert np.all(buf[:D.GUARD] == 0xA5), "bytes in front of dst were written"
    named = {k: int(counts[i]) for i, k in enumerate(COUNT_NAMES)}
    if rc != 0:
        assert np.all(buf == 0xA5), "a refused call wrote"
        return rc, None, out_off, named
    assert total <= cap and np.all(buf[D.GUARD + total:] == 0xA5), "bytes behind the output were written"
    dst = buf[D.GUARD:D.GUARD + total]
    return rc, [dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)], out_off, named
