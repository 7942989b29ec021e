"""Inputs for the HuffmanOnly writers: the smallest shapes at which each part of the block writer can go wrong, directed and seeded,
with what the model (tests/deflate_model.py) writes for them.  Shared by the model's, the emulator's and the device's tests.

A case is (name, data, block, penalty, end).  The directed multi-block cases run at compressor.init's own (32768, 10).  The seeded
ones mostly run at blocks of 2048 or 4096 bytes: the block writer takes the same paths at any block size above the quick check's
1024 bytes, the chain is as long, and the model and the emulator stay quick; one in eight runs at 32768.
"""
import functools
import os
import random

import deflate_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK, PENALTY = 32768, 10
KINDS = ("one", "two", "uniform", "random", "fib", "text", "equal", "skew-a", "skew-h", "skew-z")


@functools.lru_cache(maxsize=None)
def _twain():
    with open(os.path.join(HERE, "golden", "ref_inputs", "Mark.Twain-Tom.Sawyer.txt"), "rb") as f:
        return f.read()


def text(n, at=0):
    t = _twain()
    at %= len(t)
    out = t[at:at + n]
    while len(out) < n:
        out += t[:n - len(out)]
    return out


def fib_block(n_sym, rng):
    """n_sym symbols with the Fibonacci frequencies 1, 1, 2, 3 ...: the unconstrained code is n_sym - 1 deep (21 symbols: 28 656
    bytes and a depth of 20 against the limit of 15)."""
    f = [1, 1]
    while len(f) < n_sym:
        f.append(f[-1] + f[-2])
    b = bytearray()
    for s, k in enumerate(f):
        b += bytes([65 + s]) * k
    lst = list(b)
    rng.shuffle(lst)
    return bytes(lst)


def skewed(n, rng, heavy, alphabet=b"abcdefgh"):
    """The alphabet's bytes, `heavy` three times in four."""
    return bytes(heavy if rng.random() < 0.75 else rng.choice(alphabet) for _ in range(n))


def block_of(kind, n, rng):
    if kind == "one":
        return bytes([rng.randrange(256)]) * n
    if kind == "two":
        a, b = rng.sample(range(256), 2)
        return bytes(rng.choice((a, a, a, b)) for _ in range(n))
    if kind == "uniform":  # every value as often as every other: the quick check's sum is (nearly) zero
        lst = [k & 0xFF for k in range(n)]
        rng.shuffle(lst)
        return bytes(lst)
    if kind == "random":
        return rng.randbytes(n)
    if kind == "fib":
        k = 21
        while k > 3 and _fib_sum(k) > n:
            k -= 1
        return (fib_block(k, rng) + bytes([65]) * n)[:n]
    if kind == "text":
        return text(n, rng.randrange(1 << 18))
    if kind == "equal":
        return b"\0" * n
    if kind == "skew-a":
        return skewed(n, rng, ord("a"))
    if kind == "skew-h":
        return skewed(n, rng, ord("h"))
    if kind == "skew-z":  # a byte the other skewed blocks do not have
        return skewed(n, rng, ord("h"), b"abcdefghz")
    raise ValueError(kind)


def tie_mix(seed, n, every):
    """Random bytes with every `every`-th byte an 'A': a little under 8 bits a byte, so that at a few hundred bytes the estimate of a
    Huffman block lands on the stored size (tools/find_deflate_ties.py walks n for the exact tie)."""
    b = bytearray(random.Random(0x71E5 + seed).randbytes(1024))
    b[::every] = bytes([0x41]) * len(b[::every])
    return bytes(b[:n])


def tie_shift(seed, n, p):
    """skewed() bytes whose heavy byte is 'h' for p sixteenths of them and 'a' for the rest: behind a block heavy in 'a' the cost under
    its table grows with n until it meets the estimate of a new table."""
    rng = random.Random(0x71E6 + seed)
    return bytes(skewed(1, rng, ord("h") if rng.random() < p / 16 else ord("a"))[0] for _ in range(n))


def tie_quick(delta):
    """Two blocks of 2048 bytes over the bytes 32..255.  The second one's histogram is built, not searched: 32 byte values absent, 32
    sixteen times, 192 eight times, so that the quick check's sum of (v - 8)^2 is 32*64 + 32*64 = 4096 = 2n exactly (`abs < max` is
    false: the block goes on, and under the first block's table it is written as a Huffman block), and with a few counts moved by one,
    4096 + delta for an even delta (the sum has the parity of the sum of the deviations, which is 0).  At 4094 the quick check stores."""
    assert delta in (-2, 0, 2)
    rng = random.Random(0x71E8)
    first = []
    for v in range(32, 64):
        first += [v] * 28
    for v in range(64, 256):
        first += [v] * 6
    counts = {v: 16 for v in range(32, 64)}
    counts.update({v: 8 for v in range(64, 256)})
    if delta == 2:
        counts[64], counts[65] = 9, 7
    elif delta == -2:  # 16 -> 15 and 8 -> 9: -15 + 1; six pairs 8 -> 9 / 7: + 12
        counts[32], counts[64] = 15, 9
        for k in range(6):
            counts[66 + 2 * k], counts[67 + 2 * k] = 9, 7
    second = [v for v, k in counts.items() for _ in range(k)]
    assert len(first) == len(second) == 2048 and sum((k - 8) ** 2 for k in counts.values()) + 32 * 64 == 4096 + delta
    rng.shuffle(first)
    rng.shuffle(second)
    return bytes(first) + bytes(second)


def tie_first():
    return block_of("skew-a", 2048, random.Random(0x71E7))


# (margin name, value) -> generator arguments, found by `python tools/find_deflate_ties.py huff` with the model's margins
TIES = {("ssize-est", 0): ("mix", 0, 481, 6), ("ssize-est", 1): ("mix", 0, 482, 6),
        ("est-reuse", 0): ("shift", 0, 1597, 2), ("est-reuse", -1): ("shift", 0, 1605, 2)}


def _fib_sum(k):
    a, b, s = 1, 1, 0
    for _ in range(k):
        s += a
        a, b = b, a + b
    return s


@functools.lru_cache(maxsize=None)
def directed():
    rng = random.Random(0xDEF1A7E)
    C = []

    def add(name, data, block=BLOCK, penalty=PENALTY, ends=(M.END_CLOSE, M.END_FLUSH)):
        for e in ends:
            C.append(("%s/%s" % (name, "close" if e == M.END_CLOSE else "flush"), bytes(data), block, penalty, e))

    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 32767, 32768, 32769, 65535, 65536, 65537, 98304, 98305):
        add("text-%d" % n, text(n, 1000 + n))
    for n in range(1, 65):  # blocks and streams that end at every bit phase
        add("sweep-%d" % n, text(n, 77), ends=(M.END_CLOSE,) if n % 2 else (M.END_FLUSH,))
    for n in (1, 2, 300, 1025, 5000):
        add("one-%d" % n, block_of("one", n, rng))
        add("two-%d" % n, block_of("two", n, rng))
    add("uniform-4096", block_of("uniform", 4096, rng))
    add("uniform-32768", block_of("uniform", 32768, rng))
    add("random-1024", block_of("random", 1024, rng))   # not above 1024: the estimate stores it
    add("random-1025", block_of("random", 1025, rng))   # the quick check does
    add("random-40000", block_of("random", 40000, rng))
    add("fib-21", fib_block(21, rng))
    add("fib-21-max-block", fib_block(21, rng) + fib_block(21, rng), block=65535, penalty=8)
    add("equal-32768", b"\0" * 32768)
    add("equal-65535-one-block", b"\xAA" * 65535, block=65535, penalty=8)
    # multi-block, at 32 KiB blocks
    a1, a2 = skewed(32768, rng, ord("a")), skewed(32768, rng, ord("a"))
    add("multi-reuse", a1 + a2 + a1[:5000])
    add("multi-not-reusable", a1 + block_of("skew-z", 32768, rng))
    add("multi-new-table-cheaper", a1 + skewed(32768, rng, ord("h")) + a2[:100])
    add("multi-huff-stored-huff", a1 + rng.randbytes(32768) + a2)
    add("multi-stored-first", rng.randbytes(32768) + text(40000, 5))
    add("multi-text-4", text(4 * 32768 + 17, 9))
    # ties of writeBlockHuff and their neighbours, at blocks of 2048: ssize == estBits (stored wins) and one more; estBits == reuseSize
    # (reuse wins) and one less (a new table behind the owed EOB)
    for (name, m), (kind, seed, n, arg) in TIES.items():
        data = tie_mix(seed, n, arg) if kind == "mix" else tie_first() + tie_shift(seed, n, arg)
        add("tie-%s-%d" % (name, m), data, block=2048)
    # the quick check's `abs < max` at abs == max - 2, max and max + 2 (float64 in the reference, integers in the model and the kernel)
    for delta in (-2, 0, 2):
        add("tie-abs-max%+d" % delta, tie_quick(delta), block=2048)
    return tuple(C)


@functools.lru_cache(maxsize=None)
def seeded(count=400):
    rng = random.Random(0x5EEDED)
    C = []
    for k in range(count):
        block = 32768 if k % 8 == 7 else rng.choice((2048, 4096))
        nblk = rng.randint(1, 5)
        # chains that stay in one family of distributions (reuse, new table, not reusable) or mix everything (stored in between)
        family = rng.choice((("skew-a", "skew-a", "skew-h", "skew-z"), ("text", "text", "skew-a", "random"), KINDS, ("skew-a", "skew-h"),
                             ("skew-a", "skew-z", "uniform", "random")))
        parts = []
        for b in range(nblk):
            n = block if b + 1 < nblk else rng.choice((block, rng.randint(1, block), rng.randint(1, 64)))
            parts.append(block_of(rng.choice(family), n, rng))
        end = M.END_FLUSH if rng.random() < 0.4 else M.END_CLOSE
        C.append(("seed-%03d" % k, b"".join(parts), block, rng.choice((10, 10, 10, 8, 7)), end))
    return tuple(C)


@functools.lru_cache(maxsize=None)
def model(case, gzip=False):
    """What the model writes for a case: (bytes, Result of the flate stream)."""
    _, data, block, penalty, end = case
    res = M.deflate_ex(data, block, penalty, end)
    if not gzip:
        return res.data, res
    return M.gzip_deflate(data, block, penalty, end), res


def emu_subset():
    """What the emulator runs: every directed case and the first 160 seeded ones."""
    return directed() + seeded()[:160]


def totals(cases):
    counts = dict.fromkeys(M.DECISIONS, 0)
    boundary, endp = set(), set()
    for c in cases:
        r = model(c)[1]
        for k, v in r.counts.items():
            counts[k] += v
        boundary |= r.boundary_phases
        endp.add(r.end_phase)
    return counts, boundary, endp


def groups(cases):
    """The cases by (block, penalty, end): what one call of the writers can take together, in the order given."""
    g = {}
    for c in cases:
        g.setdefault(c[2:], []).append(c)
    return g


def check_conditions():
    """What the issue of this feature asks of the case set, counted by the model."""
    counts, boundary, endp = totals(directed() + seeded())
    assert boundary == set(range(8)) and endp == set(range(8)), (boundary, endp)
    s = seeded()
    counts = totals(s)[0]
    assert all(counts[k] >= 20 for k in M.DECISIONS), counts
    flush = sum(c[4] == M.END_FLUSH for c in s)
    assert 4 * flush >= len(s) and 4 * (len(s) - flush) >= len(s), flush
    return counts


def pack(datas):
    """The inputs concatenated behind 0xA5 guards, and their offsets: (array, offset of the first input, in_off)."""
    import numpy as np
    off = np.zeros(len(datas) + 1, dtype=np.uint64)
    for i, d in enumerate(datas):
        off[i + 1] = off[i] + len(d)
    return np.frombuffer(b"".join(datas), dtype=np.uint8).copy(), off


GUARD = 37  # bytes of 0xA5 on both sides of dst (odd: dst is not word-aligned)


def emu_deflate(datas, gzip=False, end=M.END_CLOSE, block=BLOCK, penalty=PENALTY, cap=None):
    """kcemu_flate_deflate / kcemu_gzip_deflate over `datas`.  Returns (rc, list of outputs or None, out_off); checks the guards."""
    import ctypes as C
    import numpy as np
    import emu_lib
    L = emu_lib.lib()
    fn = L.kcemu_gzip_deflate if gzip else L.kcemu_flate_deflate
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.kcemu_flate_deflate_bound.restype = C.c_uint64
    L.kcemu_flate_deflate_bound.argtypes = [C.c_uint64, C.c_uint32]
    src, off = pack(datas)
    n = len(datas)
    bound = sum(int(L.kcemu_flate_deflate_bound(len(d), block)) + (18 if gzip else 0) for d in datas)
    assert all(int(L.kcemu_flate_deflate_bound(len(d), block)) == M.bound(len(d), block) for d in datas)
    if cap is None:
        cap = bound
    buf = np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    rc = fn(src.ctypes.data if len(src) else buf.ctypes.data, off.ctypes.data, n, end, block, penalty, buf.ctypes.data + GUARD, cap, out_off.ctypes.data)
    total = int(out_off[n])
    assert np.all(buf[:GUARD] == 0xA5), "bytes in front of dst were written"
    if rc != 0:
        assert np.all(buf == 0xA5), "a refused call wrote"
        return rc, None, out_off
    assert total <= cap and np.all(buf[GUARD + total:] == 0xA5), "bytes behind the output were written"
    dst = buf[GUARD:GUARD + total]
    return rc, [dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)], out_off
