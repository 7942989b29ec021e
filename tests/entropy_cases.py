"""Directed inputs for the decisions of the zstd entropy stage that depend on a histogram (huff0 buildCTable / setMaxHeight /
cTable.write, the byte FSE of the Huffman weights, fseEncoder.normalizeCount / normalizeCount2 / writeCount, blockEnc.encodeLits /
encode / genCodes).  Plain Python + numpy, seeded; nothing is searched at test time.

A case is a small tuple of parameters (CASES below); `unit(case)` regenerates its bytes.  Three families:

  lit   a LITERAL PROGRAMME: one block without sequences, so the block's literal section is the unit.  Built from a histogram
        family, a size parameter and an order seed.  Needs all_lit_entropy=True at levels 1 and 2 (a literals-only block is stored
        raw there otherwise: zstd/encoder_options.go WithAllLitEntropyCompression); levels 3 and 4 set it by default.
  per   a PERIODIC unit: `head` noise bytes, then a noise period repeated: one sequence per block whose literals are the head
        and the first period (literal-section lengths at the 16 / 17 / 1023 / 1024 boundaries, the top match-length code, short
        offsets).
  seq   a SEQUENCE PROGRAMME: a prescribed list of (literal length, match length) per sequence.  Each is a noise literal run
        followed by a snippet of the POOL; the byte in front of a snippet differs from the pool byte in front of its source and
        the byte after it from the pool byte after its source, so the match extends neither way.  The pool is a raw-content
        dictionary (DICT: 4 KiB of noise, which every match finder indexes densely — a long noise run inside the unit does not
        work, the finders' skip step grows with the literal run).

The parameters were found by tools/find_entropy_cases.py with the oracle's decision counters as the objective; `reaches` names the
decisions (oracle/kco_counters.h) a case was picked for, per level.  tests/test_entropy_decisions.py checks that they still do."""
import numpy as np

DICT_ID = 7
_DICT = None


POOL = 4096    # the dense pool: the last 4 KiB of the dictionary, where the snippets of the sequence programmes come from
FAR = 60 << 10  # noise in front of it: sources at offsets up to 64 KiB (offset codes up to 15) and long contiguous sources


def pool():
    """The raw-content dictionary of the sequence programmes: FAR bytes of noise, then the dense POOL.  (The match finders' tables
    keep the last position of a bucket: whatever the far part does to them, the pool is entered last and stays findable.)"""
    global _DICT
    if _DICT is None:
        _DICT = (bytes(np.random.default_rng(0xFA2).integers(0, 256, FAR, dtype=np.uint8))
                 + bytes(np.random.default_rng(0xD1C7).integers(0, 256, POOL, dtype=np.uint8)))
    return _DICT


# ---- literal programmes -------------------------------------------------------------------------------------------------------

def _fib(k):
    a = [1, 1]
    while len(a) < k:
        a.append(a[-1] + a[-2])
    return a[:k]


def histogram(family, a, b, rng):
    """Counts per distinct symbol (descending families are shuffled over symbol values by the caller).
    fib      a symbols with Fibonacci counts, every count times b: a tree deeper than any table log the length allows
    skew     a distinct symbols in about b bytes, geometric-ish random counts: table logs 5..8 with a forced height limit
    flat     a symbols, every count b or b + 1 at random: near-uniform weights (a > 128: more than 128 symbols)
    equal    a symbols, every count exactly b: all weights equal
    steps    a symbols in 4 plateaus of counts b, 2b, 4b, 8b: few distinct weights
    loguni   a symbols, counts 2 ** uniform(0, b / 4): code lengths spread evenly over many depths, so that the weights are
             hard for the byte FSE (huff0/huff0.go:211-229)
    eqlast   a symbols b times each and one more, of the highest value, (a // 3) * b times.  With a = 3 * 2^j the a symbols share
             one depth: all weights the description sees are equal (the last symbol's weight is implied, not described)
    A family name with a trailing "0" (fib0, equal0, ...) puts the symbols on the values 0..a-1, so that no absent symbol (weight
    0) lies between them: what the weight description (huff0/huff0.go:180) sees is then the family's weights alone.
    """
    family = family.rstrip("0")
    if family == "fib":
        return [c * b for c in _fib(a)]
    if family == "skew":
        w = rng.random(a) ** rng.integers(2, 7)
        c = np.maximum(1, np.floor(w / w.sum() * b)).astype(int)
        return [int(x) for x in c]
    if family == "flat":
        return [int(b + x) for x in rng.integers(0, 2, a)]
    if family == "equal":
        return [b] * a
    if family == "loguni":
        return [int(x) for x in np.floor(2.0 ** rng.uniform(0, b / 4, a))]
    if family == "eqlast":
        return [b] * a + [(a // 3) * b]
    if family == "steps":
        return [b << (i * 4 // a) for i in range(a)]
    raise ValueError(family)


def dyadic_unit(weights, zeros, last, b, seed):
    """A literal section whose Huffman tree has exactly weights[w - 1] symbols of weight w, PLUS one symbol of weight `last` on the
    highest symbol value (the one the weight description leaves out) and `zeros` absent symbol values in between: the histogram
    the byte FSE of the weights sees (huff0/huff0.go:197-229) is then (zeros, weights[0], weights[1], ...) exactly.  Every symbol
    of weight w occurs 2^(w-1) * b times, so the Huffman depths are forced; the weights must fill a complete code."""
    rng = np.random.default_rng([0xD7A, seed])
    ws = [w + 1 for w, h in enumerate(weights) for _ in range(h)]
    assert (sum(1 << (w - 1) for w in ws) + (1 << (last - 1))) & ((sum(1 << (w - 1) for w in ws) + (1 << (last - 1))) - 1) == 0, "not a complete code"
    vals = rng.permutation(len(ws) + zeros)[:len(ws)]
    syms = np.array(list(vals) + [len(ws) + zeros], dtype=np.uint8)
    buf = np.repeat(syms, [b << (w - 1) for w in ws] + [b << (last - 1)])
    rng.shuffle(buf)
    return buf.tobytes()


def lit_unit(family, a, b, seed):
    rng = np.random.default_rng([0x117, seed])
    counts = histogram(family, a, b, rng)
    if family == "eqlast0":
        syms = np.arange(len(counts))
    else:
        syms = rng.permutation(len(counts)) if family.endswith("0") else rng.permutation(256)[:len(counts)]
    buf = np.repeat(syms.astype(np.uint8), counts)
    rng.shuffle(buf)
    return buf.tobytes()


def reuse_unit(block_size, e, seed):
    """Two literal-only blocks over the same 192 symbols.  Block 1 (exactly block_size bytes): 64 symbols about three times as
    frequent as the other 128, which gives a tree of 64 codes of 7 bits and 128 of 8 and compresses to 92.5 %.  Block 2: the 64
    symbols 2e times, the 128 e times.  The same code lengths are optimal for these counts, so the old table's estimate equals
    the new one's and huff0 reuses it (compress.go:153-171) - but 7.5 bits per byte plus the jump table is not below wantSize
    (15/16 of the input), and the reuse is thrown away.  (The maximum count is exactly len >> 7: not "incompressible" at sight.)"""
    rng = np.random.default_rng([0x2E5, seed])
    c = block_size // 320
    f = (block_size - 128 * c) // 64
    assert 64 * f + 128 * c == block_size and 2 * c < f < 4 * c
    syms = rng.permutation(256)[:192].astype(np.uint8)
    b1 = np.repeat(syms, [f] * 64 + [c] * 128)
    b2 = np.repeat(syms, [2 * e] * 64 + [e] * 128)
    rng.shuffle(b1)
    rng.shuffle(b2)
    return b1.tobytes() + b2.tobytes()


# ---- periodic units -----------------------------------------------------------------------------------------------------------

def per_unit(head, period, total, seed):
    rng = np.random.default_rng([0x9E7, seed])
    h = rng.integers(0, 256, head, dtype=np.uint8).tobytes()
    p = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
    return (h + p * (total // period + 1))[:total]


# ---- sequence programmes ------------------------------------------------------------------------------------------------------

LL_OF_CODE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
ML_OF_CODE = list(range(32)) + [32, 34, 36, 38, 40, 44, 48, 56, 64, 80, 96, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
# (literal length / match length - 3 at which each LL / ML code starts: zstd/seqenc.go:48-112)


def code_histogram(shape, k, top, n, rng):
    """n draws over k codes out of 0..top.  shape: flat (uniform), geo (geometric), big (one dominant code, the others once or
    twice), pair (two dominant codes, the rest once), few / fewN (a quarter of the codes / N codes share the draws equally, the rest once), ends
    (codes 0 and top only, in equal parts: a long run of unused codes between them), top (the code `top` alone)."""
    codes = np.sort(rng.choice(top + 1, size=min(k, top + 1), replace=False))
    if shape == "ends":
        codes, shape = np.array([0, top]), "flat"
    if shape == "top":  # (every draw is the code `top`)
        codes, shape = np.array([top]), "flat"
    k = len(codes)
    if shape == "flat":
        w = np.ones(k)
    elif shape == "geo":
        w = 0.5 ** (np.arange(k) * rng.uniform(0.2, 1.0))
        rng.shuffle(w)
    elif shape == "big":
        w = np.full(k, 1.5 / max(n, 1))
        w[rng.integers(0, k)] = 1.0
    elif shape.startswith("few"):
        w = np.full(k, 1.0 / max(n, 1))
        big = rng.choice(k, min(k, int(shape[3:] or max(1, k // 4))), replace=False)
        w[big] = (1.0 - (k - len(big)) / max(n, 1)) / len(big)
    elif shape == "pair":
        w = np.full(k, 1.2 / max(n, 1))
        w[rng.choice(k, min(k, 2), replace=False)] = 0.5
    else:
        raise ValueError(shape)
    c = np.maximum(1, np.floor(w / w.sum() * n)).astype(int)
    out = np.repeat(codes, c)
    rng.shuffle(out)
    if len(out) < n:
        out = np.concatenate([out, rng.choice(out, n - len(out))])
    return out[:n]


def seq_unit(n, ll_shape, ll_k, ll_top, ml_shape, ml_k, ml_top, seed, alpha=256, tail=0, base=None):
    """n sequences; LL codes drawn by (ll_shape, ll_k, ll_top), ML codes by (ml_shape, ml_k, ml_top); literal bytes over `alpha`
    consecutive values from `base` on (256: noise, raw literals; 1: an RLE literal section; in between: Huffman-compressed
    literals; base 0 keeps the Huffman table description short); `tail` literal bytes at the end.  A match is at least 8 bytes (what every finder here takes at its first byte), so ML codes start at 5."""
    rng = np.random.default_rng([0x5E9, seed])
    d = pool()[FAR:]
    r = int(rng.integers(0, 257 - alpha))
    base = r if base is None else base
    llc = code_histogram(ll_shape, ll_k, ll_top, n, rng)
    mlc = code_histogram(ml_shape, ml_k, max(ml_top - 5, 0), n, rng) + 5
    out = bytearray()
    nxt = -1  # the pool byte that follows the previous snippet's source: the next byte written must differ from it
    for i in range(n):
        ll, ml = LL_OF_CODE[int(llc[i])], ML_OF_CODE[int(mlc[i])] + 3
        ml = min(ml, len(d) - 64)
        while True:
            lit = bytearray((base + rng.integers(0, alpha, ll)).astype(np.uint8).tobytes())
            p = int(rng.integers(1, len(d) - ml - 1))
            first = lit[0] if ll else d[p]
            before = lit[-1] if ll else (out[-1] if out else -1)
            # (a small literal alphabet cannot avoid a given byte by a redraw: keep the byte after the source out of it)
            if first != nxt and before != d[p - 1] and (alpha > 8 or not base <= d[p + ml] < base + alpha):
                break
        out += lit + d[p:p + ml]
        nxt = d[p + ml]
    while True:
        t = (base + rng.integers(0, alpha, tail)).astype(np.uint8).tobytes()
        if not tail or t[0] != nxt:
            break
    return bytes(out + t)


def punched_unit(n, step, seed):
    """An RLE literal section of n bytes: a contiguous piece of the dictionary's far part with every step-th byte replaced by one
    byte z.  After the first match (the unit starts with 64 untouched bytes: any of their positions finds it, and it extends back
    to the start) every further match has the same offset and is taken by the repeat-offset check, so the literals are the z alone."""
    rng = np.random.default_rng([0xB07, seed])
    d = pool()
    a = int(rng.integers(64, 4096))
    u = bytearray(d[a:a + 64 + n * step])
    z = int(rng.integers(0, 256))
    for i in range(64 + step - 1, len(u), step):
        u[i] = z  # (where the source byte is z already the match just goes on)
    return bytes(u)


def ofs_unit(n, seed, ml=16):
    """An OFFSET PROGRAMME for fseEncoder.normalizeCount2's second pass in the offset coder: n (about 250) sequences of one
    literal and ml bytes (64 for the farthest).  The first thirteen use thirteen offset codes once each - a repeat of the previous offset (code 0), a run
    of one byte (offset 1: code 2) and one offset in each of the codes 3 .. 12 and 15, the short ones first, while the unit is
    still shorter than they are - and all the others draw their offset from the codes 13 and 14, whose sources lie in the
    dictionary whatever the position.  With 16 codes in use the table log is 5: thirteen symbols of one slot each and two that
    share the rest send the first normalisation 11 slots over, and in normalizeCount2 the 237 remaining counts over 19 slots are
    above lowOne."""
    rng = np.random.default_rng([0x0F5, seed])
    d = pool()
    D = len(d)
    buf = bytearray(d)
    singles = [12, 28, 60, 124, 250, 500, 1000, 2000, 4000, 8000, "rep", 1, 60000]
    nxt = -1
    prev_off = None
    for i in range(n):
        for _ in range(1000):
            if i < len(singles):
                off = singles[i]
                if off == "rep":
                    off = prev_off
                elif off > 1:
                    off = int(off - rng.integers(0, max(1, off // 8)))
            else:
                off = int(rng.integers(8192, 32000))
            cur = len(buf) + 1  # where the match starts, after the one literal
            g = int(rng.integers(0, 256))
            src = cur - off
            if g != nxt and (off == 1 or g != buf[src - 1]):  # the match extends neither way
                break
        buf.append(g)
        for _ in range(64 if off > 32768 else ml):  # (the far one long enough for a finder whose table lost its first positions)
            buf.append(buf[len(buf) - off])  # (byte by byte: a source nearer than the length runs into what is being written)
        nxt = buf[len(buf) - off]
        prev_off = off
    while True:
        t = int(rng.integers(0, 256))
        if t != nxt:
            break
    buf.append(t)
    return bytes(buf[D:])


# ---- the committed cases ------------------------------------------------------------------------------------------------------

def unit(case):
    kind, params = case[1], case[2]
    return {"lit": lit_unit, "lit2": reuse_unit, "litw": dyadic_unit, "rle": punched_unit, "ofs": ofs_unit, "per": per_unit, "seq": seq_unit}[kind](*params)


def uses_dict(case):
    return case[1] in ("seq", "rle", "ofs")


def oracle_kw(case, level):
    """Encoder options of a case at a level (tests/oracle_lib.make_opts keywords)."""
    kw = {"level": level}
    if case[1] in ("lit", "lit2", "litw") and level < 3:
        kw["all_lit_entropy"] = True
    if uses_dict(case):
        kw.update(dict_id=DICT_ID, dict_content=pool())
    return kw


LEVELS = (1, 2, 3, 4)

# (name, family, parameters, {level: [decision names]}) — the list that tools/find_entropy_cases.py --emit prints
# BEGIN CASES
CASES = [
    ('lit0000', 'lit', ('equal0', 2, 20, 2), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 1',
            'huff0/huff0.go:180 cTable.write: maxSym < 2'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 1',
            'huff0/huff0.go:180 cTable.write: maxSym < 2'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 1',
            'huff0/huff0.go:180 cTable.write: maxSym < 2'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 1',
            'huff0/huff0.go:180 cTable.write: maxSym < 2'],
    }),
    ('lit0012', 'lit', ('fib0', 4, 1, 0), {
        1: ['zstd/blockenc.go:337 encodeLits: n < 8'],
        2: ['zstd/blockenc.go:337 encodeLits: n < 8'],
        3: ['zstd/blockenc.go:337 encodeLits: n < 8'],
        4: ['zstd/blockenc.go:337 encodeLits: n < 8'],
    }),
    ('lit0018', 'lit', ('fib0', 5, 1, 0), {
        1: ['zstd/blockenc.go:337 encodeLits: n < 32 without a dictionary table'],
        2: ['zstd/blockenc.go:337 encodeLits: n < 32 without a dictionary table'],
        3: ['zstd/blockenc.go:337 encodeLits: n < 32 without a dictionary table'],
        4: ['zstd/blockenc.go:337 encodeLits: n < 32 without a dictionary table'],
    }),
    ('lit0036', 'lit', ('fib0', 8, 1, 0), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 5',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 5',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by output size (fse/compress.go:18)',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, odd maxSym'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 5',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 5',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by output size (fse/compress.go:18)',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, odd maxSym',
            'zstd/blockenc.go:481 encode: saved < 16'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 5',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 5',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by output size (fse/compress.go:18)',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, odd maxSym',
            'zstd/blockenc.go:481 encode: saved < 16'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 5',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 5',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by output size (fse/compress.go:18)',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, odd maxSym',
            'zstd/blockenc.go:481 encode: saved < 16'],
    }),
    ('lit0108', 'lit', ('fib', 10, 1, 10), {
        1: ['huff0/compress.go:609 setMaxHeight: entered, maxNbBits 8'],
        4: ['huff0/compress.go:609 setMaxHeight: entered, maxNbBits 8'],
    }),
    ('lit0735', 'lit', ('skew', 10, 80, 534), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 7',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 7',
            'huff0/compress.go:609 setMaxHeight: excess depth 1'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 7',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 7'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 7',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 7'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 7',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 7'],
    }),
    ('lit1721', 'lit', ('skew0', 8, 1092, 20), {
        2: ['zstd/blockenc.go:481 encode: nSeq exactly 127'],
    }),
    ('lit1730', 'lit', ('skew0', 3, 1261, 29), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 2',
            'huff0/huff0.go:180 cTable.write: FSE returned ErrUseRLE'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 2',
            'huff0/huff0.go:180 cTable.write: FSE returned ErrUseRLE',
            'll zstd/fse_encoder.go:488 writeCount: zero run >= 3'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 2',
            'huff0/huff0.go:180 cTable.write: FSE returned ErrUseRLE',
            'll zstd/fse_encoder.go:488 writeCount: zero run >= 3'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 2',
            'huff0/huff0.go:180 cTable.write: FSE returned ErrUseRLE'],
    }),
    ('lit1933', 'lit', ('skew0', 4, 38, 232), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 3',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by maxCount (fse/compress.go:18)',
            'zstd/blockenc.go:481 encode: saved < 16'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 3',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by maxCount (fse/compress.go:18)',
            'zstd/blockenc.go:337,481 literals: 17 literals, 1X'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 3',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by maxCount (fse/compress.go:18)',
            'zstd/blockenc.go:337,481 literals: 17 literals, 1X'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 3',
            'huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by maxCount (fse/compress.go:18)'],
    }),
    ('lit1944', 'lit', ('skew0', 13, 287, 243), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 6',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 6',
            'huff0/huff0.go:180 cTable.write: FSE succeeded but was not smaller',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, even maxSym',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 3 bytes',
            'zstd/blockenc.go:831 genCodes: highest OF code < 8'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 6',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 6',
            'huff0/compress.go:609 setMaxHeight: excess depth 3',
            'huff0/huff0.go:180 cTable.write: FSE succeeded but was not smaller',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, even maxSym',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 3 bytes',
            'zstd/blockenc.go:831 genCodes: highest OF code < 8'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 6',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 6',
            'huff0/huff0.go:180 cTable.write: FSE succeeded but was not smaller',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, even maxSym',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 3 bytes',
            'zstd/blockenc.go:831 genCodes: highest OF code < 8'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 6',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 6',
            'huff0/compress.go:609 setMaxHeight: excess depth 3',
            'huff0/huff0.go:180 cTable.write: FSE succeeded but was not smaller',
            'huff0/huff0.go:180 cTable.write: raw 4-bit weights, even maxSym',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:831 genCodes: highest OF code < 8'],
    }),
    ('lit1960', 'lit', ('skew0', 11, 1903, 259), {
        1: ['zstd/blockenc.go:481 encode: nSeq exactly 127'],
    }),
    ('lit2242', 'lit', ('skew', 11, 35, 41), {
        1: ['zstd/blockenc.go:337 encodeLits: compressed no smaller than raw with both headers'],
        2: ['zstd/blockenc.go:337 encodeLits: compressed no smaller than raw with both headers'],
        3: ['zstd/blockenc.go:337 encodeLits: compressed no smaller than raw with both headers'],
        4: ['zstd/blockenc.go:337 encodeLits: compressed no smaller than raw with both headers'],
    }),
    ('lit2505', 'lit', ('eqlast0', 192, 5, 192), {
        1: ['huff0/huff0.go:180 cTable.write: more than 128 symbols, ErrIncompressible'],
        2: ['huff0/huff0.go:180 cTable.write: more than 128 symbols, ErrIncompressible'],
        3: ['huff0/huff0.go:180 cTable.write: more than 128 symbols, ErrIncompressible'],
        4: ['huff0/huff0.go:180 cTable.write: more than 128 symbols, ErrIncompressible'],
    }),
    ('lit2696', 'lit', ('loguni', 80, 55, 190), {
        1: ['huff0/compress.go:609 setMaxHeight: entered, maxNbBits 10',
            'huff0/compress.go:609 setMaxHeight: excess depth >= 4'],
        3: ['huff0/compress.go:609 setMaxHeight: excess depth 3'],
        4: ['huff0/compress.go:43 compress: reuse possible, new table built'],
    }),
    ('litw2711', 'litw', ((2, 1, 2, 2, 2, 2, 2), 1, 3, 3, 2), {
        1: ['fse/compress.go:557 normalizeCount2: entered',
            'fse/compress.go:557 normalizeCount2: proportional exit'],
        2: ['fse/compress.go:557 normalizeCount2: entered',
            'fse/compress.go:557 normalizeCount2: proportional exit'],
        3: ['fse/compress.go:557 normalizeCount2: entered',
            'fse/compress.go:557 normalizeCount2: proportional exit'],
        4: ['fse/compress.go:557 normalizeCount2: entered',
            'fse/compress.go:557 normalizeCount2: proportional exit'],
    }),
    ('lit22717', 'lit2', (131072, 100, 100), {
        1: ['huff0/compress.go:43 compress: reuse taken',
            'huff0/compress.go:43 compress: reuse taken, then >= wantSize'],
        2: ['huff0/compress.go:43 compress: reuse taken',
            'huff0/compress.go:43 compress: reuse taken, then >= wantSize'],
        3: ['huff0/compress.go:43 compress: reuse taken',
            'huff0/compress.go:43 compress: reuse taken, then >= wantSize'],
        4: ['huff0/compress.go:43 compress: reuse taken',
            'huff0/compress.go:43 compress: reuse taken, then >= wantSize'],
    }),
    ('per2719', 'per', (0, 1, 40, 1), {
        1: ['zstd/blockenc.go:481 encode: single-sequence RLE block'],
        2: ['zstd/blockenc.go:481 encode: single-sequence RLE block'],
        3: ['zstd/blockenc.go:481 encode: single-sequence RLE block'],
        4: ['zstd/blockenc.go:481 encode: single-sequence RLE block'],
    }),
    ('per2737', 'per', (0, 16, 40, 16), {
        1: ['zstd/blockenc.go:337,481 literals: 16 literals, no entropy coder'],
        2: ['zstd/blockenc.go:337,481 literals: 16 literals, no entropy coder'],
        3: ['zstd/blockenc.go:337,481 literals: 16 literals, no entropy coder'],
        4: ['zstd/blockenc.go:337,481 literals: 16 literals, no entropy coder'],
    }),
    ('per2757', 'per', (0, 1023, 140000, 1023), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 9',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 9',
            'huff0/compress.go:609 setMaxHeight: inner for, break on highTotal <= lowTotal',
            'll zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'ml zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'of zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 1 byte',
            'zstd/blockenc.go:337,481 literals: 1023 literals, 1X',
            'zstd/blockenc.go:831 genCodes: highest ML code >= 43'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 9',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 9',
            'huff0/compress.go:609 setMaxHeight: inner for, break on highTotal <= lowTotal',
            'll zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'ml zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'of zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 1 byte',
            'zstd/blockenc.go:337,481 literals: 1023 literals, 1X',
            'zstd/blockenc.go:831 genCodes: highest LL code >= 25',
            'zstd/blockenc.go:831 genCodes: highest ML code 52 (top)',
            'zstd/blockenc.go:831 genCodes: highest ML code >= 43'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 9',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 9',
            'huff0/compress.go:609 setMaxHeight: excess depth 2',
            'huff0/compress.go:609 setMaxHeight: inner for, break on highTotal <= lowTotal',
            'ml zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'of zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 1 byte',
            'zstd/blockenc.go:337,481 literals: 1023 literals, 1X',
            'zstd/blockenc.go:831 genCodes: highest LL code >= 25',
            'zstd/blockenc.go:831 genCodes: highest ML code 52 (top)',
            'zstd/blockenc.go:831 genCodes: highest ML code >= 43'],
        4: ['huff0/compress.go:609 setMaxHeight: excess depth 2',
            'huff0/compress.go:609 setMaxHeight: inner for, break on highTotal <= lowTotal',
            'll zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'ml zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'of zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 1 byte',
            'zstd/blockenc.go:337,481 literals: 1023 literals, 1X',
            'zstd/blockenc.go:831 genCodes: highest LL code >= 25',
            'zstd/blockenc.go:831 genCodes: highest ML code 52 (top)',
            'zstd/blockenc.go:831 genCodes: highest ML code >= 43'],
    }),
    ('per2848', 'per', (65536, 300, 131072, 1), {
        2: ['zstd/blockenc.go:831 genCodes: highest LL code 35 (top)'],
        3: ['zstd/blockenc.go:831 genCodes: highest LL code 35 (top)'],
        4: ['zstd/blockenc.go:831 genCodes: highest LL code 35 (top)'],
    }),
    ('seq2850', 'seq', (43, 'flat', 8, 15, 'flat', 43, 47, 1), {
        1: ['ml zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
        2: ['ml zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
        3: ['ml zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
    }),
    ('seq2854', 'seq', (22, 'flat', 22, 24, 'flat', 3, 12, 5), {
        1: ['ll zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
        2: ['ll zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
        3: ['ll zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
        4: ['ll zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin'],
    }),
    ('seq2861', 'seq', (127, 'geo', 12, 20, 'geo', 12, 30, 2), {
        1: ['zstd/blockenc.go:481 encode: nSeq exactly 128'],
        2: ['zstd/blockenc.go:481 encode: nSeq exactly 128'],
        3: ['zstd/blockenc.go:481 encode: nSeq exactly 127'],
        4: ['zstd/blockenc.go:481 encode: nSeq exactly 127'],
    }),
    ('seq2863', 'seq', (128, 'geo', 12, 20, 'geo', 12, 30, 1), {
        3: ['zstd/blockenc.go:481 encode: nSeq exactly 128'],
        4: ['zstd/blockenc.go:481 encode: nSeq exactly 128'],
    }),
    ('seq2971', 'seq', (43, 'big', 7, 15, 'flat', 8, 10, 2, 256, 0), {
        1: ["huff0/compress.go:609 setMaxHeight: the rank's last position is 0"],
        2: ["huff0/compress.go:609 setMaxHeight: the rank's last position is 0"],
        3: ["huff0/compress.go:609 setMaxHeight: the rank's last position is 0"],
        4: ["huff0/compress.go:609 setMaxHeight: the rank's last position is 0",
            'll zstd/fse_encoder.go:488 writeCount: zero run >= 3'],
    }),
    ('seq3056', 'seq', (600, 'pair', 22, 8, 'big', 8, 31, 3, 16, 7), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 10',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 7'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 10',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 10',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 7'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 10',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 10',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 4 bytes'],
    }),
    ('seq3089', 'seq', (20, 'top', 1, 1, 'top', 1, 13, 0, 1), {
        1: ['huff0/compress.go:43 compress: ErrUseRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: RLE, 2 bytes'],
        2: ['huff0/compress.go:43 compress: ErrUseRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: RLE, 2 bytes'],
        3: ['huff0/compress.go:43 compress: ErrUseRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: RLE, 2 bytes'],
        4: ['huff0/compress.go:43 compress: ErrUseRLE',
            'zstd/blockenc.go:150 literalsHeader.setSize: RLE, 2 bytes'],
    }),
    ('seq3095', 'seq', (3, 'top', 1, 0, 'top', 1, 13, 0, 8, 17, 0), {
        1: ['huff0/compress.go:457 buildCTable: actualTableLog 4',
            'zstd/blockenc.go:337,481 literals: 17 literals, 1X'],
        2: ['huff0/compress.go:457 buildCTable: actualTableLog 4'],
        3: ['huff0/compress.go:457 buildCTable: actualTableLog 4'],
        4: ['huff0/compress.go:457 buildCTable: actualTableLog 4',
            'zstd/blockenc.go:337,481 literals: 17 literals, 1X'],
    }),
    ('seq3462', 'seq', (200, 'ends', 2, 29, 'ends', 2, 36, 29), {
        1: ['ll zstd/fse_encoder.go:488 writeCount: zero run >= 24'],
        3: ['ll zstd/fse_encoder.go:488 writeCount: zero run >= 24'],
        4: ['ll zstd/fse_encoder.go:488 writeCount: zero run >= 24'],
    }),
    ('seq3472', 'seq', (255, 'few2', 16, 15, 'few2', 16, 20, 1), {
        1: ['ll zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass'],
    }),
    ('seq3788', 'seq', (511, 'few2', 27, 26, 'few2', 27, 31, 3), {
        1: ['huff0/compress.go:43 compress: incompressible by maxCount',
            'll zstd/fse_encoder.go:334 normalizeCount2: entered',
            'll zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'ml zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 3 bytes'],
        2: ['huff0/compress.go:43 compress: incompressible by maxCount',
            'll zstd/fse_encoder.go:334 normalizeCount2: entered',
            'll zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'll zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'ml zstd/fse_encoder.go:334 normalizeCount2: entered',
            'ml zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'ml zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 3 bytes'],
        3: ['huff0/compress.go:43 compress: incompressible by maxCount',
            'll zstd/fse_encoder.go:334 normalizeCount2: entered',
            'll zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'll zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'ml zstd/fse_encoder.go:334 normalizeCount2: entered',
            'ml zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'ml zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 3 bytes'],
        4: ['huff0/compress.go:43 compress: incompressible by maxCount',
            'll zstd/fse_encoder.go:334 normalizeCount2: entered',
            'll zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'll zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'ml zstd/fse_encoder.go:334 normalizeCount2: entered',
            'ml zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'ml zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 3 bytes'],
    }),
    ('rle3884', 'rle', (4200, 12, 0), {
        1: ['zstd/blockenc.go:150 literalsHeader.setSize: RLE, 3 bytes'],
        2: ['zstd/blockenc.go:150 literalsHeader.setSize: RLE, 3 bytes'],
        3: ['zstd/blockenc.go:150 literalsHeader.setSize: RLE, 3 bytes'],
        4: ['zstd/blockenc.go:150 literalsHeader.setSize: RLE, 3 bytes'],
    }),
    ('ofs3897', 'ofs', (250, 0), {
        1: ['huff0/compress.go:229 compress1X',
            'huff0/compress.go:43 compress: new table, then >= wantSize',
            'huff0/compress.go:457 buildCTable: actualTableLog 8',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'll zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 24',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'of zstd/fse_encoder.go:334 normalizeCount2: entered',
            'of zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'of zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 2 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code < 16',
            'zstd/blockenc.go:831 genCodes: highest ML code 32..42',
            'zstd/blockenc.go:831 genCodes: highest OF code 8..15'],
        2: ['huff0/compress.go:229 compress1X',
            'huff0/compress.go:43 compress: new table, then >= wantSize',
            'huff0/compress.go:457 buildCTable: actualTableLog 8',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 8',
            'huff0/compress.go:609 setMaxHeight: excess depth 1',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 24',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'of zstd/fse_encoder.go:334 normalizeCount2: entered',
            'of zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'of zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 2 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code < 16',
            'zstd/blockenc.go:831 genCodes: highest ML code 32..42',
            'zstd/blockenc.go:831 genCodes: highest OF code 8..15'],
        3: ['huff0/compress.go:229 compress1X',
            'huff0/compress.go:43 compress: new table, then >= wantSize',
            'huff0/compress.go:457 buildCTable: actualTableLog 8',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 8',
            'll zstd/fse_encoder.go:259 normalizeCount: useRLE',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 24',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'of zstd/fse_encoder.go:334 normalizeCount2: entered',
            'of zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'of zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 2 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code < 16',
            'zstd/blockenc.go:831 genCodes: highest ML code 32..42',
            'zstd/blockenc.go:831 genCodes: highest OF code 8..15'],
        4: ['huff0/compress.go:43 compress: new table, then >= wantSize',
            'huff0/compress.go:457 buildCTable: actualTableLog 8',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'll zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'll zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 24',
            'ml zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'of zstd/fse_encoder.go:334 normalizeCount2: entered',
            'of zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'of zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 5',
            'zstd/blockenc.go:150 literalsHeader.setSize: raw, 2 bytes',
            'zstd/blockenc.go:831 genCodes: highest ML code 32..42',
            'zstd/blockenc.go:831 genCodes: highest OF code 8..15'],
    }),
    ('seq3906', 'seq', (4, 'flat', 1, 0, 'flat', 3, 30, 1024, 256, 1024), {
        1: ['zstd/blockenc.go:337,481 literals: 1024 literals, 4X'],
        2: ['zstd/blockenc.go:337,481 literals: 1024 literals, 4X'],
        3: ['zstd/blockenc.go:337,481 literals: 1024 literals, 4X'],
        4: ['zstd/blockenc.go:337,481 literals: 1024 literals, 4X'],
    }),
    ('seq3916', 'seq', (4000, 'geo', 10, 24, 'geo', 10, 30, 0, 12), {
        1: ['huff0/compress.go:269 compress4X',
            'huff0/compress.go:43 compress: reuse possible, new table built',
            'huff0/compress.go:457 buildCTable: actualTableLog 11',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 11',
            'huff0/compress.go:609 setMaxHeight: excess depth 2',
            'huff0/compress.go:609 setMaxHeight: excess depth 3',
            'huff0/compress.go:609 setMaxHeight: inner for, break on lowPos == noSymbol',
            'huff0/compress.go:609 setMaxHeight: lower rank seeded (rankLast[n-1] == noSymbol)',
            'huff0/compress.go:609 setMaxHeight: rank emptied by the nBits mismatch',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] == noSymbol',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] set',
            'huff0/compress.go:609 setMaxHeight: totalCost < 0 loop',
            'huff0/compress.go:609 setMaxHeight: totalCost > 0 loop',
            'huff0/compress.go:609 setMaxHeight: upward skip over empty ranks',
            'huff0/huff0.go:180 cTable.write: FSE of the weights used',
            'll zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'll zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'll zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'll zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'ml zstd/fse_encoder.go:334 normalizeCount2: entered',
            'ml zstd/fse_encoder.go:334 normalizeCount2: proportional exit',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'ml zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'ml zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'of zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'of zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 4 bytes',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 5 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code 16..24',
            'zstd/blockenc.go:831 genCodes: highest LL code >= 25',
            'zstd/blockenc.go:831 genCodes: highest ML code < 32',
            'zstd/blockenc.go:831 genCodes: highest OF code >= 16'],
        2: ['huff0/compress.go:269 compress4X',
            'huff0/compress.go:43 compress: reuse possible, new table built',
            'huff0/compress.go:457 buildCTable: actualTableLog 10',
            'huff0/compress.go:457 buildCTable: actualTableLog 11',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 10',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 11',
            'huff0/compress.go:609 setMaxHeight: excess depth 2',
            'huff0/compress.go:609 setMaxHeight: excess depth >= 4',
            'huff0/compress.go:609 setMaxHeight: inner for, break on lowPos == noSymbol',
            'huff0/compress.go:609 setMaxHeight: lower rank seeded (rankLast[n-1] == noSymbol)',
            'huff0/compress.go:609 setMaxHeight: rank emptied by the nBits mismatch',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] == noSymbol',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] set',
            'huff0/compress.go:609 setMaxHeight: totalCost < 0 loop',
            'huff0/compress.go:609 setMaxHeight: totalCost > 0 loop',
            'huff0/compress.go:609 setMaxHeight: upward skip over empty ranks',
            'huff0/huff0.go:180 cTable.write: FSE of the weights used',
            'll zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'll zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'll zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'll zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'ml zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'ml zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 7',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'of zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'of zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 4 bytes',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 5 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code 16..24',
            'zstd/blockenc.go:831 genCodes: highest ML code < 32',
            'zstd/blockenc.go:831 genCodes: highest OF code >= 16'],
        3: ['huff0/compress.go:269 compress4X',
            'huff0/compress.go:43 compress: reuse possible, new table built',
            'huff0/compress.go:457 buildCTable: actualTableLog 11',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 11',
            'huff0/compress.go:609 setMaxHeight: excess depth 1',
            'huff0/compress.go:609 setMaxHeight: excess depth >= 4',
            'huff0/compress.go:609 setMaxHeight: inner for, break on lowPos == noSymbol',
            'huff0/compress.go:609 setMaxHeight: lower rank seeded (rankLast[n-1] == noSymbol)',
            'huff0/compress.go:609 setMaxHeight: rank emptied by the nBits mismatch',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] == noSymbol',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] set',
            'huff0/compress.go:609 setMaxHeight: totalCost < 0 loop',
            'huff0/compress.go:609 setMaxHeight: totalCost > 0 loop',
            'huff0/compress.go:609 setMaxHeight: upward skip over empty ranks',
            'huff0/huff0.go:180 cTable.write: FSE of the weights used',
            'll zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'll zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'll zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'll zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'ml zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'ml zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 6',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'of zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'of zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 4 bytes',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 5 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code 16..24',
            'zstd/blockenc.go:831 genCodes: highest ML code < 32',
            'zstd/blockenc.go:831 genCodes: highest OF code >= 16'],
        4: ['huff0/compress.go:229 compress1X',
            'huff0/compress.go:269 compress4X',
            'huff0/compress.go:457 buildCTable: actualTableLog 11',
            'huff0/compress.go:457 buildCTable: actualTableLog 9',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 11',
            'huff0/compress.go:609 setMaxHeight: entered, maxNbBits 9',
            'huff0/compress.go:609 setMaxHeight: excess depth 1',
            'huff0/compress.go:609 setMaxHeight: excess depth >= 4',
            'huff0/compress.go:609 setMaxHeight: inner for, break on lowPos == noSymbol',
            'huff0/compress.go:609 setMaxHeight: lower rank seeded (rankLast[n-1] == noSymbol)',
            'huff0/compress.go:609 setMaxHeight: rank emptied by the nBits mismatch',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] == noSymbol',
            'huff0/compress.go:609 setMaxHeight: repay, rankLast[1] set',
            'huff0/compress.go:609 setMaxHeight: totalCost < 0 loop',
            'huff0/compress.go:609 setMaxHeight: totalCost > 0 loop',
            'huff0/compress.go:609 setMaxHeight: upward skip over empty ranks',
            'huff0/huff0.go:180 cTable.write: FSE of the weights used',
            'll zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'll zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'll zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'ml zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'ml zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'ml zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'ml zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'ml zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol',
            'of zstd/fse_encoder.go:259 normalizeCount: small proba rounded up',
            'of zstd/fse_encoder.go:429 optimalTableLog: tableLog 8',
            'of zstd/fse_encoder.go:488 writeCount: cnt >= threshold',
            'of zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol',
            'of zstd/fse_encoder.go:488 writeCount: zero run >= 3',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 3 bytes',
            'zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 5 bytes',
            'zstd/blockenc.go:831 genCodes: highest LL code 16..24',
            'zstd/blockenc.go:831 genCodes: highest LL code < 16',
            'zstd/blockenc.go:831 genCodes: highest ML code < 32',
            'zstd/blockenc.go:831 genCodes: highest OF code >= 16'],
    }),
]
# END CASES
