"""Inputs of the zlib tests, shared by the model's own test (test_zlib_model.py), the emulator suite (test_emu_zlib.py) and the GPU
suite (test_gpu_zlib.py).  A case is a flate_cases.Case with fmt "zlib"; every case is judged by tests/zlib_model.py, nothing here
knows what the device answers.

    cases()        the directed ones: every header rule, truncation at every byte, FDICT, trailers, the reference's own vectors
    mutations()    480 seeded mutations of six valid streams: one random bit, a truncation, one bit in the first 16 bytes, an insertion
    generated()    the 2000 raw-DEFLATE streams of flate_cases.generated() wrapped as zlib
    adler_sweep()  (first, case): payloads for the write pass's Adler-32, each to start `first` bytes behind a word boundary in dst
    verdict(case)  what the DEVICE is to answer: the model's (bytes, class, consumed) with stale_tables=False, computed once per case
"""
import json
import os
import random
import struct
import zlib

import flate_cases as FC
import flate_model as M
import zlib_model as Z
from flate_cases import BW, fixed_block, stored_block

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def C(name, data, dict=b""):
    return FC.C(name, data, fmt="zlib", dict=dict)


_verdicts, _fired = {}, {}


def verdict(c, stale_tables=False):
    k = (c.data, c.dict, stale_tables)
    if k not in _verdicts:
        _verdicts[k] = Z.inflate(c.data, c.dict, stale_tables=stale_tables)
        _fired[k] = frozenset(M.fired)
    return _verdicts[k]


def fired(c, stale_tables=False):
    verdict(c, stale_tables)
    return _fired[(c.data, c.dict, stale_tables)]


def _warm_one(job):
    c, stale = job
    return verdict(c, stale), fired(c, stale)


def warm(cases, stale_tables=False):
    """The verdicts of many cases in forked children (wall-clock time of the CPU suite only; never once a GPU is open)."""
    import multiprocessing as mp
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return
    todo = [c for c in cases if (c.data, c.dict, stale_tables) not in _verdicts]
    procs = min(8, os.cpu_count() or 1, int(os.environ.get("KC_EMU_PROCS", "8")))
    if procs <= 1 or len(todo) < 200:
        return
    with mp.get_context("fork").Pool(procs) as pool:
        for c, (v, f) in zip(todo, pool.map(_warm_one, [(c, stale_tables) for c in todo], chunksize=25)):
            _verdicts[(c.data, c.dict, stale_tables)], _fired[(c.data, c.dict, stale_tables)] = v, f


def header(cmf=0x78, flevel=2, fdict=False, fcheck=None):
    """CMF and FLG; fcheck None: the value that makes the header divisible by 31."""
    flg = (flevel << 6) | (0x20 if fdict else 0)
    if fcheck is None:
        fcheck = (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, flg | fcheck])


def wrap(body, payload, dictid=None, trailer=None, **kw):
    """header [+ DICTID] + body + the big-endian Adler-32 of payload (or `trailer`, four bytes)."""
    h = header(fdict=dictid is not None, **kw)
    if dictid is not None:
        h += struct.pack(">I", dictid)
    return h + body + (struct.pack(">I", zlib.adler32(payload)) if trailer is None else trailer)


_TEXT = b"the quick brown fox jumps over the lazy dog; the lazy dog naps, the quick fox jumps. " * 3
_DICT = b"the quick brown fox jumps over the lazy dog"
_BIG_DICT = bytes((i * 13 + (i >> 9) * 7 + 5) & 255 for i in range(40000))   # longer than the window: its id is not its tail's


def _bodies():
    """(kind, payload, body): a stored, a fixed and a dynamic DEFLATE stream."""
    hello = b"hello"
    fixed = FC._deflate(b"hello, hello, hello!", 6, zlib.Z_FIXED)
    rng = random.Random(0x2D1)
    skewed = bytes(rng.choice(b"aaaaaaaaaaaabbbbbbccccdde ") for _ in range(240))   # few symbols, no repeats worth a match
    dyn = FC._deflate(skewed, 6, zlib.Z_HUFFMAN_ONLY)
    assert (fixed[0] >> 1) & 3 == 1 and (dyn[0] >> 1) & 3 == 2
    return [("stored", hello, stored_block(BW(), hello).bytes()), ("fixed", b"hello, hello, hello!", fixed), ("dynamic", skewed, dyn)]


def _headers():
    hello = b"hello"
    body = stored_block(BW(), hello).bytes()
    out = []
    for cinfo in range(16):   # reader.go:151: above 7 is ErrHeader; at or below it the value is not used
        out.append(C("hdr/cinfo-%d" % cinfo, wrap(body, hello, cmf=cinfo << 4 | 8)))
    for cm in (0, 7, 9, 15):
        out.append(C("hdr/cm-%d" % cm, wrap(body, hello, cmf=0x70 | cm)))
    right = header()[1] & 31
    for fc in range(32):      # every value of FCHECK: the right one alone makes the header divisible by 31
        out.append(C("hdr/fcheck-%d%s" % (fc, "-right" if fc == right else ""), wrap(body, hello, fcheck=fc)))
    for fl in range(4):
        out.append(C("hdr/flevel-%d" % fl, wrap(body, hello, flevel=fl)))
    return out


def _truncations():
    out = []
    for kind, payload, body in _bodies():   # header, body and trailer, cut at every byte
        full = wrap(body, payload)
        out.append(C("cut/%s-whole" % kind, full))
        out += [C("cut/%s-%d" % (kind, k), full[:k]) for k in range(len(full))]
    body = FC._deflate(_TEXT[:60], 9, zdict=_DICT)
    full = wrap(body, _TEXT[:60], dictid=zlib.adler32(_DICT))   # header, DICTID, body, trailer
    out += [C("cut/fdict-%d" % k, full[:k], dict=_DICT) for k in range(len(full))]
    return out


def _fdict():
    payload = _TEXT[:100]
    body = FC._deflate(payload, 9, zdict=_DICT)
    plain = FC._deflate(payload, 9)
    big_payload = _BIG_DICT[100:400] + b"!" + _BIG_DICT[39000:39900]    # matches into the window's far and near end
    big_body = FC._deflate(big_payload, 9, zdict=_BIG_DICT)
    assert zlib.adler32(_BIG_DICT) != zlib.adler32(_BIG_DICT[-32768:])
    into_dict = fixed_block(BW(), [65, (3, 17)]).bytes()              # a match that reaches 16 bytes in front of the output
    return [C("fdict/right", wrap(body, payload, dictid=zlib.adler32(_DICT)), dict=_DICT),
            C("fdict/right-40000", wrap(big_body, big_payload, dictid=zlib.adler32(_BIG_DICT)), dict=_BIG_DICT),
            C("fdict/id-of-the-tail-40000", wrap(big_body, big_payload, dictid=zlib.adler32(_BIG_DICT[-32768:])), dict=_BIG_DICT),
            C("fdict/wrong", wrap(body, payload, dictid=zlib.adler32(_DICT)), dict=_DICT[:-1]),
            C("fdict/none-given-id-1", wrap(plain, payload, dictid=1)),            # adler32(nil) = 1: accepted, no history
            C("fdict/none-given-id-1-match-into-it", wrap(into_dict, b"", dictid=1)),
            C("fdict/none-given-id-other", wrap(body, payload, dictid=zlib.adler32(_DICT))),
            C("fdict/given-stream-has-none", wrap(plain, payload), dict=_DICT),    # the dictionary is ignored
            C("fdict/given-stream-has-none-match-into-it", wrap(into_dict, b"AAAA"), dict=b"dictionary tail..")]


def _trailers():
    payload = _TEXT[:77]
    body = FC._deflate(payload, 6)
    a = zlib.adler32(payload)
    assert a >> 16 != a & 0xFFFF and struct.pack("<I", a) != struct.pack(">I", a)
    second = wrap(stored_block(BW(), b"second").bytes(), b"second")
    # the input ends inside the extra bit of a length code (six 9-bit literals, then symbol 265: 64 bits): flate's raw io.EOF (R3)
    r3 = fixed_block(BW(), [200] * 6, eob=False).code(FC.FIXED[265]).bytes()
    assert len(r3) == 8
    return [C("trailer/one-bit", wrap(body, payload, trailer=struct.pack(">I", a ^ 0x00010000))),
            C("trailer/little-endian", wrap(body, payload, trailer=struct.pack("<I", a))),
            C("trailer/s1-s2-swapped", wrap(body, payload, trailer=struct.pack(">I", (a & 0xFFFF) << 16 | a >> 16))),
            C("trailer/excess-1", wrap(body, payload) + b"\x00"),
            C("trailer/excess-4", wrap(body, payload) + b"\xff\xff\xff\xff"),
            C("trailer/excess-a-second-stream", wrap(body, payload) + second),
            C("trailer/empty-payload", wrap(b"\x03\x00", b"")),
            C("trailer/empty-payload-stored", wrap(stored_block(BW(), b"").bytes(), b"")),
            C("trailer/body-ends-by-raw-eof", header() + r3)]


def vectors():
    rows = json.load(open(os.path.join(GOLD, "zlib_vectors.json")))["rows"]
    return [(C("vec/" + r["desc"], bytes.fromhex(r["stream"]), dict=bytes.fromhex(r["dict"] or "")), bytes.fromhex(r["want"]), r["class"]) for r in rows]


def cases():
    return _headers() + _truncations() + _fdict() + _trailers() + [c for c, _, _ in vectors()]


def mutations():
    """480 seeded mutations of flate_cases.bases() wrapped as zlib — one random bit, a truncation, one bit in the first 16 bytes (the
    header and the first block's), one inserted byte — with flate_cases.mutations()'s discipline: one random.Random, base k % 6, kind
    (k // 6) % 4."""
    rng = random.Random(0x21B0DEF)
    bs, plain = FC.bases()
    out = []
    for k in range(480):
        i = k % 6
        b = bytearray(wrap(bs[i], plain[i]))
        kind = (k // 6) % 4
        if kind == 0:
            p = rng.randrange(len(b) * 8)
            b[p >> 3] ^= 1 << (p & 7)
        elif kind == 1:
            b = b[:rng.randrange(len(b))]
        elif kind == 2:
            p = rng.randrange(16 * 8)
            b[p >> 3] ^= 1 << (p & 7)
        else:
            b.insert(rng.randrange(len(b) + 1), rng.randrange(256))
        out.append(C("zmut/%d-base%d-kind%d" % (k, i, kind), b))
    return out


_gen_cache = {}


def generated(seed=FC.GEN_SEED, n=2000):
    """flate_cases.generated(seed, n) wrapped: 78 9c + body + the Adler-32 of what the flate model decodes from the body alone, or, for
    a case with a dictionary, 78 bb + DICTID + body + that Adler-32.  The model then judges the wrapped stream afresh: the appended
    bytes change some parses (a body that ran into the input's end now reads the trailer as DEFLATE)."""
    if (seed, n) not in _gen_cache:
        fl = FC.generated(seed, n)
        FC.warm(fl)
        out = []
        for c in fl:
            payload = FC.verdict(c)[0]
            out.append(C("z" + c.name, wrap(c.data, payload, dictid=zlib.adler32(c.dict) if c.dict else None), dict=c.dict))
        _gen_cache[(seed, n)] = out
    return _gen_cache[(seed, n)]


SWEEP_LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 5551, 5552, 5553, 65520, 65521, 65522, 65535, 65536)
SWEEP_FILLS = ("ff", "00", "rand")
ADLER_WRAPS = "adler/len65521-ff"   # 65521 bytes of 0xFF: s1 = 1 + 65521 * 255 = 1 and s2 = 0 mod 65521: the empty stream's 0x00000001


def _deflate_any(payload, fill):
    """0xFF / 0x00: what zlib writes (long matches at distance 1); random bytes: stored blocks."""
    c = zlib.compressobj(6 if fill != "rand" else 0, zlib.DEFLATED, -15)
    return c.compress(payload) + c.flush()


def sweep_payload(n, fill):
    if fill == "rand":
        return random.Random(0xAD1E2 + n).randbytes(n)
    return bytes([0xFF if fill == "ff" else 0]) * n


def adler_sweep(lengths=SWEEP_LENGTHS):
    """-> [(first, case)]: every length x fill x first in (1, 2, 3), and a twin of each whose trailer has one bit flipped (CHECKSUM,
    the planned range zero-filled).  `first`: the bytes in dst between a word boundary and the case's range (layout() below)."""
    out = []
    for n in lengths:
        for fill in SWEEP_FILLS:
            payload = sweep_payload(n, fill)
            body = _deflate_any(payload, fill)
            a = zlib.adler32(payload)
            for first in (1, 2, 3):
                name = "adler/len%d-%s" % (n, fill)
                out.append((first, C("%s-first%d" % (name, first), wrap(body, payload))))
                bit = 1 << ((n * 7 + first * 11) % 32)
                out.append((first, C("%s-first%d-bad" % (name, first), wrap(body, payload, trailer=struct.pack(">I", a ^ bit)))))
    return out


def head(k):
    """A stream of k decoded bytes, to shift what follows it in dst."""
    p = bytes(range(65, 65 + k))
    return C("head/%d" % k, wrap(stored_block(BW(), p).bytes(), p))


def layout(sweep, sizes):
    """One batch for the whole sweep: in front of every case a head of 1..4 bytes so that the case's range begins `first` bytes behind
    a multiple of 4 of the batch's output (sizes[i]: the planned bytes of sweep case i).  -> (cases of the batch, index of every
    sweep case in it)."""
    batch, at, cur = [], [], 0
    for (first, c), size in zip(sweep, sizes):
        k = (first - cur) % 4 or 4
        batch.append(head(k))
        cur += k
        assert cur % 4 == first % 4
        at.append(len(batch))
        batch.append(c)
        cur += size
    return batch, at


def families():
    return [("directed", cases()), ("zmut", mutations()), ("generated", generated())]


def batches(cs):
    """cs grouped into batches that share their dictionary: [(dict, [cases])]."""
    return [(d, v) for _, d, _, v in FC.batches(cs)]
