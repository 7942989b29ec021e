"""The model of the stateless writers (tests/stateless_model.py) against what pins it.

By the reference's bytes: its own expectations of writeBlockDynamic at logNewTablePenalty 0 (flate/testdata/*.dyn.expect,
*.sync.expect and their -noinput twins under tests/golden/flate_dyn/).  The token lists of those tests are recovered from the fixtures
themselves: a -noinput file is never stored, so a token-level inflate reads it back into literals, (length, distance) pairs and EOB.
The model, fed those tokens and the input, must write all four files of a name byte for byte.  That pins indexTokens, both generates,
the codegen over both alphabets, dynamicSize against fixedSize against stored, and writeTokens -- for single blocks.

By validity: the reference's own inflate and gunzip, CPython's zlib and gzip read every stream of the case set back.

statelessEnc's choices, everything across blocks and EstimatedBits are held to the translated reference by tests/test_ref_deflate.py."""
import glob
import gzip
import os
import struct
import zlib

import pytest

import oracle_goref as G
import stateless_cases as S
import stateless_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_flate = pytest.mark.skipif(not G.flate_available(), reason="oracle/_ref/libzstdref.so with the reference's inflate neither present nor buildable")
needs_gunzip = pytest.mark.skipif(not G.gunzip_available(), reason="oracle/_ref/libzstdref.so with the reference's gunzip neither present nor buildable")
ALL = S.all_cases()
FL_EOF = 2  # io.ErrUnexpectedEOF in the classes of include/kcgpu.h, which oracle_goref reports


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def get(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lens):
    """canonical code of RFC 1951 3.2.2 -> {(length, code read most significant bit first): symbol}"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, l in enumerate(lens):
        if l:
            tab[(l, nxt[l])] = s
            nxt[l] += 1
    return tab


def _symbol(br, tab):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | br.get(1)
        if (l, code) in tab:
            return tab[(l, code)]
    raise ValueError("no such code")


def tokens_of(stream):
    """The tokens of ONE fixed or dynamic block: [literal | (length, distance)], whether an EOB stands in the stream's bytes, and the
    final bit.  RFC 1951 3.2.5 - 3.2.7."""
    br = _Bits(stream)
    final, kind = br.get(1), br.get(2)
    assert kind in (1, 2), "a -noinput fixture is never stored"
    if kind == 1:
        lit, dist = _decoder(M.FIXED_LIT_LEN), _decoder([5] * 30)
    else:
        hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
        cl = [0] * 19
        for k in range(hclen):
            cl[M.CODEGEN_ORDER[k]] = br.get(3)
        cltab = _decoder(cl)
        lens = []
        while len(lens) < hlit + hdist:
            s = _symbol(br, cltab)
            if s < 16:
                lens.append(s)
            elif s == 16:
                lens += [lens[-1]] * (3 + br.get(2))
            elif s == 17:
                lens += [0] * (3 + br.get(3))
            else:
                lens += [0] * (11 + br.get(7))
        assert len(lens) == hlit + hdist
        lit, dist = _decoder(lens[:hlit]), _decoder(lens[hlit:])
    out = []
    while True:
        s = _symbol(br, lit)
        if s < 256:
            out.append(s)
        elif s == 256:
            break
        else:
            lc = s - 257
            length = 3 + M.LENGTH_BASE[lc] + br.get(M.LENGTH_EXTRA[lc])
            dc = _symbol(br, dist)
            out.append((length, 1 + M.OFFSET_BASE[dc] + br.get(M.OFFSET_EXTRA[dc])))
    assert (br.pos + 7) // 8 == len(stream), "one block and its padding"
    return out, final


def _tokens(symbols):
    t = M.Tokens()
    for s in symbols:
        if isinstance(s, tuple):
            t.add_match(s[0] - 3, s[1] - 1)  # indexTokens :185-194: AddMatch, no split
        else:
            t.add_literals([s])
    return t


def golden_names():
    names = sorted(os.path.basename(p)[:-len(".dyn.expect-noinput")] for p in glob.glob(os.path.join(GOLD, "flate_dyn", "*.dyn.expect-noinput")))
    assert len(names) == 9 and "null-long-match" in names
    return names


def _read(*parts):
    with open(os.path.join(GOLD, *parts), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", golden_names())
@pytest.mark.parametrize("mode", ["dyn", "sync"])
def test_model_writes_the_references_expectations(name, mode):
    """writeBlockDynamic(tokens, false, input | nil, mode == sync) and flush at penalty 0: the reference's TestWriteBlockDynamic /
    ...Sync, byte for byte, with the tokens read back from the -noinput file of the OTHER mode as well as this one's."""
    sync = mode == "sync"
    for source in ("dyn", "sync"):
        symbols, final = tokens_of(_read("flate_dyn", "%s.%s.expect-noinput" % (name, source)))
        assert final == 0
        want = _read("flate_dyn", "%s.%s.expect-noinput" % (name, mode))
        assert M.block_dynamic_alone(_tokens(symbols), None, sync) == want, (name, mode, source, "noinput")
        if os.path.exists(os.path.join(GOLD, "flate_dyn", "%s.%s.expect" % (name, mode))):
            data = _read("flate_in", name + ".in")
            assert M.block_dynamic_alone(_tokens(symbols), data, sync) == _read("flate_dyn", "%s.%s.expect" % (name, mode)), (name, mode, source, "input")


def test_recovered_tokens_spell_the_inputs():
    """The token lists read back from the fixtures expand to the .in files (where the reference's test has an input at all)."""
    for name in golden_names():
        if not os.path.exists(os.path.join(GOLD, "flate_in", name + ".in")):
            continue
        symbols, _ = tokens_of(_read("flate_dyn", name + ".dyn.expect-noinput"))
        out = bytearray()
        for s in symbols:
            if isinstance(s, tuple):
                for _ in range(s[0]):
                    out.append(out[-s[1]])
            else:
                out.append(s)
        assert bytes(out) == _read("flate_in", name + ".in"), name


@needs_flate
def test_reference_inflate_reads_every_stream():
    for c in ALL:
        out = S.model(c).data
        got, err, used = G.flate_inflate(out, dict=c[3][-M.MAX_DICT:], max_out=len(c[1]) + 64)
        if c[2] and c[0] in S.NO_FINAL_BLOCK:  # the last block Huffman-only under the table in force: no header, so no final bit
            assert c[1].startswith(got) and len(got) >= len(c[1]) - 32768 and (err, used) == (FL_EOF, len(out)), c[0]   # (what the window still held is not handed out with the error)
        elif c[2]:
            assert (got, err, used) == (c[1], 0, len(out)), c[0]
        else:  # a non-eof call leaves the stream open: everything is there, and the reader wants more
            assert got == c[1] and err == FL_EOF, c[0]


@needs_gunzip
def test_reference_gunzip_reads_every_stream():
    for c in ALL[::3]:
        out = S.model_gzip(c)
        got, err, used = G.gunzip(out, max_out=len(c[1]) + 64)
        assert (got, err, used) == (c[1], 0, len(out)), c[0]


def test_cpython_reads_every_stream():
    for c in ALL:
        out = S.model(c).data
        do = zlib.decompressobj(-15, zdict=c[3][-M.MAX_DICT:]) if c[3] else zlib.decompressobj(-15)
        assert do.decompress(out) == c[1] and do.unused_data == b"", c[0]
        assert do.eof == (c[2] and c[0] not in S.NO_FINAL_BLOCK), c[0]
        assert len(out) <= M.bound(len(c[1]), len(c[3])), c[0]
    for c in ALL[::3]:
        gz = S.model_gzip(c)
        assert gzip.decompress(gz) == c[1], c[0]
        assert len(gz) <= M.bound(len(c[1])) + 20, c[0]
        if not c[3] and not c[2]:
            assert gz[10:-10] == S.model(c).data and gz[-10:-8] == b"\x03\x00", c[0]


def test_no_match_reaches_beyond_the_history():
    """Every match token of every block: its distance stays inside the block's bytes so far plus its history (8192, or the dictionary)."""
    for c in ALL:
        hist = min(len(c[3]), M.MAX_DICT)
        for k, t in enumerate(S.model(c).blocks):
            pos = 0
            for tok in t.tok:
                if tok < M.MATCH:
                    pos += tok != 256
                    continue
                assert (tok & 0xFFFF) + 1 <= pos + (hist if k == 0 else M.MAX_DICT), c[0]
                pos += ((tok >> 22) & 0xFF) + 3


def test_case_set_conditions():
    """Every decision is met, in the whole set and in the emulator's subset, so no suite can pass by never meeting a branch."""
    assert len(S.directed()) >= 150 and len(S.seeded()) == 300
    assert len({c[0] for c in ALL}) == len(ALL)
    for cases in (ALL, S.emu_subset()):
        counts = S.total_counts(cases)
        assert set(counts) == set(M.DECISIONS)
        assert all(v > 0 for v in counts.values()), counts
    assert any(not c[2] for c in ALL) and any(c[3] for c in ALL)


def test_cuts_and_endings():
    assert M.block_cuts(32767, 0) == [32767] and M.block_cuts(32768, 0) == [32767, 1]
    assert M.block_cuts(32767 + 24575 + 1, 0) == [32767, 24575, 1]
    assert M.block_cuts(32767, 8192) == [24575, 8192] and M.block_cuts(40000, 100) == [32667, 7333]
    for n in (0, 1, 32767, 32768, 57342, 57343, 100000):
        for d in (0, 1, 8192, 9000):
            assert M.n_blocks(n, d) == len(M.block_cuts(n, min(d, 8192)))
    assert M.stateless_deflate(b"") == bytes([0x03, 0x00])                               # writeStoredHeader(0, true) alone
    assert M.stateless_deflate(b"", eof=False) == bytes([0x00, 0x00, 0x00, 0xFF, 0xFF])  # the empty stored block alone
    assert M.gzip_stateless(b"") == M.GZIP_HEADER + bytes([0, 0, 0, 0xFF, 0xFF, 3, 0]) + bytes(8)
    # a dictionary longer than 8192 bytes is its last 8192
    d = S.text(9000, 5)
    assert M.stateless_deflate(S.text(500, 8000), dict=d) == M.stateless_deflate(S.text(500, 8000), dict=d[-8192:])


def _r32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _log2_by_hand(v, fused):
    """mFastLog2 over Python floats rounded to single precision by struct after every operation -- or, fused, after every multiply-add."""
    ux = struct.unpack("i", struct.pack("f", v))[0]
    lg = float(((ux >> 23) & 255) - 128)
    u = struct.unpack("f", struct.pack("i", (ux & ~0x7F800000) + (127 << 23)))[0]
    c1, c2, c3 = _r32(-0.34484843), _r32(2.02466578), _r32(0.67487759)
    if fused:
        t = _r32(_r32(c1 * u + c2) * u - c3)
    else:
        t = _r32(_r32(_r32(_r32(c1 * u) + c2) * u) - c3)
    return _r32(lg + t)


def _estimated_bits_by_hand(t):
    total, sh, bits, nm = t.n, 0.0, 0, 0
    inv = _r32(1.0 / total)

    def term(v, inv):
        b = -_log2_by_hand(_r32(float(v) * inv), False)
        return _r32(max(b, 1.0) * v)
    for v in t.lit_hist:
        if v:
            sh = _r32(sh + term(v, inv))
    sh = _r32(sh + 15.0)
    for i, v in enumerate(t.extra_hist[1:30]):
        if v:
            sh, bits, nm = _r32(sh + term(v, inv)), bits + M.LENGTH_EXTRA[i] * v, nm + v
    if nm:
        inv = _r32(1.0 / nm)
        for i, v in enumerate(t.off_hist[:30]):
            if v:
                sh, bits = _r32(sh + term(v, inv)), bits + M.OFFSET_EXTRA[i] * v
    return int(sh) + bits


def test_estimated_bits_is_float32_in_loop_order():
    """mFastLog2 to the bit at arguments where a fused multiply-add gives another float, and EstimatedBits of one histogram with
    literals, length codes and offset codes against the value worked out by hand (single precision by struct, the loops' order)."""
    # n / 7 in float32: the unfused value's bits, which the fused evaluation misses by 1 to 4 units in the last place
    want = {2: 3219643280, 3: 3214661000, 4: 3209672480, 5: 3203987560}
    for num, bits in want.items():
        v = M.F32(M.F32(num) * M.F32(M.F32(1.0) / M.F32(7)))
        got = struct.unpack("I", struct.pack("f", float(M.fast_log2(v))))[0]
        assert got == bits, (num, got)
        assert struct.unpack("I", struct.pack("f", _log2_by_hand(float(v), True)))[0] != bits   # (the fused twin differs: the pin means something)
        assert struct.unpack("I", struct.pack("f", _log2_by_hand(float(v), False)))[0] == bits
    t = M.Tokens()
    t.add_literals([65] * 37 + [66] * 5 + [67] * 1 + [200] * 19)
    for xl, xo in ((0, 0), (0, 0), (9, 5), (255, 7000), (40, 300), (40, 300), (130, 24576)):
        t.add_match(xl, xo)
    # extra bits: lengths 1 + 0 + 3 + 3 + 4 = 11, offsets 1 + 11 + 7 + 7 + 13 = 39; int(shannon) = 167
    assert t.estimated_bits() == 217 == _estimated_bits_by_hand(t)
    t.add_eob()  # the EOB token counts in the total and nowhere else
    assert t.estimated_bits() == _estimated_bits_by_hand(t)
    rng = S.random.Random(31)
    for _ in range(200):
        t = M.Tokens()
        for k in range(rng.randrange(1, 30)):
            t.add_literals([rng.randrange(256)] * rng.randrange(1, 200))
        for _ in range(rng.randrange(0, 40)):
            t.add_match(rng.randrange(256), rng.randrange(32767))
        assert t.estimated_bits() == _estimated_bits_by_hand(t)


def _events(name, block=0):
    c = next(c for c in ALL if c[0] == name)
    return c, S.model(c).blocks[block].events


def test_directed_cases_meet_the_rule_they_are_named_after():
    """An event is (s, t, bytes extended backwards, nextEmit before the match, the candidate came from a slot never written)."""
    for name, at in (("slot-0-hit", 12), ("slot-0-hit-later", 1), ("equal-259", 1)):
        _, ev = _events(name)
        assert ev[0] == (at, 0, 0, 0, True), name            # the first match: offset 0 answered by a zeroed slot, and taken
    _, ev = _events("back-to-t0")
    assert ev[0] == (20, 0, 1, 0, False)                      # found at 21 against 1, extended back until t == 0
    c, ev = _events("back-to-next-emit")
    s, t, back, next_emit, _ = ev[1]
    assert back == 1 and s == next_emit == 37 and t == 14 and c[1][t - 1] == c[1][s - 1]   # the byte in front matches too: nextEmit stopped it
    for name in ("match-into-history-tail", "match-into-history-tail-random"):
        _, ev = _events(name, 1)
        s, t, back, next_emit, _ = ev[0]
        assert s == M.MAX_DICT == next_emit and t < M.MAX_DICT and t >= M.MAX_DICT - 100, name   # the block's first byte into the history's last bytes
    _, ev = _events("match-at-history-head-random", 1)
    assert ev[0][:2] == (M.MAX_DICT, 0)                       # ... and into the history's first byte, 8192 back
    _, ev = _events("match-into-dict-tail")
    assert ev[0][0] == 5000 and 5000 - 80 <= ev[0][1] < 5000
    _, ev = _events("match-into-dict-head")
    assert ev[0][:2] == (5000, 0)
    _, ev = _events("match-into-dict-beyond-8192")
    assert ev[0][:2] == (8193, 0)                             # the dictionary is its last 8192 bytes: position 0 is dict[1]... the input's first byte matches there
    for run in range(258, 266):                               # AddMatchLong's split: 258s, and 255 where fewer than 3 would be left over
        c = next(c for c in ALL if c[0] == "equal-%d" % (run + 1))
        lens = [((tok >> 22) & 0xFF) + 3 for tok in S.model(c).blocks[0].tok if tok >= M.MATCH]
        assert sum(lens) == run and lens == ([run] if run == 258 else [255, run - 255] if run <= 261 else [258, run - 258]), (run, lens)
