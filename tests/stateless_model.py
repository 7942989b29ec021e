"""flate.StatelessDeflate of the reference, restated in plain Python: the model the emulator and the device are compared with.

What is restated (the reference's Go, by file and line):
  flate/stateless.go      StatelessDeflate :76-162 (the block cutter: the first block 32767 - len(dict) bytes, every later one
                          32767 - 8192 behind 8 KiB of history; stored / writeBlockHuff / writeBlockDynamic per block :134-145; the
                          empty stored block of a non-eof call :156-159), statelessEnc :176-325, NewStatelessWriter :21-55
  flate/token.go          AddMatchLong :284-309, AddEOB :311-315, EstimatedBits :225-260 and mFastLog2 :212-220 (float32)
  flate/huffman_bit_writer.go
                          writeBlockDynamic :620-765, canReuse :163-190, indexTokens :784-815, extraBitSize / fixedSize / storedSize /
                          dynamicSize / dynamicReuseSize / headerSize :350-419, writeFixedHeader :531-547, writeTokens :824-975;
                          writeBlockHuff and what it calls come from deflate_model.py
  gzip/gzip.go            Write :171-235 (every Write one non-eof StatelessDeflate), Close :264-290 (the eof call on nothing)

The bit writer is bitWriterPool's: newHuffmanBitWriter(nil) and reset, so logNewTablePenalty is 0 -- the estimate of a new table is
DOUBLED (newSize>>0 at :665, estBits>>0 at :1042), where HuffmanOnly adds a 1024th.
"""
import struct
import zlib

import numpy as np

from deflate_model import CODEGEN_ORDER, GZIP_HEADER, MAXI32, BitWriter, _reverse, generate, generate_codegen

MAX_BLOCK = 32767   # maxStatelessBlock
MAX_DICT = 8192     # maxStatelessDict
TABLE_SHIFT = 32 - 13
MAX_PREDEF = 250    # maxPredefinedTokens
MATCH = 1 << 30     # matchType
DECISIONS = ("stored-no-match", "huffman-only", "dyn-first-table", "dyn-reuse", "dyn-new-table-eob-owed", "dyn-fixed",
             "dyn-stored-by-size", "cannot-reuse")

LENGTH_BASE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 255)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
OFFSET_BASE = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192,
               12288, 16384, 24576)
OFFSET_EXTRA = tuple(0 if c < 2 else c // 2 - 1 for c in range(30))
LENGTH_CODE = np.zeros(256, dtype=np.int64)   # lengthCodes[length - 3]
for _c, _b in enumerate(LENGTH_BASE):
    LENGTH_CODE[_b:] = _c
OFFSET_CODE = np.zeros(32768, dtype=np.int64)  # offsetCode(offset - 1)
for _c, _b in enumerate(OFFSET_BASE):
    OFFSET_CODE[_b:] = _c

FIXED_LIT_LEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_LIT_CODE = ([_reverse(0x30 + c, 8) for c in range(144)] + [_reverse(0x190 + c, 9) for c in range(112)] +
                  [_reverse(c, 7) for c in range(24)] + [_reverse(0xC0 + c, 8) for c in range(8)])
FIXED_OFF_LEN = [5] * 30
FIXED_OFF_CODE = [_reverse(c, 5) for c in range(30)]

F32 = np.float32


def fast_log2(val):
    """token.go:212-220 in float32, every operation rounded on its own (the reference's default amd64 build fuses nothing)."""
    ux = int(np.array([val], dtype=np.float32).view(np.int32)[0])
    log2 = F32(((ux >> 23) & 255) - 128)
    ux &= ~0x7F800000
    ux += 127 << 23
    uval = np.array([ux], dtype=np.int32).view(np.float32)[0]
    t = F32(F32(-0.34484843) * uval)
    t = F32(t + F32(2.02466578))
    t = F32(t * uval)
    t = F32(t - F32(0.67487759))
    return F32(log2 + t)


class Tokens:
    """tokens of token.go: the three histograms, n and the token words (literal, or matchType | length-3 << 22 | code << 16 | offset-1)."""

    def __init__(self):
        self.lit_hist = [0] * 256
        self.extra_hist = [0] * 32
        self.off_hist = [0] * 32
        self.tok = []
        self.events = []  # per match found by stateless_enc: (s, t, bytes extended backwards, nextEmit before it, candidate from a slot never written)

    @property
    def n(self):
        return len(self.tok)

    def add_literals(self, data):
        for v in data:
            self.lit_hist[v] += 1
        self.tok.extend(data)

    def add_match(self, xlength, xoffset):  # AddMatch :264-280: length - 3, offset - 1
        oc = int(OFFSET_CODE[xoffset])
        self.extra_hist[int(LENGTH_CODE[xlength]) + 1] += 1
        self.off_hist[oc] += 1
        self.tok.append(MATCH | xlength << 22 | oc << 16 | xoffset)

    def add_match_long(self, length, xoffset):  # :284-309
        while length > 0:
            xl = length
            if xl > 258:
                xl = 258 if xl > 258 + 3 else 258 - 3
            length -= xl
            self.add_match(xl - 3, xoffset)

    def add_eob(self):  # :311-315
        self.tok.append(256)
        self.extra_hist[0] += 1

    def estimated_bits(self):  # :225-260, nFilled = 0
        shannon = F32(0)
        bits = 0
        n_matches = 0
        total = self.n
        at_least_one = lambda v: F32(1) if v < 1 else F32(15) if v > 15 else v  # noqa: E731  (huffman_code.go:374-382)
        if total > 0:
            inv = F32(F32(1.0) / F32(total))
            for v in self.lit_hist:
                if v > 0:
                    n = F32(v)
                    shannon = F32(shannon + F32(at_least_one(-fast_log2(F32(n * inv))) * n))
            shannon = F32(shannon + F32(15))
            for i, v in enumerate(self.extra_hist[1:30]):
                if v > 0:
                    n = F32(v)
                    shannon = F32(shannon + F32(at_least_one(-fast_log2(F32(n * inv))) * n))
                    bits += LENGTH_EXTRA[i] * v
                    n_matches += v
        if n_matches > 0:
            inv = F32(F32(1.0) / F32(n_matches))
            for i, v in enumerate(self.off_hist[:30]):
                if v > 0:
                    n = F32(v)
                    shannon = F32(shannon + F32(at_least_one(-fast_log2(F32(n * inv))) * n))
                    bits += OFFSET_EXTRA[i] * v
        return int(shannon) + bits


def _hash(u):
    return ((u * 0x1E35A7BD) & 0xFFFFFFFF) >> TABLE_SHIFT


def stateless_enc(dst, src, start_at):
    """stateless.go:176-325.  The reference keeps its positions in int16 and tests nextS <= 0 for the wrap; plain integers are
    equivalent, because a value that wrapped is also above sLimit (len(src) <= 32767)."""
    n = len(src)
    assert n <= MAX_BLOCK
    if n - start_at < 13:
        return
    ld32 = lambda i: int.from_bytes(src[i:i + 4], "little")  # noqa: E731
    ld64 = lambda i: int.from_bytes(src[i:i + 8], "little")  # noqa: E731
    table = [0] * 8192
    written = bytearray(8192)  # (for the tests alone: which slots were ever written)
    if start_at > 0:
        cv = ld32(0)
        for i in range(start_at):
            table[_hash(cv)] = i
            written[_hash(cv)] = 1
            cv = (cv >> 8) | (src[i + 4] << 24)
    s = start_at + 1
    next_emit = start_at
    s_limit = n - 11
    cv = ld32(s)
    done = False
    while not done:
        next_s = s
        while True:
            h = _hash(cv)
            cand, fresh = table[h], not written[h]
            next_s = s + 2 + ((s - next_emit) >> 5)
            if next_s > s_limit:
                done = True
                break
            now = ld64(next_s)
            table[h] = s
            written[h] = 1
            h = _hash(now & 0xFFFFFFFF)
            if cv == ld32(cand):
                table[h] = next_s
                written[h] = 1
                break
            cv = now & 0xFFFFFFFF
            s = next_s
            next_s += 1
            cand, fresh = table[h], not written[h]
            now >>= 8
            table[h] = s
            written[h] = 1
            if cv == ld32(cand):
                table[h] = next_s
                written[h] = 1
                break
            cv = now & 0xFFFFFFFF
            s = next_s
        if done:
            break
        while True:
            t = cand
            l = 4
            a, b = s + 4, t + 4
            while a < n and src[a] == src[b]:
                step = 64
                if src[a:a + step] == src[b:b + step] and a + step <= n:
                    a += step; b += step; l += step
                    continue
                a += 1; b += 1; l += 1
            back = 0
            while t > 0 and s > next_emit and src[t - 1] == src[s - 1]:
                s -= 1; t -= 1; l += 1; back += 1
            dst.events.append((s, t, back, next_emit, fresh))
            if next_emit < s:
                dst.add_literals(src[next_emit:s])
            assert 1 <= s - t <= 32767 and t >= 0
            dst.add_match_long(l, s - t - 1)
            s += l
            next_emit = s
            if next_s >= s:
                s = next_s + 1
            if s >= s_limit:
                done = True
                break
            x = ld64(s - 2)
            o = s - 2
            table[_hash(x & 0xFFFFFFFF)] = o
            written[_hash(x & 0xFFFFFFFF)] = 1
            x >>= 16
            h = _hash(x & 0xFFFFFFFF)
            cand, fresh = table[h], not written[h]
            table[h] = o + 2
            written[h] = 1
            if (x & 0xFFFFFFFF) != ld32(cand):
                cv = (x >> 8) & 0xFFFFFFFF
                s += 1
                break
    if next_emit < n:
        if dst.n == 0:
            return
        dst.add_literals(src[next_emit:])


def bit_length(lens, freq):
    return sum(f * lens[i] for i, f in enumerate(freq) if f)


class Writer(BitWriter):
    """huffmanBitWriter as StatelessDeflate drives it: writeBlockHuff (deflate_model.BitWriter) alternating with writeBlockDynamic."""

    def __init__(self):
        BitWriter.__init__(self, 0)
        self.counts.update(dict.fromkeys(DECISIONS, 0))
        self.last_huffman = False
        self.olens = self.ocodes = None

    def write_block_huff(self, eof, data, sync):
        table = self.lens
        self._wrote_codes = False
        BitWriter.write_block_huff(self, eof, data, sync)
        if not self._wrote_codes:    # a stored block: lastHuffMan stays
            return
        if self.lens is not table:   # :1082
            self.last_huffman = True
        if eof or sync:              # :1169-1173
            self.last_huffman = False

    def write_codes(self, data, lens, codes):
        self._wrote_codes = True
        BitWriter.write_codes(self, data, lens, codes)

    def _put_fields(self, vals, lens):
        vals = np.asarray(vals, dtype=np.int64)
        lens = np.asarray(lens, dtype=np.int64)
        end = np.cumsum(lens)
        start = end - lens
        bits = np.zeros(int(end[-1]) if len(end) else 0, dtype=np.uint8)
        for k in range(16):
            m = lens > k
            bits[start[m] + k] = (vals[m] >> k) & 1
        self.parts.append(bits)
        self.total += len(bits)

    def write_fixed_header(self, eof):  # :531-547
        self._owed_eob()
        self.write_bits(3 if eof else 2, 3)

    def write_tokens(self, tok, lens, codes, olens, ocodes):  # :824-975
        t = np.asarray(tok, dtype=np.int64)
        if len(t) == 0:
            return
        is_match = t >= MATCH
        xl = (t >> 22) & 0xFF
        lc = LENGTH_CODE[xl]
        off = t & 0xFFFF
        oc = (t >> 16) & 31
        sym = np.where(is_match, 257 + lc, t)
        L = np.asarray(lens, dtype=np.int64)
        Cd = np.asarray(codes, dtype=np.int64)
        OL = np.asarray(list(olens) + [0] * 2, dtype=np.int64)
        OC = np.asarray(list(ocodes) + [0] * 2, dtype=np.int64)
        assert (L[sym] > 0).all() and (OL[oc[is_match]] > 0).all(), "a symbol without a code"
        vals = np.zeros((len(t), 4), dtype=np.int64)
        ln = np.zeros((len(t), 4), dtype=np.int64)
        vals[:, 0] = Cd[sym]
        ln[:, 0] = L[sym]
        vals[:, 1] = np.where(is_match, xl - np.asarray(LENGTH_BASE)[lc], 0)
        ln[:, 1] = np.where(is_match, np.asarray(LENGTH_EXTRA)[lc], 0)
        vals[:, 2] = np.where(is_match, OC[oc], 0)
        ln[:, 2] = np.where(is_match, OL[oc], 0)
        vals[:, 3] = np.where(is_match, off - np.asarray(OFFSET_BASE + (0, 0))[oc], 0)
        ln[:, 3] = np.where(is_match, np.asarray(OFFSET_EXTRA + (0, 0))[oc], 0)
        self._put_fields(vals.reshape(-1), ln.reshape(-1))

    def can_reuse(self, t):  # :163-190
        for i in range(30):
            if t.off_hist[i] and self.olens[i] == 0:
                return False
        for i in range(30):
            if t.extra_hist[i] and self.lens[256 + i] == 0:
                return False
        for i in range(256):
            if t.lit_hist[i] and self.lens[i] == 0:
                return False
        return True

    def _stored(self, data, eof):
        self.counts["dyn-stored-by-size"] += 1
        self.write_stored_header(len(data), eof)
        self.write_bytes(data)

    def _fixed(self, t, eof, sync):
        self.counts["dyn-fixed"] += 1
        self.write_fixed_header(eof)
        if not sync:
            t.add_eob()
        self.write_tokens(t.tok, FIXED_LIT_LEN, FIXED_LIT_CODE, FIXED_OFF_LEN, FIXED_OFF_CODE)

    def write_block_dynamic(self, t, eof, data, sync):  # :620-765
        sync = sync or eof
        if sync:
            t.add_eob()
        if (self.last_huffman or eof) and self.last_header > 0:
            self._owed_eob()
            self.last_huffman = False
        if self.last_header > 0 and not self.can_reuse(t):
            self.counts["cannot-reuse"] += 1
            self._owed_eob()
        first = self.last_header == 0
        # indexTokens(t, true) :784-815
        lit_freq = t.lit_hist + t.extra_hist[:30]
        off_freq = list(t.off_hist[:30])
        lit_freq[256] = 1
        num_lit = 286
        while lit_freq[num_lit - 1] == 0:
            num_lit -= 1
        num_off = 30
        while num_off > 0 and off_freq[num_off - 1] == 0:
            num_off -= 1
        if num_off == 0:
            off_freq[0] = 1
            num_off = 1
        storable = data is not None and len(data) <= 65535
        ssize = (len(data) + 5) * 8 if storable else 0
        extra = 0
        if storable or self.last_header > 0:  # extraBitSize :389-398
            extra = sum(f * LENGTH_EXTRA[i] for i, f in enumerate(lit_freq[257:286])) + sum(f * OFFSET_EXTRA[i] for i, f in enumerate(off_freq))
        fixed = 3 + bit_length(FIXED_LIT_LEN, lit_freq) + bit_length(FIXED_OFF_LEN, off_freq) + extra
        if self.last_header > 0:
            new_size = self.last_header + t.estimated_bits()
            new_size += self.lens[256] + (new_size >> self.penalty)
            reuse = bit_length(self.lens, lit_freq) + bit_length(self.olens, off_freq) + extra
            self.margins.append(("dyn-new-reuse", new_size - reuse))
            if new_size < reuse:
                self.counts["dyn-new-table-eob-owed"] += 1
                self._owed_eob()
                size = new_size
            else:
                size = reuse
            if t.n < MAX_PREDEF and fixed + 7 < size:
                if storable and ssize <= size:
                    return self._stored(data, eof)
                return self._fixed(t, eof, sync)
            if storable and ssize <= size:
                return self._stored(data, eof)
        if self.last_header == 0:
            lens, codes = generate(lit_freq, 15)
            olens, ocodes = generate(off_freq, 15)
            # generate() has run on the writer's encoders: they are the table "in force" from here on, whatever is written (a later
            # block consults them only while lastHeader > 0, and that needs the header below)
            cg, cgfreq = generate_codegen(lens[:num_lit], olens[:num_off])
            cglens, cgcodes = generate(cgfreq, 7)
            ncg = 19
            while ncg > 4 and cgfreq[CODEGEN_ORDER[ncg - 1]] == 0:
                ncg -= 1
            header = (3 + 5 + 5 + 4 + 3 * ncg + sum(f * l for f, l in zip(cgfreq, cglens)) + cgfreq[16] * 2 + cgfreq[17] * 3 + cgfreq[18] * 7)
            size = header + bit_length(lens, lit_freq) + bit_length(olens, off_freq) + extra
            if t.n < MAX_PREDEF and fixed <= size:
                if storable and ssize <= fixed:
                    return self._stored(data, eof)
                return self._fixed(t, eof, sync)
            if storable and ssize <= size:
                return self._stored(data, eof)
            if first:
                self.counts["dyn-first-table"] += 1
            self.lens, self.codes, self.olens, self.ocodes = lens, codes, olens, ocodes
            self.write_bits(5 if eof else 4, 3)  # writeDynamicHeader :458-497
            self.write_bits(num_lit - 257, 5)
            self.write_bits(num_off - 1, 5)
            self.write_bits(ncg - 4, 4)
            for i in range(ncg):
                self.write_bits(cglens[CODEGEN_ORDER[i]], 3)
            i = 0
            while i < len(cg):
                w = cg[i]
                i += 1
                self.write_bits(cgcodes[w], cglens[w])
                if w >= 16:
                    self.write_bits(cg[i], {16: 2, 17: 3, 18: 7}[w])
                    i += 1
            if not sync:
                self.last_header = header
            self.last_huffman = False
        else:
            self.counts["dyn-reuse"] += 1
        if sync:
            self.last_header = 0
        self.write_tokens(t.tok, self.lens, self.codes, self.olens, self.ocodes)


class Result:
    def __init__(self, data, counts, blocks):
        self.data, self.counts, self.blocks = data, counts, blocks
        self.margins = []


def block_cuts(n, dict_len):
    """The lengths of the blocks of an input of n bytes behind a dictionary of dict_len (<= 8192) bytes: stateless.go:106-116."""
    cuts = []
    first = True
    while n > 0:
        todo = min(n, MAX_BLOCK - dict_len if first else MAX_BLOCK - MAX_DICT)
        cuts.append(todo)
        n -= todo
        first = False
    return cuts


def stateless_deflate_ex(data, eof=True, dict=b""):
    data = bytes(data)
    w = Writer()
    blocks = []
    if eof and len(data) == 0:
        w.write_stored_header(0, True)
        w.flush()
        return Result(w.bytes(), w.counts, blocks)
    dict = bytes(dict)[-MAX_DICT:] if dict else b""
    pos = 0
    for k, todo in enumerate(block_cuts(len(data), len(dict))):
        unc = data[pos:pos + todo]
        if k == 0:
            src, start = dict + unc, len(dict)
        else:
            src, start = data[pos - MAX_DICT:pos + todo], MAX_DICT
        pos += todo
        last = pos == len(data)
        t = Tokens()
        stateless_enc(t, src, start)
        is_eof = eof and last
        w._wrote_codes = False
        if t.n == 0:
            w.counts["stored-no-match"] += 1
            w.write_stored_header(len(unc), is_eof)
            w.write_bytes(unc)
        elif t.n > len(unc) - (len(unc) >> 4):
            w.margins.append(("tokens-15/16", t.n - (len(unc) - (len(unc) >> 4))))
            w.counts["huffman-only"] += 1
            w.write_block_huff(is_eof, unc, last)
        else:
            w.margins.append(("tokens-15/16", t.n - (len(unc) - (len(unc) >> 4))))
            w.write_block_dynamic(t, is_eof, unc, last)
        blocks.append(t)
    if not eof:
        w.write_stored_header(0, False)
    w.flush()
    res = Result(w.bytes(), w.counts, blocks)
    res.margins = w.margins
    return res


def stateless_deflate(data, eof=True, dict=b""):
    return stateless_deflate_ex(data, eof, dict).data


def gzip_stateless(data):
    """gzip.NewWriterLevel(w, gzip.StatelessCompression); Write(data); Close()."""
    data = bytes(data)
    return (GZIP_HEADER + stateless_deflate(data, False) + stateless_deflate(b"", True) +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF))


def block_dynamic_alone(tokens, data, sync):
    """What the reference's own test of writeBlockDynamic does: one writeBlockDynamic(tokens, false, input, sync), then flush."""
    w = Writer()
    w.write_block_dynamic(tokens, False, data, sync)
    w.flush()
    return w.bytes()


def n_blocks(n, dict_len=0):
    dict_len = min(dict_len, MAX_DICT)
    first = MAX_BLOCK - dict_len
    return 0 if n == 0 else 1 if n <= first else 1 + (n - first + MAX_BLOCK - MAX_DICT - 1) // (MAX_BLOCK - MAX_DICT)


def bound(n, dict_len=0):
    """kc_flate_stateless_bound (gzip adds 18 + 2).  Per block its bytes and 176: a stored block costs 5 and an owed EOB; a dynamic,
    reused or fixed block is written only where its exact size is below the stored size (writeBlockDynamic's ssize <= size
    returns), so it costs less than a stored one plus the EOB owed in front of it; a Huffman-only block inherits the 560-bit
    header guess of writeBlockHuff (176 bytes, kc_flate_deflate_bound).  8 for the end: the empty stored block of a non-eof call
    behind an owed EOB, or the ten-bit block of an empty eof call."""
    return n + 176 * n_blocks(n, dict_len) + 8
