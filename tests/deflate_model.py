"""The HuffmanOnly writer of the reference, restated in plain Python: the model the emulator and the device are compared with.

What is restated (the reference's Go, by file and line):
  flate/deflate.go        init :795-799 (32 KiB window, logNewTablePenalty 10), write / storeHuff :755-770, :701-708 (every full
                          window is one writeBlockHuff(false, window, false)), close :865-880 and syncFlush :772-785 (the rest
                          with sync = true, then writeStoredHeader(0, eof) and flush)
  flate/huffman_bit_writer.go
                          writeBlockHuff :987-1174, generateCodegen :269-348, codegens / headerSize :350-368,
                          writeDynamicHeader :458-497, writeStoredHeader :502-529, flush :192-218
  flate/huffman_code.go   generate :339-371, bitCounts :183-309, assignEncodingAndSize :313-333, canReuseBits :151-163
  gzip/gzip.go            the default header (XFL 0 at this level, OS 255) and the CRC-32 / ISIZE trailer

The block size, the penalty and the end mode are parameters: compressor.init fixes (32768, 10) for HuffmanOnly; the reference's
own goldens of writeBlockHuff are single blocks of up to 65535 bytes at penalty 8.
"""
import struct
import zlib

import numpy as np

MAXI32 = (1 << 31) - 1
END_CLOSE, END_FLUSH = 0, 1
DECISIONS = ("quick-stored", "est-stored", "first-table", "reuse", "new-table-eob-owed", "not-reusable")
CODEGEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def bit_counts(lst, max_bits):
    """huffman_code.go:183-309, statement by statement.  lst: (literal, freq) ascending by (freq, literal), at least 3."""
    n = len(lst)
    lst = lst + [(0xFFFF, 0xFFFF)]  # maxNode
    if max_bits > n - 1:
        max_bits = n - 1
    # levels: [level, lastFreq, nextCharFreq, nextPairFreq, needed]
    levels = [[0, 0, 0, 0, 0] for _ in range(17)]
    leaf = [[0] * 16 for _ in range(16)]
    l2f = lst[2][1]
    l1f = lst[1][1]
    l0f = lst[0][1] + lst[1][1]
    for level in range(1, max_bits + 1):
        levels[level] = [level, l1f, l2f, l0f, 0]
        leaf[level][level] = 2
        if level == 1:
            levels[level][3] = MAXI32
    levels[max_bits][4] = 2 * n - 4
    level = max_bits
    while level < 16:
        l = levels[level]
        if l[3] == MAXI32 and l[2] == MAXI32:
            l[4] = 0
            levels[level + 1][3] = MAXI32
            level += 1
            continue
        prev_freq = l[1]
        if l[2] < l[3]:
            k = leaf[level][level] + 1
            l[1] = l[2]
            leaf[level][level] = k
            e = lst[k]
            l[2] = e[1] if e[0] < 0xFFFF else MAXI32
        else:
            l[1] = l[3]
            save = leaf[level][level]
            leaf[level] = list(leaf[level - 1])
            leaf[level][level] = save
            levels[l[0] - 1][4] = 2
        l[4] -= 1
        if l[4] == 0:
            if l[0] == max_bits:
                break
            levels[l[0] + 1][3] = prev_freq + l[1]
            level += 1
        else:
            while levels[level - 1][4] > 0:
                level -= 1
    assert leaf[max_bits][max_bits] == n
    bit_count = [0] * (max_bits + 1)
    bits = 1
    counts = leaf[max_bits]
    for level in range(max_bits, 0, -1):
        bit_count[bits] = counts[level] - counts[level - 1]
        bits += 1
    return bit_count


def generate(freq, max_bits):
    """huffman_code.go:339-371: (lengths, bit-reversed codes) of the code for freq."""
    nsym = len(freq)
    lens = [0] * nsym
    codes = [0] * nsym
    lst = [(i, f) for i, f in enumerate(freq) if f]
    if len(lst) <= 2:
        for i, (lit, _) in enumerate(lst):
            lens[lit], codes[lit] = 1, i
        return lens, codes
    lst.sort(key=lambda e: (e[1], e[0]))
    bit_count = bit_counts(lst, max_bits)
    code = 0
    for n, bits in enumerate(bit_count):  # assignEncodingAndSize :313-333
        code <<= 1
        if n == 0 or bits == 0:
            continue
        chunk = sorted(lst[len(lst) - bits:])
        for lit, _ in chunk:
            lens[lit], codes[lit] = n, _reverse(code, n)
            code += 1
        lst = lst[:len(lst) - bits]
    return lens, codes


def can_reuse_bits(lens, freq):
    total = 0
    for i, f in enumerate(freq):
        if f:
            if lens[i] == 0:
                return MAXI32
            total += f * lens[i]
    return total


def generate_codegen(lit_lens, off_lens):
    """huffman_bit_writer.go:269-348: the codegen sequence (without its end marker) and its frequencies."""
    BAD = 255
    cg = list(lit_lens) + list(off_lens) + [BAD]
    freq = [0] * 19
    out = []
    size, count = cg[0], 1
    i = 1
    while size != BAD:
        nxt = cg[i]
        i += 1
        if nxt == size:
            count += 1
            continue
        if size != 0:
            out.append(size)
            freq[size] += 1
            count -= 1
            while count >= 3:
                n = min(6, count)
                out += [16, n - 3]
                freq[16] += 1
                count -= n
        else:
            while count >= 11:
                n = min(138, count)
                out += [18, n - 11]
                freq[18] += 1
                count -= n
            if count >= 3:
                out += [17, count - 3]
                freq[17] += 1
                count = 0
        count -= 1
        while count >= 0:
            out.append(size)
            freq[size] += 1
            count -= 1
        size, count = nxt, 1
    return out, freq


class BitWriter:
    """huffmanBitWriter as far as the HuffmanOnly level drives it."""

    def __init__(self, penalty):
        self.parts = []    # the stream so far: arrays of bits, first bit first
        self.total = 0     # bits written
        self.penalty = penalty
        self.last_header = 0
        self.lens = None   # literalEncoding: the table in force
        self.codes = None
        self.counts = dict.fromkeys(DECISIONS, 0)
        self.boundary_phases = set()  # bit phases at which a block's codes ended
        self.margins = []  # (decision, left side - right side) of every comparison taken between two encodings: what tools/find_deflate_ties.py reads

    @property
    def nbits(self):
        return self.total & 7

    def write_bits(self, v, n):
        self.parts.append(np.array([(v >> k) & 1 for k in range(n)], dtype=np.uint8))
        self.total += n

    def write_bytes(self, data):
        assert self.total & 7 == 0
        self.parts.append(np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little"))
        self.total += 8 * len(data)

    def write_codes(self, data, lens, codes):
        """Every byte's code, one after the other (numpy only for speed: bit k of symbol j lands at start[j] + k)."""
        sym = np.frombuffer(bytes(data), dtype=np.uint8)
        ln = np.asarray(lens[:256], dtype=np.int64)[sym]
        cd = np.asarray(codes[:256], dtype=np.int64)[sym]
        end = np.cumsum(ln)
        start = end - ln
        bits = np.zeros(int(end[-1]) if len(end) else 0, dtype=np.uint8)
        for k in range(15):
            m = ln > k
            bits[start[m] + k] = (cd[m] >> k) & 1
        self.parts.append(bits)
        self.total += len(bits)

    def bytes(self):
        assert self.total & 7 == 0
        if not self.parts:
            return b""
        return np.packbits(np.concatenate(self.parts), bitorder="little").tobytes()

    def _owed_eob(self):
        if self.last_header > 0:
            self.write_bits(self.codes[256], self.lens[256])
            self.last_header = 0

    def flush(self):  # :192-218
        self._owed_eob()
        if self.nbits:
            self.write_bits(0, 8 - self.nbits)

    def write_stored_header(self, length, eof):  # :502-529
        self._owed_eob()
        if length == 0 and eof:
            self.write_bits(3, 3)
            self.write_bits(0, 7)
            self.flush()
            return
        self.write_bits(1 if eof else 0, 3)
        self.flush()
        self.write_bits(length, 16)
        self.write_bits(~length & 0xFFFF, 16)

    def write_block_huff(self, eof, data, sync):  # :987-1174
        n = len(data)
        assert 0 < n <= 65535
        freq = np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=257).tolist()
        ssize = (n + 5) * 8
        if n > 1024:
            # float64 in the reference; exact in integers: sum (v - n/256)^2 < 2n  <=>  sum (256 v - n)^2 < 2 n 65536
            self.margins.append(("abs-max", sum((256 * v - n) ** 2 for v in freq[:256]) - 2 * n * 65536))
            if sum((256 * v - n) ** 2 for v in freq[:256]) < 2 * n * 65536:
                self.counts["quick-stored"] += 1
                self.write_stored_header(n, eof)
                self.write_bytes(data)
                return
        freq[256] = 1
        tmp_lens, tmp_codes = generate(freq, 15)
        est = can_reuse_bits(tmp_lens, freq)
        if est < MAXI32:
            est += self.last_header
            if self.last_header == 0:
                est += 70 * 8
            est += est >> self.penalty
        self.margins.append(("ssize-est", ssize - est))
        if ssize <= est:
            self.counts["est-stored"] += 1
            self.write_stored_header(n, eof)
            self.write_bytes(data)
            return
        first = self.last_header == 0
        if self.last_header > 0:
            reuse = can_reuse_bits(self.lens, freq[:256])
            self.margins.append(("est-reuse", est - reuse))
            if est < reuse:
                self.counts["new-table-eob-owed"] += 1
                if reuse == MAXI32:
                    self.counts["not-reusable"] += 1
                self.write_bits(self.codes[256], self.lens[256])
                self.last_header = 0
            else:
                self.counts["reuse"] += 1
        if self.last_header == 0:
            if first:
                self.counts["first-table"] += 1
            self.lens, self.codes = tmp_lens, tmp_codes
            cg, cgfreq = generate_codegen(self.lens, [1])  # huffOffset: one offset code of length 1
            cglens, cgcodes = generate(cgfreq, 7)
            ncg = 19
            while ncg > 4 and cgfreq[CODEGEN_ORDER[ncg - 1]] == 0:
                ncg -= 1
            # writeDynamicHeader :458-497
            self.write_bits(5 if eof else 4, 3)
            self.write_bits(257 - 257, 5)
            self.write_bits(1 - 1, 5)
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
            self.last_header = (3 + 5 + 5 + 4 + 3 * ncg + sum(f * l for f, l in zip(cgfreq, cglens)) +
                                cgfreq[16] * 2 + cgfreq[17] * 3 + cgfreq[18] * 7)  # headerSize :358-368
        self.write_codes(data, self.lens, self.codes)
        self.boundary_phases.add(self.nbits)
        if eof or sync:
            self.write_bits(self.codes[256], self.lens[256])
            self.last_header = 0


class Result:
    def __init__(self, data, counts, boundary_phases, end_phase):
        self.data, self.counts, self.boundary_phases, self.end_phase = data, counts, boundary_phases, end_phase
        self.margins = []


def deflate_ex(data, block=32768, penalty=10, end=END_CLOSE):
    """flate.NewWriter(w, HuffmanOnly); Write(data); Close() -- or Flush() with end=END_FLUSH."""
    w = BitWriter(penalty)
    n = len(data)
    pos = 0
    while n - pos > block:  # a rest of exactly one window goes out with sync = true (close :869-870)
        w.write_block_huff(False, data[pos:pos + block], False)
        pos += block
    if n - pos:
        w.write_block_huff(False, data[pos:], True)
    end_phase = w.nbits
    w.write_stored_header(0, end == END_CLOSE)
    w.flush()
    res = Result(w.bytes(), w.counts, w.boundary_phases, end_phase)
    res.margins = w.margins
    return res


def deflate(data, block=32768, penalty=10, end=END_CLOSE):
    return deflate_ex(data, block, penalty, end).data


GZIP_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])


def gzip_deflate(data, block=32768, penalty=10, end=END_CLOSE):
    """gzip.NewWriterLevel(w, HuffmanOnly); Write(data); Close() -- Flush() ends without the trailer."""
    body = GZIP_HEADER + deflate(data, block, penalty, end)
    if end == END_FLUSH:
        return body
    return body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def block_huff_alone(data, penalty=8):
    """What the reference's own test of writeBlockHuff does: one writeBlockHuff(false, all, false), then flush."""
    w = BitWriter(penalty)
    w.write_block_huff(False, data, False)
    w.flush()
    return w.bytes()


def bound(n, block=32768):
    """kc_flate_deflate_bound (gzip adds 18).  A stored block costs its bytes + 5 and up to 15 bits of owed EOB in front.  A Huffman
    block is taken only when bytes*8 + 40 > codes + 560 (the header GUESS), but its real header may reach 17 + 19*3 + 258*7 = 1880
    bits, and an owed EOB and its own EOB add up to 30: at most bytes*8 + 1390 bits.  So 176 bytes per block, and 8 for the end."""
    nblk = (n + block - 1) // block
    return n + 176 * nblk + 8
