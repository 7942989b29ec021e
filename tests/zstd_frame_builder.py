"""A zstd frame writer in plain Python, written from the format (RFC 8878), for hand-built decoder inputs: the plain reference of
tests/zstd_frame_cases.py.  It takes an explicit description of a frame — blocks, literal sections, sequences as (ll, ml, ofVal),
the mode and the table of each sequence stream, Huffman weights and how they are coded, every header field — and returns the frame's
bytes and the plaintext, which it computes with its own sequence executor (literal runs, matches, the repeat-offset rules, dictionary
history).  Every field the writer computes can be overridden, so that a case can be wrong by exactly one field.

Nothing here chooses anything for compression's sake: there is no match finder and no statistics beyond what makes a description
valid (a flat Huffman code over the literals' alphabet, counts proportional to use for an FSE table that the case leaves open)."""
import struct

MAGIC = 0xFD2FB528

# RFC 8878 3.1.1.3.2.1.1: baselines and extra bits of the literal-length and match-length codes
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_BASE, ML_BASE = [], []
_b = 0
for _n in LL_BITS:
    LL_BASE.append(_b); _b += 1 << _n
_b = 3
for _n in ML_BITS:
    ML_BASE.append(_b); _b += 1 << _n
assert LL_BASE[16] == 16 and LL_BASE[25] == 64 and LL_BASE[35] == 65536 and ML_BASE[32] == 35 and ML_BASE[43] == 131 and ML_BASE[52] == 65539
# RFC 8878 3.1.1.3.2.2: the predefined distributions
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
              1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1]
DEFAULTS = {"ll": (LL_DEFAULT, 6), "of": (OF_DEFAULT, 5), "ml": (ML_DEFAULT, 6)}
PREDEFINED, RLE, FSE, REPEAT = 0, 1, 2, 3


def ll_code(v):
    c = max(i for i in range(36) if LL_BASE[i] <= v)
    assert v - LL_BASE[c] < 1 << LL_BITS[c], v
    return c, v - LL_BASE[c], LL_BITS[c]


def ml_code(v):
    c = max(i for i in range(53) if ML_BASE[i] <= v)
    assert v - ML_BASE[c] < 1 << ML_BITS[c], v
    return c, v - ML_BASE[c], ML_BITS[c]


def of_code(of_val):
    c = of_val.bit_length() - 1
    return c, of_val - (1 << c), c


# ---- bit writers -------------------------------------------------------------------------------------------------------------
class ForwardBits:
    """Little-endian bit writer read from the front (FSE table descriptions)."""
    def __init__(self):
        self.acc, self.n = 0, 0

    def add(self, value, nbits):
        assert 0 <= value < 1 << nbits or nbits == 0 and value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def backward_stream(reads, final_bit=True, pad_bits=0):
    """The bytes of a stream read from its end: `reads` lists (value, nbits) in the order the decoder reads them (each most significant
    bit first).  The writer lays them down last read first, then the closing 1 bit.  pad_bits: unread zero bits below the first value
    written, i.e. bits the decoder leaves behind."""
    w = ForwardBits()
    w.add(0, pad_bits)
    for v, n in reversed(reads):
        w.add(v, n)
    if final_bit:
        w.add(1, 1)
    return w.bytes()


# ---- FSE ---------------------------------------------------------------------------------------------------------------------
def fse_description(norm, table_log, acc_log_field=None):
    """FSE_Table_Description (RFC 8878 4.1.1) of explicit normalised counts: -1 entries, zero-run flags (chained 3,3,x)."""
    w = ForwardBits()
    w.add(table_log - 5 if acc_log_field is None else acc_log_field, 4)
    remaining = 1 << table_log
    i = 0
    while i < len(norm):
        p = norm[i]
        value = p + 1
        mx = remaining + 1
        bits = mx.bit_length()
        low = (1 << bits) - 1 - mx
        if value < low:
            w.add(value, bits - 1)
        elif value < 1 << (bits - 1):
            w.add(value, bits)
        else:
            w.add(value + low, bits)
        remaining -= 1 if p < 0 else p
        i += 1
        if p == 0:
            z = 0
            while i + z < len(norm) and norm[i + z] == 0:
                z += 1
            i += z
            while z >= 3:
                w.add(3, 2); z -= 3
            w.add(z, 2)
    assert remaining == 0, "counts do not sum to the table size"
    return w.bytes()


class FseTable:
    """Decoding cells (symbol, bits, base) from normalised counts (RFC 8878 4.1.1, the symbol spread), and their inverse for encoding."""
    def __init__(self, norm, table_log):
        self.log = table_log
        size = 1 << table_log
        sym = [None] * size
        high = size - 1
        nxt = []
        for s, p in enumerate(norm):
            if p == -1:
                sym[high] = s; high -= 1
                nxt.append(1)
            else:
                nxt.append(p)
        step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
        for s, p in enumerate(norm):
            for _ in range(max(p, 0)):
                sym[pos] = s
                pos = (pos + step) & mask
                while pos > high:
                    pos = (pos + step) & mask
        assert pos == 0 and None not in sym, "counts do not fill the table"
        self.cells = []
        self.by_sym = {}
        for u in range(size):
            s = sym[u]
            x = nxt[s]; nxt[s] += 1
            nb = table_log - (x.bit_length() - 1)
            base = (x << nb) - size
            self.cells.append((s, nb, base))
            self.by_sym.setdefault(s, []).append((base, nb, u))

    @staticmethod
    def rle(symbol):
        t = FseTable.__new__(FseTable)
        t.log, t.cells, t.by_sym = 0, [(symbol, 0, 0)], {symbol: [(0, 0, 0)]}
        return t

    def last_state(self, s):
        """Any state that decodes s; the one with the most bits to read, so that a two-state stream ends where it should."""
        return max(self.by_sym[s], key=lambda c: c[1])[2]

    def state_before(self, s, next_state):
        """(state, value, nbits): the state that decodes s and from which reading `nbits` bits as `value` leads to next_state."""
        for base, nb, u in self.by_sym[s]:
            if base <= next_state < base + (1 << nb):
                return u, next_state - base, nb
        raise AssertionError("symbol %d cannot lead to state %d" % (s, next_state))

    def chain(self, symbols):
        """States s_0 .. s_{n-1} and the (value, nbits) read between them, for the symbols in decoding order."""
        n = len(symbols)
        states, steps = [0] * n, [None] * max(n - 1, 0)
        states[-1] = self.last_state(symbols[-1])
        for i in range(n - 2, -1, -1):
            states[i], v, nb = self.state_before(symbols[i], states[i + 1])
            steps[i] = (v, nb)
        return states, steps


def normalise(symbols, table_log, n_syms=None):
    """Counts in proportion to use, at least 1 for a used symbol, the most used one takes the rest."""
    n_syms = n_syms or max(symbols) + 1
    hist = [0] * n_syms
    for s in symbols:
        hist[s] += 1
    size, total = 1 << table_log, len(symbols)
    norm = [max(1, h * size // total) if h else 0 for h in hist]
    top = max(range(n_syms), key=lambda s: hist[s])
    norm[top] += size - sum(norm)
    assert norm[top] >= 1, "table log too small for the alphabet"
    return norm


def fse_two_state(symbols, table):
    """Huffman weights as an FSE stream with two interleaved states (RFC 8878 4.2.1.2): even symbols by the first state."""
    assert len(symbols) >= 2
    a, b = table.chain(symbols[0::2]), table.chain(symbols[1::2])
    reads = [(a[0][0], table.log), (b[0][0], table.log)]
    for k in range(len(symbols) - 2):
        reads.append((a if k % 2 == 0 else b)[1][k // 2])
    return backward_stream(reads)


# ---- Huffman -----------------------------------------------------------------------------------------------------------------
def flat_weights(data):
    """Weights of a valid code over the bytes that occur (two lengths at most); a second symbol is added to a one-letter alphabet."""
    used = sorted(set(data))
    if not used:
        used = [0]
    if len(used) == 1:
        used = sorted(used + [(used[0] + 1) % 256])
    k = len(used)
    L = (k - 1).bit_length()
    short = (1 << L) - k  # symbols with a code of L - 1 bits
    w = [0] * (used[-1] + 1)
    for i, s in enumerate(used):
        w[s] = 2 if i < short else 1
    return w


def huf_codes(weights):
    """(table log, {symbol: (code, nbits)}) of the canonical code: by weight ascending, then symbol ascending, from code 0."""
    total = sum((1 << w) >> 1 for w in weights)
    log = total.bit_length() - 1
    assert total == 1 << log, "weights do not sum to a power of two"
    codes, pos = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (pos >> (w - 1), log + 1 - w)
                pos += 1 << (w - 1)
    return log, codes


def huf_stream(data, codes, **kw):
    return backward_stream([codes[b] for b in data], **kw)


def huf_weights_header(weights, coding="direct", table_log=6, norm=None, n_weights=None, header_byte=None, cut=None):
    """Huffman_Tree_Description: all weights but the last (implied) one, 4 bits each (`direct`) or as an FSE stream (`fse`)."""
    n = len(weights) - 1 if n_weights is None else n_weights
    ws = list(weights[:n])
    if coding == "direct":
        ws2 = ws + [0] * (len(ws) & 1)
        body = bytes(ws2[i] << 4 | ws2[i + 1] for i in range(0, len(ws2), 2))
        return bytes([127 + n if header_byte is None else header_byte]) + body
    norm = norm or normalise(ws, table_log)
    body = fse_description(norm, table_log) + fse_two_state(ws, FseTable(norm, table_log))
    if cut is not None:
        body = body[:cut]
    assert len(body) < 128
    return bytes([len(body) if header_byte is None else header_byte]) + body


# ---- descriptions ------------------------------------------------------------------------------------------------------------
class Lits:
    """A literals section.  kind: raw / rle / huf / treeless.  sf: the size-format field (0..3).  For huf: `weights` (explicit, one per
    symbol up to the last used one; default flat_weights) and `wcoding` = "direct" or ("fse", table log[, norm]).  Overrides: regen,
    comp (the two size fields), streams (the stream bytes as a list), jump (the three jump-table values), tree (the tree description),
    payload (everything behind the header)."""
    def __init__(self, kind, data, sf=None, weights=None, wcoding="direct", **ov):
        self.kind, self.data, self.sf, self.weights, self.wcoding, self.ov = kind, bytes(data), sf, weights, wcoding, ov


class Block:
    """kind: raw / rle / compressed / reserved.  raw: data.  rle: data = one byte, n = repeat count.  compressed: lits (Lits), seqs
    [(ll, ml, ofVal)], modes {"ll"/"of"/"ml": PREDEFINED | RLE | REPEAT | (FSE, table log[, norm])}, and whatever literals the sequences
    leave are the trailing ones.  Overrides: size (the header's size field), btype, nseq (the count written), mode_reserved, seq_bytes
    (the sequence section as bytes), body (the whole block content), tables (dict kind -> description bytes)."""
    def __init__(self, kind, data=b"", n=None, lits=None, seqs=(), modes=None, last=None, **ov):
        self.kind, self.data, self.n, self.lits, self.seqs, self.modes, self.last, self.ov = kind, bytes(data), n, lits, list(seqs), modes or {}, last, ov


class Corrupt(Exception):
    pass


class State:
    """What a frame carries from block to block: history, repeat offsets, the Huffman code and the three sequence tables."""
    def __init__(self, dict_content=b""):
        self.hist = bytearray(dict_content)
        self.base = len(dict_content)
        self.rep = [1, 4, 8]
        self.huf = None
        self.tab = {"ll": None, "of": None, "ml": None}


def execute(state, literals, seqs, strict=True):
    """The sequence executor: literal runs, matches, repeat-offset rules (RFC 8878 3.1.1.5), over state.hist.  Returns the block's bytes."""
    h, rep, lp, start = state.hist, state.rep, 0, len(state.hist)
    for ll, ml, of_val in seqs:
        if lp + ll > len(literals):
            raise Corrupt("literals overrun")
        h += literals[lp:lp + ll]; lp += ll
        if of_val > 3:
            off = of_val - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = of_val - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            elif idx == 1:
                off = rep[1]; rep[:] = [rep[1], rep[0], rep[2]]
            elif idx == 2:
                off = rep[2]; rep[:] = [rep[2], rep[0], rep[1]]
            else:
                off = rep[0] - 1
                if off == 0:
                    raise Corrupt("repeat offset 1 minus one byte is zero")
                rep[:] = [off, rep[0], rep[1]]
        if off > len(h):
            raise Corrupt("offset beyond history")
        for _ in range(ml) if off < ml else ():
            h.append(h[-off])
        if off >= ml:
            h += h[len(h) - off:len(h) - off + ml]
    h += literals[lp:]
    return bytes(h[start:])


# ---- sections ----------------------------------------------------------------------------------------------------------------
def literals_section(L, state):
    ov = L.ov
    data = L.data
    regen = ov.get("regen", len(data))
    if L.kind in ("raw", "rle"):
        t = 0 if L.kind == "raw" else 1
        sf = L.sf if L.sf is not None else (0 if regen < 32 else 1 if regen < 4096 else 3)
        if sf == 0:  # one bit of size format: the second bit is the size's lowest
            hdr = bytes([t | (regen & 31) << 3])
        elif sf == 1:
            hdr = struct.pack("<H", t | sf << 2 | (regen & 4095) << 4)
        else:
            hdr = struct.pack("<I", t | sf << 2 | (regen & 0xFFFFF) << 4)[:3]
        body = data if L.kind == "raw" else (data[:1] or b"\0")
        return hdr + ov.get("payload", body)
    t = 2 if L.kind == "huf" else 3
    tree = b""
    if L.kind == "huf":
        weights = L.weights if L.weights is not None else flat_weights(data)
        if "tree" in ov:
            tree = ov["tree"]
        elif L.wcoding == "direct":
            tree = huf_weights_header(weights, "direct", **ov.get("tree_kw", {}))
        else:
            tree = huf_weights_header(weights, "fse", table_log=L.wcoding[1], norm=L.wcoding[2] if len(L.wcoding) > 2 else None, **ov.get("tree_kw", {}))
        state.huf = huf_codes(weights)
    if state.huf is None:  # treeless with nothing to reuse: written with the code the case assumes, for the decoder to refuse
        state.huf = huf_codes(ov["assume_weights"])
    codes = state.huf[1]
    sf = L.sf if L.sf is not None else 1
    if "streams" in ov:
        streams = ov["streams"]
    elif sf == 0:
        streams = [huf_stream(data, codes, **ov.get("stream_kw", {}))]
    else:
        q = (len(data) + 3) // 4
        streams = [huf_stream(data[i * q:(i + 1) * q], codes, **(ov.get("stream_kw", {}) if i == 3 else {})) for i in range(4)]
    body = tree
    if len(streams) == 4:
        jump = ov.get("jump", [len(s) for s in streams[:3]])
        body += struct.pack("<HHH", *jump)
    body += b"".join(streams)
    body = ov.get("payload", body)
    comp = ov.get("comp", len(body))
    if sf in (0, 1):
        hdr = (t | sf << 2 | (regen & 1023) << 4 | (comp & 1023) << 14).to_bytes(3, "little")
    elif sf == 2:
        hdr = (t | sf << 2 | (regen & 16383) << 4 | (comp & 16383) << 18).to_bytes(4, "little")
    else:
        hdr = (t | sf << 2 | (regen & 0x3FFFF) << 4 | (comp & 0x3FFFF) << 22).to_bytes(5, "little")
    return hdr + body


def sequences_section(B, state):
    ov = B.ov
    if "seq_bytes" in ov:
        return ov["seq_bytes"]
    n = ov.get("nseq", len(B.seqs))
    if n == 0:
        out = b"\0"
    elif n < 128:
        out = bytes([n])
    elif n < 0x7F00:
        out = bytes([(n >> 8) + 128, n & 255])
    else:
        out = b"\xff" + struct.pack("<H", n - 0x7F00)
    if ov.get("nseq_bytes") is not None:
        out = ov["nseq_bytes"]
    if not B.seqs:
        return out
    coded = [(ll_code(ll), ml_code(ml), of_code(ov_)) for ll, ml, ov_ in B.seqs]
    syms = {"ll": [c[0][0] for c in coded], "ml": [c[1][0] for c in coded], "of": [c[2][0] for c in coded]}
    if "of_codes" in ov:  # the symbols of the offset stream, the extra bits staying as computed (a code above the limit)
        syms["of"] = ov["of_codes"]
    mode_byte, descr = 0, b""
    for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        m = B.modes.get(kind, PREDEFINED)
        if m == PREDEFINED:
            state.tab[kind] = FseTable(*DEFAULTS[kind]); code = 0
        elif m == RLE or isinstance(m, tuple) and m[0] == RLE:
            s = syms[kind][0] if m == RLE else m[1]
            if m == RLE:
                assert len(set(syms[kind])) == 1, "RLE mode needs one symbol"
            state.tab[kind] = FseTable.rle(s); code = 1
            descr += ov.get("tables", {}).get(kind, bytes([s]))
        elif m == REPEAT:
            code = 3
            if state.tab[kind] is None:  # nothing to repeat: the stream is written with the predefined table, the decoder must refuse
                state.tab[kind] = FseTable(*DEFAULTS[kind])
        else:
            log = m[1]
            norm = m[2] if len(m) > 2 and m[2] is not None else normalise(syms[kind], log)
            code = 2
            descr += ov.get("tables", {}).get(kind, fse_description(norm, log) + (m[3] if len(m) > 3 else b""))
            state.tab[kind] = FseTable(norm, log)
        mode_byte |= code << shift
    mode_byte |= ov.get("mode_reserved", 0)
    chains = {k: state.tab[k].chain(syms[k]) for k in ("ll", "of", "ml")}
    reads = [(chains[k][0][0], state.tab[k].log) for k in ("ll", "of", "ml")]
    last = len(coded) - 1
    for i, (lc, mc, oc) in enumerate(coded):
        reads += [(oc[1], oc[2]), (mc[1], mc[2]), (lc[1], lc[2])]
        if i != last:
            reads += [chains["ll"][1][i], chains["ml"][1][i], chains["of"][1][i]]
    return out + bytes([ov.get("mode_byte", mode_byte)]) + descr + ov.get("bitstream", backward_stream(reads, **ov.get("stream_kw", {})))


def block_bytes(B, state, last):
    """(header + content, bytes this block regenerates)."""
    ov = B.ov
    if B.kind == "raw":
        body, size, t, plain = B.data, len(B.data), 0, B.data
        state.hist += plain
    elif B.kind == "rle":
        body, size, t, plain = B.data[:1], B.n, 1, B.data[:1] * B.n
        state.hist += plain
    elif B.kind == "reserved":
        body, size, t, plain = B.data, len(B.data), 3, b""
    else:
        t = 2
        if "body" in ov:
            body, plain = ov["body"], b""
        else:
            body = literals_section(B.lits, state) + sequences_section(B, state)
            try:
                plain = execute(state, B.lits.data, B.seqs)
            except Corrupt:
                plain = b""
        size = len(body)
    size = ov.get("size", size)
    t = ov.get("btype", t)
    hdr = (int(last) | t << 1 | size << 3).to_bytes(3, "little")
    return hdr + body, plain


def frame(blocks, fcs_bytes=None, single=None, window_desc=None, dict_id=None, did_bytes=None, checksum=False, dict_content=b"",
          reserved_bit=0, unused_bit=0, content_size=None, checksum_value=None, magic=MAGIC, xxh64=None):
    """(frame bytes, plaintext).  fcs_bytes: 0 / 1 / 2 / 4 / 8 (default: the smallest that holds the size, single segment);
    window_desc: the Window_Descriptor byte (its presence clears the single-segment flag unless `single` says otherwise)."""
    state = State(dict_content)
    parts = []
    for i, B in enumerate(blocks):
        last = B.last if B.last is not None else i == len(blocks) - 1
        parts.append(block_bytes(B, state, last)[0])
    body, plain = b"".join(parts), bytes(state.hist[state.base:])
    size = len(plain) if content_size is None else content_size
    if single is None:
        single = window_desc is None
    if fcs_bytes is None:
        fcs_bytes = 0 if not single else 1 if size < 256 else 2 if size < 65536 + 256 else 4 if size < 1 << 32 else 8
    if did_bytes is None:
        did_bytes = 0 if dict_id is None else 1 if dict_id < 256 else 2 if dict_id < 65536 else 4
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6 | int(single) << 5 | unused_bit << 4 | reserved_bit << 3 | int(checksum) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    assert not (fcs_bytes == 1 and not single) and not (fcs_bytes == 0 and single), "the format cannot say this"
    out = struct.pack("<IB", magic, fhd)
    if not single:
        out += bytes([window_desc if window_desc is not None else 0x50])
    out += (dict_id or 0).to_bytes(did_bytes, "little")
    if fcs_bytes:
        out += ((size - 256) & 0xFFFF if fcs_bytes == 2 else size).to_bytes(fcs_bytes, "little")
    out += body
    if checksum:
        v = checksum_value if checksum_value is not None else xxh64(plain) & 0xFFFFFFFF
        out += struct.pack("<I", v)
    return out, plain


def skippable(payload=b"", nibble=0, size=None):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload) if size is None else size) + payload
