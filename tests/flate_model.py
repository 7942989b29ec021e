"""The judge of the inflate tests: what io.ReadAll(flate.NewReader(input)) and io.ReadAll(gzip.NewReader(input)) of the reference
return, restated in plain Python from the rules of flate/inflate.go, flate/inflate_gen.go and gzip/gunzip.go.  It is written from
those rules, not from the device code, and it is deliberately slow and literal.

    inflate(data, dict=b"")            -> (bytes, class, consumed)
    gunzip(data, multistream=True)     -> (bytes, class, consumed)

`class` is one of the KC_FL_* numbers below; `bytes` is what ReadAll hands back (on an error: what was decoded in front of it);
`consumed` is the number of input bytes the reference has read when it stops (for gzip with class OK: through the last trailer).
`fired` names, after a call, which of the rules below decided something in it (R1, R2, R3, R5).

Rules that differ from zlib, all taken from the reference (the tests print them where a mutated input lands on one):

  R1  a literal/length code without an end-of-block symbol is accepted (huffmanDecoder.init only asks for a complete code, the
      single one-bit code, or no code at all); zlib refuses it.  Such a block can only end in an error or at the input's end.
  R2  an incomplete code is refused as a whole unless it is the single code of length 1 (inflate.go:171); zlib's rules for
      incomplete codes are its own.
  R3  the input ending inside the extra bits of a length, inside the five bits of a fixed distance or inside the extra bits of a
      distance is io.EOF, not io.ErrUnexpectedEOF (inflate_gen.go:114-122, 142-151, 210-219 assign the raw error): ReadAll then
      returns what was decoded WITHOUT an error.  gzip goes on to the trailer, finds none, and reports ErrUnexpectedEOF.
  R4  bytes enter the bit buffer one at a time, and only as many as the shortest code (or the end-of-block code) needs
      (huffSym, inflate.go:740-783; readHuffman's maxRead, :582-594): whether a short input is EOF or CORRUPT follows from that,
      and in a block that is not the last the symbols inside the input's final bits are never decoded (maxRead + 10).
  R5  gzip: a NUL-less name or comment that runs into the input's end is the raw io.EOF (gunzip.go:157-160): NewReader fails
      with io.EOF, and behind a complete member the file simply ends there without an error.  One longer than 511 bytes is ErrHeader.

One corner is NOT restated: init() leaves the previous block's chunks in place when a table is empty (inflate.go:126-156 returns
before clearing them), so that a symbol read through an empty table may decode through a stale one.  Model and device both treat
an empty table as empty: every symbol read through it is CORRUPT once maxRead bits are there.
"""
import zlib

OK, CORRUPT, EOF, HEADER, CHECKSUM, SIZE_EXCEEDED = 0, 1, 2, 3, 4, 5
NAMES = {OK: "OK", CORRUPT: "CORRUPT", EOF: "EOF", HEADER: "HEADER", CHECKSUM: "CHECKSUM", SIZE_EXCEEDED: "SIZE_EXCEEDED"}

_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# length symbols 257..285: (base, extra bits) — RFC 1951 3.2.5
_LEN = [(3 + i, 0) for i in range(8)]
for _e in range(1, 6):
    for _k in range(4):
        _LEN.append((3 + (4 << _e) + (_k << _e), _e))
_LEN.append((258, 0))
assert len(_LEN) == 29 and _LEN[8] == (11, 1) and _LEN[27] == (227, 5)


fired = set()   # the rules R1..R5 above that decided something in the last inflate() / gunzip() call


class _Stop(Exception):
    def __init__(self, cls):
        self.cls = cls


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1)
        c >>= 1
    return r


def _init(lengths):
    """huffmanDecoder.init: None when the code is refused, else (table over max bits, mask, shortest length)."""
    count = [0] * 16
    mn = mx = 0
    for n in lengths:
        if n:
            count[n] += 1
            mn = n if mn == 0 or n < mn else mn
            mx = n if n > mx else mx
    if mx == 0:
        return ([0], 0, 0)
    code = 0
    nxt = [0] * 16
    for i in range(mn, mx + 1):
        code <<= 1
        nxt[i] = code
        code += count[i]
    if code != 1 << mx and not (code == 1 and mx == 1):
        if code < 1 << mx:
            fired.add("R2")
        return None
    tab = [0] * (1 << mx)
    for sym, n in enumerate(lengths):
        if n:
            r = _rev(nxt[n], n)
            nxt[n] += 1
            for off in range(r, 1 << mx, 1 << n):
                tab[off] = (sym << 4) | n
    return (tab, (1 << mx) - 1, mn)


_FIXED = _init([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)


class _Inflater:
    """One decompressor over data[pos:]: b / nb are the reference's bit buffer, pos its read offset."""

    def __init__(self, data, pos, hist):
        self.d, self.pos, self.b, self.nb = data, pos, 0, 0
        self.out = bytearray(hist[-32768:])
        self.base = len(self.out)

    def more(self, raw=False):
        if self.pos >= len(self.d):
            if raw:
                fired.add("R3")
            raise _Stop(OK if raw else EOF)  # R3: the raw io.EOF ends ReadAll without an error
        self.b |= self.d[self.pos] << self.nb
        self.nb += 8
        self.pos += 1

    def take(self, n, raw=False):
        while self.nb < n:
            self.more(raw)
        v = self.b & ((1 << n) - 1)
        self.b >>= n
        self.nb -= n
        return v

    def sym(self, h, max_read):
        tab, mask, _ = h
        n = max_read
        while True:
            while self.nb < n:
                self.more()
            e = tab[self.b & mask]
            n = e & 15
            if n <= self.nb:
                if n == 0:
                    raise _Stop(CORRUPT)
                self.b >>= n
                self.nb -= n
                return e >> 4

    def stored(self):
        self.b >>= self.nb & 7
        self.nb -= self.nb & 7
        hdr = bytearray()
        while self.nb:
            hdr.append(self.take(8))
        while len(hdr) < 4:
            if self.pos >= len(self.d):
                raise _Stop(EOF)
            hdr.append(self.d[self.pos])
            self.pos += 1
        n, nn = hdr[0] | hdr[1] << 8, hdr[2] | hdr[3] << 8
        if nn != n ^ 0xFFFF:
            raise _Stop(CORRUPT)
        got = self.d[self.pos:self.pos + n]
        self.out += got
        self.pos += len(got)
        if len(got) < n:
            raise _Stop(EOF)

    def dynamic(self, final):
        nlit = self.take(5) + 257
        if nlit > 286:
            raise _Stop(CORRUPT)
        ndist = self.take(5) + 1
        if ndist > 30:
            raise _Stop(CORRUPT)
        nclen = self.take(4) + 4
        cl = [0] * 19
        for i in range(nclen):
            cl[_ORDER[i]] = self.take(3)
        hc = _init(cl)
        if hc is None:
            raise _Stop(CORRUPT)
        bits, n = [], nlit + ndist
        while len(bits) < n:
            x = self.sym(hc, hc[2])
            if x < 16:
                bits.append(x)
                continue
            if x == 16:
                if not bits:
                    raise _Stop(CORRUPT)
                rep, v = 3 + self.take(2), bits[-1]
            elif x == 17:
                rep, v = 3 + self.take(3), 0
            else:
                rep, v = 11 + self.take(7), 0
            if len(bits) + rep > n:
                raise _Stop(CORRUPT)
            bits += [v] * rep
        hl, hd = _init(bits[:nlit]), _init(bits[nlit:])
        if hl is None or hd is None:
            raise _Stop(CORRUPT)
        if hl[1] and not bits[256]:
            fired.add("R1")
        mr = max(hl[2], bits[256])
        if not final:
            mr += 10
        return hl, mr, hd

    def huffman(self, hl, mr, hd):
        out = self.out
        while True:
            v = self.sym(hl, mr)
            if v < 256:
                out.append(v)
                continue
            if v == 256:
                return
            if v >= 286:
                raise _Stop(CORRUPT)
            base, extra = _LEN[v - 257]
            length = base + (self.take(extra, raw=True) if extra else 0)
            if hd is None:
                dist = _rev(self.take(5, raw=True), 5)
            else:
                dist = self.sym(hd, hd[2])
            if dist < 4:
                dist += 1
            elif dist < 30:
                nb = (dist - 2) >> 1
                dist = (1 << (nb + 1)) + 1 + ((dist & 1) << nb) + self.take(nb, raw=True)
            else:
                raise _Stop(CORRUPT)
            if dist > min(len(out), 32768):
                raise _Stop(CORRUPT)
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])

    def run(self):
        """-> class; self.out[self.base:] is what was written, self.pos what was read."""
        try:
            while True:
                final = self.take(1)
                typ = self.take(2)
                if typ == 0:
                    self.stored()
                elif typ == 1:
                    self.huffman(_FIXED, 7, None)
                elif typ == 2:
                    self.huffman(*self.dynamic(final))
                else:
                    raise _Stop(CORRUPT)
                if final:
                    return OK
        except _Stop as s:
            return s.cls


def inflate(data, dict=b""):
    fired.clear()
    f = _Inflater(bytes(data), 0, bytes(dict))
    cls = f.run()
    return bytes(f.out[f.base:]), cls, f.pos


def _gz_header(d, pos):
    """readHeader: -> (class or None for io.EOF, position behind the header, fields)."""
    if len(d) - pos < 10:
        return (None if len(d) == pos else EOF), len(d), None
    h = d[pos:pos + 10]
    if h[0] != 0x1F or h[1] != 0x8B or h[2] != 8:
        return HEADER, pos + 10, None
    flg = h[3]
    fields = {"ModTime": int.from_bytes(h[4:8], "little"), "OS": h[9], "Extra": None, "Name": "", "Comment": ""}
    start = pos
    pos += 10
    if flg & 4:
        if len(d) - pos < 2:
            return EOF, len(d), None
        n = d[pos] | d[pos + 1] << 8
        pos += 2
        if len(d) - pos < n:
            return EOF, len(d), None
        fields["Extra"] = d[pos:pos + n]
        pos += n
    for bit, key in ((8, "Name"), (16, "Comment")):
        if flg & bit:
            i = 0
            while True:
                if i >= 512:
                    return HEADER, pos + i, None
                if pos + i >= len(d):
                    fired.add("R5")
                    return None, len(d), None  # R5
                if d[pos + i] == 0:
                    break
                i += 1
            fields[key] = d[pos:pos + i].decode("latin-1")
            pos += i + 1
    if flg & 2:
        if len(d) - pos < 2:
            return EOF, len(d), None
        if (d[pos] | d[pos + 1] << 8) != (zlib.crc32(d[start:pos]) & 0xFFFF):
            return HEADER, pos + 2, None
        pos += 2
    if flg >> 5:
        return HEADER, pos, None
    return OK, pos, fields


def gunzip(data, multistream=True, want_header=False):
    fired.clear()
    d = bytes(data)
    out = bytearray()
    cls, pos, first = _gz_header(d, 0)
    if cls is None:
        cls = EOF  # NewReader returns io.EOF
    res = None
    while res is None:
        if cls != OK:
            res = (bytes(out), cls, pos)
            break
        f = _Inflater(d, pos, b"")
        c = f.run()
        member = bytes(f.out)
        out += member
        pos = f.pos
        if c != OK:
            res = (bytes(out), c, pos)
            break
        if len(d) - pos < 8:
            res = (bytes(out), EOF, len(d))
            break
        if int.from_bytes(d[pos:pos + 4], "little") != zlib.crc32(member) or int.from_bytes(d[pos + 4:pos + 8], "little") != len(member) & 0xFFFFFFFF:
            res = (bytes(out), CHECKSUM, pos + 8)
            break
        pos += 8
        if not multistream:
            res = (bytes(out), OK, pos)
            break
        end = pos
        cls, pos, _ = _gz_header(d, pos)
        if cls is None:
            res = (bytes(out), OK, end)
    return res + (first,) if want_header else res
