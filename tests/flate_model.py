"""The judge of the inflate tests: what io.ReadAll(flate.NewReader(input)) and io.ReadAll(gzip.NewReader(input)) of the reference
return, restated in plain Python from the rules of flate/inflate.go, flate/inflate_gen.go and gzip/gunzip.go.  It is written from
those rules, not from the device code, and it is deliberately slow and literal.

    inflate(data, dict=b"", stale_tables=False)           -> (bytes, class, consumed)
    gunzip(data, multistream=True, stale_tables=False)    -> (bytes, class, consumed)

`class` is one of the KC_FL_* numbers below; `bytes` is what ReadAll hands back (on an error: what was decoded in front of it);
`consumed` is the number of input bytes the reference has read when it stops (for gzip with class OK: through the last trailer, or
through the input's end where the reader went on to look for another member).
`fired` names, after a call, which of the rules below decided something in it (R1, R2, R3, R5, R6).

With stale_tables=True the model is the reference, byte for byte and read for read: tests/test_ref_flate.py holds it against the
reference's own code (translated: oracle/ref_go) on every case the suites use.  With stale_tables=False it is what the device
implements: the same, except that rule R6 is replaced by "an empty table is empty".

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

  R6  (stale_tables) huffmanDecoder.init returns on an empty code (inflate.go:154-156) after it has reset maxRead and linkMask to 0
      (:126-128) and BEFORE it clears chunks (:180-183): a symbol read through an empty table is looked up, from n = 0 bits on, in
      whatever that decoder held last.  h1 serves the code-length code and then the literal/length code (readHuffman :506, :575),
      so an empty literal/length code decodes through THIS block's code-length table (the symbols 0..18 come out as literals, and
      no end-of-block symbol exists: the block ends in an error), an empty code-length code through the table h1 held before (the
      last literal/length code, or a code-length table behind an empty one; a symbol above 18 out of it is an InternalError, class
      INTERNAL), an empty distance code through the last dynamic block's distance table.  gzip keeps h1 and h2 from member to
      member (decompressor.Reset :812-824).  A decoder never built holds zeroes: CORRUPT at once.  _HD below is the reference's
      table layout (9-bit chunks, link tables) for this path only.  The device does not follow R6: there an empty table is empty
      and every symbol read through it is CORRUPT (RFC 1951's reading, and zlib's); see profiles/flate_reference_parity.md.
"""
import zlib

OK, CORRUPT, EOF, HEADER, CHECKSUM, SIZE_EXCEEDED = 0, 1, 2, 3, 4, 5
INTERNAL = 99   # flate.InternalError: reachable through R6 only; no device status
NAMES = {OK: "OK", CORRUPT: "CORRUPT", EOF: "EOF", HEADER: "HEADER", CHECKSUM: "CHECKSUM", SIZE_EXCEEDED: "SIZE_EXCEEDED", INTERNAL: "INTERNAL"}

_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# length symbols 257..285: (base, extra bits) — RFC 1951 3.2.5
_LEN = [(3 + i, 0) for i in range(8)]
for _e in range(1, 6):
    for _k in range(4):
        _LEN.append((3 + (4 << _e) + (_k << _e), _e))
_LEN.append((258, 0))
assert len(_LEN) == 29 and _LEN[8] == (11, 1) and _LEN[27] == (227, 5)


fired = set()   # the rules R1..R6 above that decided something in the last inflate() / gunzip() call


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


class _HD:
    """huffmanDecoder as the reference lays it out (inflate.go:104-279), kept beside the model's own tables for rule R6: what init
    leaves behind when it returns early.  chunks: 512 entries over 9 bits, value << 4 | length, a length above 9 = a link index."""

    def __init__(self):
        self.max_read, self.chunks, self.links, self.link_mask = 0, [0] * 512, [], 0

    def init(self, lengths):
        if self.max_read != 0:
            self.max_read, self.link_mask = 0, 0   # *h = huffmanDecoder{chunks: h.chunks, links: h.links}
        count = [0] * 16
        mn = mx = 0
        for n in lengths:
            if n:
                mn = n if mn == 0 or n < mn else mn
                mx = n if n > mx else mx
                count[n] += 1
        if mx == 0:
            return True            # chunks and links stay as they are
        code, nxt = 0, [0] * 16
        for i in range(mn, mx + 1):
            code <<= 1
            nxt[i] = code
            code += count[i]
        if code != 1 << mx and not (code == 1 and mx == 1):
            return False
        self.max_read = mn
        self.chunks = [0] * 512
        if mx > 9:
            nlinks = 1 << (mx - 9)
            self.link_mask = nlinks - 1
            link = nxt[10] >> 1
            self.links = [[0] * nlinks for _ in range(512 - link)]
            for j in range(link, 512):
                self.chunks[_rev(j, 16) >> 7] = ((j - link) << 4) | 10
        else:
            self.links = []
        for i, n in enumerate(lengths):
            if n == 0:
                continue
            c = nxt[n]
            nxt[n] += 1
            chunk = (i << 4) | n
            r = _rev(c, 16) >> (16 - n)
            if n <= 9:
                for off in range(r, 512, 1 << n):
                    self.chunks[off] = chunk
            else:
                tab = self.links[self.chunks[r & 511] >> 4]
                for off in range(r >> 9, len(tab), 1 << (n - 9)):
                    tab[off] = chunk
        return True


class _Inflater:
    """One decompressor over data[pos:]: b / nb are the reference's bit buffer, pos its read offset."""

    def __init__(self, data, pos, hist, hds=None):
        self.d, self.pos, self.b, self.nb = data, pos, 0, 0
        self.out = bytearray(hist[-32768:])
        self.base = len(self.out)
        self.h1, self.h2 = hds if hds else (None, None)   # R6: the reference's h1 / h2, or None (an empty table is empty)

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

    def sym(self, h, max_read, hd=None):
        tab, mask, _ = h
        n = max_read
        if mask == 0 and hd is not None:   # R6: huffSym through what init left in place (an empty table: max_read is h.maxRead)
            fired.add("R6")
            while True:
                while self.nb < n:
                    self.more()
                chunk = hd.chunks[self.b & 511]
                n = chunk & 15
                if n > 9:
                    chunk = hd.links[chunk >> 4][(self.b >> 9) & hd.link_mask]
                    n = chunk & 15
                if n <= self.nb:
                    if n == 0:
                        raise _Stop(CORRUPT)
                    self.b >>= n
                    self.nb -= n
                    return chunk >> 4
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
        v = self.take(14)   # HLIT, HDIST and HCLEN are read together, before either is checked (inflate.go:466-470)
        nlit = (v & 31) + 257
        if nlit > 286:
            raise _Stop(CORRUPT)
        ndist = (v >> 5 & 31) + 1
        if ndist > 30:
            raise _Stop(CORRUPT)
        nclen = (v >> 10) + 4
        cl = [0] * 19
        for i in range(nclen):
            cl[_ORDER[i]] = self.take(3)
        hc = _init(cl)
        if self.h1:
            self.h1.init(cl)
        if hc is None:
            raise _Stop(CORRUPT)
        bits, n = [], nlit + ndist
        while len(bits) < n:
            x = self.sym(hc, hc[2], self.h1)
            if x < 16:
                bits.append(x)
                continue
            if x == 16:
                if not bits:
                    raise _Stop(CORRUPT)
                rep, v = 3 + self.take(2), bits[-1]
            elif x == 17:
                rep, v = 3 + self.take(3), 0
            elif x == 18:
                rep, v = 11 + self.take(7), 0
            else:
                raise _Stop(INTERNAL)   # (R6 only: a symbol above 18 out of a stale literal/length table)
            if len(bits) + rep > n:
                raise _Stop(CORRUPT)
            bits += [v] * rep
        hl = _init(bits[:nlit])
        if self.h1:
            self.h1.init(bits[:nlit])
        if hl is None:   # (h1.init(...) || h2.init(...): h2 is not touched when h1 is refused — the error ends the stream either way)
            raise _Stop(CORRUPT)
        hd = _init(bits[nlit:])
        if self.h2:
            self.h2.init(bits[nlit:])
        if hd is None:
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
            v = self.sym(hl, mr, self.h1 if hd is not None else None)
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
                dist = self.sym(hd, hd[2], self.h2)
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


def inflate(data, dict=b"", stale_tables=False):
    fired.clear()
    f = _Inflater(bytes(data), 0, bytes(dict), (_HD(), _HD()) if stale_tables else None)
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


def gunzip_header(data):
    """The first member's header fields as gunzip(want_header=True) returns them: None where NewReader fails."""
    return _gz_header(bytes(data), 0)[2]


def gunzip(data, multistream=True, want_header=False, stale_tables=False):
    fired.clear()
    hds = (_HD(), _HD()) if stale_tables else None   # one decompressor serves every member (Reset keeps h1 and h2)
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
        f = _Inflater(d, pos, b"", hds)
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
        cls, pos, _ = _gz_header(d, pos)
        if cls is None:   # io.EOF where the next header should be: the file ends, and what was read looking for it is read (R5: to the end)
            res = (bytes(out), OK, pos)
    return res + (first,) if want_header else res
