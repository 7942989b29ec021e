"""The judge of the zip tests: what zip.NewReader and f.Open() / io.ReadAll / Close of the reference return, restated in plain Python
from zip/reader.go (Reader.init :146-207, File.Open :247-286, checksumReader.Read :324-362, findBodyOffset :368-381,
readDirectoryHeader :386-564, readDataDescriptor :566-603, readDirectoryEnd :605-682, findDirectory64End :687-708,
readDirectory64End :712-732, findSignatureInBlock :734-750) and detectUTF8 of zip/writer.go:230-248, over tests/flate_model.py with
stale_tables=False (what the device implements).  It is written from those rules, not from the device code.

    directory(data)          -> (class, Dir or None)
    member(data, m)          -> (bytes, class, planned)     m: a Member; planned: the bytes of its range in the layout, or None
    read_all(data, members)  -> [(bytes of the range, class)], the layout's total

`fired` names, after member(), the return of the rules that decided it (the eight rules of include/kcgpu.h, "5a" .. for their
branches): tests/zip_cases.py records it per case and the suite asserts that every one is hit.

Two classes stand for more than one error of the reference, because the C ABI has one number for them: DIR_EOF is
io.ErrUnexpectedEOF and the plain io.EOF that init hands through (a zip64 end record that lies past the archive's end, :714-716; a
directory whose headers run exactly to the archive's end, :388, :413); READAT is whatever the ReaderAt returns for the thirty bytes
of the local header (io.EOF over a byte slice, "negative offset" below zero).  SIZE is this library's own limit of 1 GiB per
member."""
import collections
import struct
import zlib

import flate_model as FM

OK, CORRUPT, EOF = FM.OK, FM.CORRUPT, FM.EOF
FORMAT, DIR_EOF, COMMENT, ALGORITHM, CHECKSUM, READAT, SIZE = 16, 17, 18, 19, 20, 21, 22
NAMES = {OK: "OK", CORRUPT: "CORRUPT", EOF: "EOF", FORMAT: "FORMAT", DIR_EOF: "DIR_EOF", COMMENT: "COMMENT", ALGORITHM: "ALGORITHM",
         CHECKSUM: "CHECKSUM", READAT: "READAT", SIZE: "SIZE"}
MAX_MEMBER = 1 << 30

Member = collections.namedtuple("Member", "header_offset compressed_size uncompressed_size crc32 method flags is_dir")
Entry = collections.namedtuple("Entry", "name comment extra non_utf8 creator_version reader_version flags method modified_time modified_date "
                                        "crc32 compressed_size64 uncompressed_size64 external_attrs header_offset")
Dir = collections.namedtuple("Dir", "comment base_offset files")

fired = set()
_IOEOF = "io.EOF"   # (inside this file only: the plain io.EOF, where the reference tells it from io.ErrUnexpectedEOF)


def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def detect_utf8(s):
    """writer.go:230-248 -> (valid, require)"""
    try:
        s.decode("utf-8")   # strict: no overlong forms, no surrogates, nothing above U+10FFFF -- utf8.DecodeRuneInString's rules
    except UnicodeDecodeError:
        return False, False
    return True, any(b < 0x20 or b > 0x7d or b == 0x5c for b in s)


def _header(data, pos, end):
    """readDirectoryHeader over data[pos:end] -> (error or None, Entry, position behind it)"""
    if end - pos < 46:
        return (_IOEOF if end == pos else DIR_EOF), None, pos
    (sig, cver, rver, flags, method, mtime, mdate, crc, csize, usize, nl, el, cl, _disk, _iattr, eattr, hoff) = struct.unpack_from("<IHHHHHHIIIHHHHHII", data, pos)
    if sig != 0x02014b50:
        return FORMAT, None, pos
    var = nl + el + cl
    have = end - (pos + 46)
    if have < var:
        return (_IOEOF if have == 0 else DIR_EOF), None, pos
    p = pos + 46
    name, extra, comment = data[p:p + nl], data[p + nl:p + nl + el], data[p + nl + el:p + var]
    v1, r1 = detect_utf8(name)
    v2, r2 = detect_utf8(comment)
    if not v1 or not v2:
        non_utf8 = True
    elif not r1 and not r2:
        non_utf8 = False
    else:
        non_utf8 = flags & 0x800 == 0
    need_u, need_c, need_h = usize == 0xFFFFFFFF, csize == 0xFFFFFFFF, hoff == 0xFFFFFFFF
    x = extra
    while len(x) >= 4:
        tag, size = struct.unpack_from("<HH", x)
        x = x[4:]
        if len(x) < size:
            break
        fb, x = x[:size], x[size:]
        if tag != 1:
            continue
        if need_u:
            need_u = False
            if len(fb) < 8:
                return FORMAT, None, pos
            usize, fb = struct.unpack_from("<Q", fb)[0], fb[8:]
        if need_c:
            need_c = False
            if len(fb) < 8:
                return FORMAT, None, pos
            csize, fb = struct.unpack_from("<Q", fb)[0], fb[8:]
        if need_h:
            need_h = False
            if len(fb) < 8:
                return FORMAT, None, pos
            hoff, fb = _i64(struct.unpack_from("<Q", fb)[0]), fb[8:]
    if need_c or need_h:
        return FORMAT, None, pos
    return None, Entry(name, comment, extra, non_utf8, cver, rver, flags, method, mtime, mdate, crc, csize, usize, eattr, hoff), pos + 46 + var


def _find_signature(b):
    for i in range(len(b) - 22, -1, -1):
        if b[i:i + 4] == b"PK\x05\x06":
            n = b[i + 20] | b[i + 21] << 8
            if n + 22 + i > len(b):
                return -1
            return i
    return -1


def _directory_end(data):
    """readDirectoryEnd -> (error or None, records, size, offset, comment, baseOffset)"""
    size = len(data)
    for i, blen in enumerate((1024, 65 * 1024)):
        blen = min(blen, size)
        buf = data[size - blen:]
        p = _find_signature(buf)
        if p >= 0:
            buf = buf[p:]
            end_off = size - blen + p
            break
        if i == 1 or blen == size:
            return FORMAT, 0, 0, 0, b"", 0
    _, _, _, records, dsize, doff, clen = struct.unpack_from("<HHHHIIH", buf, 4)
    b = buf[22:]
    if clen > len(b):
        return COMMENT, 0, 0, 0, b"", 0
    comment = b[:clen]
    if records == 0xffff or dsize == 0xffff or doff == 0xffffffff:
        loc = end_off - 20
        p64 = -1
        if loc >= 0:
            sig, disk, p, total = struct.unpack_from("<IIQI", data, loc)
            if sig == 0x07064b50 and disk == 0 and total == 1:
                p64 = _i64(p)
        if p64 >= 0:
            end_off = p64
            if p64 + 56 > size:
                return _IOEOF, 0, 0, 0, b"", 0
            if struct.unpack_from("<I", data, p64)[0] != 0x06064b50:
                return FORMAT, 0, 0, 0, b"", 0
            records, dsize, doff = struct.unpack_from("<QQQ", data, p64 + 32)
    if dsize > (1 << 63) - 1 or doff > (1 << 63) - 1:
        return FORMAT, 0, 0, 0, b"", 0
    base = _i64(end_off - dsize - doff)
    o = _i64(base + doff)
    if o < 0 or o >= size:
        return FORMAT, 0, 0, 0, b"", 0
    if base > 0 and doff < size and _header(data, doff, size)[0] is None:
        base = 0
    return None, records, dsize, doff, comment, base


def directory(data):
    data = bytes(data)
    err, records, dsize, doff, comment, base = _directory_end(data)
    if err is not None:
        return (DIR_EOF if err == _IOEOF else err), None
    files, pos = [], base + doff
    while True:
        err, e, pos = _header(data, pos, len(data))
        if err in (FORMAT, DIR_EOF):
            break
        if err is not None:
            return DIR_EOF, None
        files.append(e._replace(header_offset=_i64(e.header_offset + base)))
    if len(files) & 0xFFFF != records & 0xFFFF:
        return err, None
    return OK, Dir(comment, base, files)


def member_of(e):
    return Member(e.header_offset, e.compressed_size64, e.uncompressed_size64, e.crc32, e.method, e.flags, e.name.endswith(b"/"))


def body_offset(data, m):
    """findBodyOffset -> (class, headerOffset + bodyOffset)"""
    off = m.header_offset
    if off < 0 or off + 30 > len(data):
        return READAT, 0
    if data[off:off + 4] != b"PK\x03\x04":
        return FORMAT, 0
    nl, el = struct.unpack_from("<HH", data, off + 26)
    return OK, off + 30 + nl + el


def _decide(rule, content, cls, planned):
    fired.add(rule)
    return content, cls, planned


def member(data, m):
    fired.clear()
    cls, body = body_offset(data, m)                                      # rule 1
    if cls:
        return _decide("1-readat" if cls == READAT else "1-format", b"", cls, None)
    if m.is_dir:                                                          # rule 2
        return _decide("2-format", b"", FORMAT, None) if m.uncompressed_size else _decide("2-ok", b"", OK, None)
    if m.method not in (0, 8):                                            # rule 3
        return _decide("3", b"", ALGORITHM, None)
    if m.compressed_size > MAX_MEMBER or m.uncompressed_size > MAX_MEMBER:  # the library's limit
        return _decide("8", b"", SIZE, None)
    raw = data[body:body + m.compressed_size]                             # rule 4: the SectionReader ends with the file
    usize = m.uncompressed_size
    if m.method == 0:
        out, err = raw, OK
        planned = usize if len(raw) == usize else None
    else:
        out, err, _ = FM.inflate(raw, stale_tables=False)
        planned = usize if usize <= 1032 * len(raw) + 1032 else None
    if len(out) > usize:                                                  # rule 5
        return _decide("5-format", b"", FORMAT, planned)
    if err:
        return _decide("5-corrupt" if err == CORRUPT else "5-eof", b"", err, planned)
    if len(out) != usize:
        return _decide("5-short", b"", EOF, planned)
    crc = zlib.crc32(out)
    if m.flags & 8:                                                       # rule 6
        d = data[body + m.compressed_size:body + m.compressed_size + 16] if body + m.compressed_size <= len(data) else b""
        if len(d) < 4:
            return _decide("6-absent", b"", EOF, planned)
        sig = d[:4] == b"PK\x07\x08"
        if len(d) < (16 if sig else 12):
            return _decide("6-short", b"", EOF, planned)
        if struct.unpack_from("<I", d, 4 if sig else 0)[0] != m.crc32:
            return _decide("6-field", b"", CHECKSUM, planned)
        if crc != m.crc32:
            return _decide("6-hash", b"", CHECKSUM, planned)
        return _decide("6-ok", out, OK, planned)
    if m.crc32 != 0 and crc != m.crc32:                                   # rule 7
        return _decide("7-hash", b"", CHECKSUM, planned)
    return _decide("7-ok" if m.crc32 else "7-unset", out, OK, planned)


def read_all(data, members):
    """What kc_zip_read leaves: per member the bytes of its range (zero-filled where it failed) and its class; the layout's total."""
    res, total = [], 0
    for m in members:
        out, cls, planned = member(data, m)
        n = planned or 0
        total += n
        res.append((out if cls == OK else bytes(n), cls))
        if cls == OK:
            assert len(out) == n, (m, len(out), planned)
    return res, total
