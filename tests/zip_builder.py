"""A small zip writer in plain Python for the hand-built archives of tests/zip_cases.py: every field of every record can be set
to what no real writer emits.  APPNOTE 6.3.x record layouts; nothing here is taken from the code under test."""
import struct
import zlib

U32 = 0xFFFFFFFF


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def zip64_extra(*vals):
    body = b"".join(struct.pack("<Q", v) for v in vals)
    return struct.pack("<HH", 1, len(body)) + body


def descriptor(crc, csize, usize, sig=True):
    return (b"PK\x07\x08" if sig else b"") + struct.pack("<III", crc, csize & U32, usize & U32)


class M:
    """One member.  body: the bytes behind the local header; the directory fields default to what is true of (data, body) and can
    each be overridden; local_name / local_extra: what the LOCAL header carries where it differs; trailer: bytes behind the body
    (a data descriptor)."""

    def __init__(self, name, data=b"", method=8, level=6, body=None, **kw):
        self.name = name if isinstance(name, bytes) else name.encode()
        self.data = data
        self.body = body if body is not None else (deflate(data, level) if method == 8 else data)
        self.method = method
        self.flags = kw.pop("flags", 0)
        self.crc = kw.pop("crc", zlib.crc32(data))
        self.csize = kw.pop("csize", len(self.body))
        self.usize = kw.pop("usize", len(data))
        self.extra = kw.pop("extra", b"")
        self.comment = kw.pop("comment", b"")
        self.local_name = kw.pop("local_name", self.name)
        self.local_extra = kw.pop("local_extra", b"")
        self.local_sig = kw.pop("local_sig", b"PK\x03\x04")
        self.trailer = kw.pop("trailer", b"")
        self.hoff = kw.pop("hoff", None)          # the directory's header offset, where it is not the true one
        self.raw32 = kw.pop("raw32", None)        # (csize32, usize32, hoff32) as the directory's 32-bit fields, where not derived
        self.eattr = kw.pop("eattr", 0)
        self.cver, self.rver = kw.pop("cver", 20), kw.pop("rver", 20)
        assert not kw, kw

    def local(self):
        return (self.local_sig + struct.pack("<HHHHHIIIHH", self.rver, self.flags, self.method, 0, 0x21, self.crc, min(self.csize, U32), min(self.usize, U32),
                                             len(self.local_name), len(self.local_extra)) + self.local_name + self.local_extra + self.body + self.trailer)

    def central(self, at):
        hoff = at if self.hoff is None else self.hoff
        c32, u32, h32 = self.raw32 if self.raw32 else (min(self.csize, U32), min(self.usize, U32), min(hoff, U32))
        return (b"PK\x01\x02" + struct.pack("<HHHHHHIIIHHHHHII", self.cver, self.rver, self.flags, self.method, 0, 0x21, self.crc, c32, u32, len(self.name),
                                            len(self.extra), len(self.comment), 0, 0, self.eattr, h32) + self.name + self.extra + self.comment)


def end_record(records, dsize, doff, comment=b"", comment_len=None):
    return b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, records & 0xFFFF, records & 0xFFFF, dsize & U32, doff & U32,
                                       len(comment) if comment_len is None else comment_len) + comment


def end_record64(records, dsize, doff):
    return b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, records, records, dsize, doff)


def locator64(off, disk=0, total=1):
    return b"PK\x06\x07" + struct.pack("<IQI", disk, off, total)


def build(members, comment=b"", prefix=b"", records=None, zip64=False, dsize=None, doff=None, junk=b"", comment_len=None, end32=None):
    """-> (archive bytes, [true header offset per member]).  prefix: bytes in front that the end record's offsets do not count;
    records / dsize / doff: what the end record states where it is not the truth; zip64: a zip64 end record and locator, the
    32-bit end record maxed out (end32: its (records, dsize, doff) instead); junk: bytes behind the end record."""
    out, offs = bytearray(), []
    for m in members:
        offs.append(len(out))
        out += m.local()
    cd_at = len(out)
    for m, at in zip(members, offs):
        out += m.central(at)
    size = len(out) - cd_at
    records = len(members) if records is None else records
    dsize = size if dsize is None else dsize
    doff = cd_at if doff is None else doff
    if zip64:
        at64 = len(out)
        out += end_record64(records, dsize, doff) + locator64(at64)
        out += end_record(*(end32 or (0xFFFF, U32, U32)), comment, comment_len)
    else:
        out += end_record(records, dsize, doff, comment, comment_len)
    return bytes(prefix) + bytes(out) + bytes(junk), [len(prefix) + o for o in offs]
