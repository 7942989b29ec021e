"""The judge of the zlib tests: what io.ReadAll(zlib.NewReaderDict(bytes.NewReader(data), dict)) of the reference returns from a
FRESH reader, restated literally from zlib/reader.go (Reset :134-187 is the header, Read :93-121 the trailer) over the DEFLATE
decoder of tests/flate_model.py.  It is written from those lines, not from the device code.

    inflate(data, dict=b"", stale_tables=False, body=None) -> (bytes, class, consumed)

`class` is one of flate_model's KC_FL_* numbers or DICTIONARY = 6 (zlib.ErrDictionary); `bytes` is what ReadAll hands back (on an
error: what was decoded in front of it); `consumed` is the number of input bytes the reader has read when it stops.
`body(stream, dict) -> (bytes, class, consumed)` is the DEFLATE decoder the container is wrapped around: flate_model.inflate by
default (with stale_tables as given), or oracle_goref.flate_inflate, the reference's own translated inflate.

The reference's zlib reader itself cannot be executed here: the translated reference (oracle/) is frozen and holds its flate and
gzip readers only.  What pins this model instead:
  - the reference's own inflate for the body (tests/test_zlib_model.py, where oracle/_ref is present);
  - CPython's zlib.adler32 and zlib.decompressobj for the container, on every family of tests/zlib_cases.py;
  - the reference's own expectations of its reader: the rows of zlibTests in zlib/reader_test.go, committed as data in
    tests/golden/zlib_vectors.json.

Two points where the reference and zlib differ, both kept as the reference has them:
  - a stream with FDICT read WITHOUT a dictionary is compared with adler32(nil) = 1 (reader.go:164-165), so DICTID 1 is accepted
    and decoded without history; zlib asks for a dictionary;
  - the window size in CINFO is checked (<= 7) and otherwise not used: distances reach 32 KiB back whatever it says.
Not modelled: a REUSED reader, whose Reset hands the dictionary to the decompressor even without FDICT (reader.go:177-179).
"""
import zlib

import flate_model as M

OK, CORRUPT, EOF, HEADER, CHECKSUM, SIZE_EXCEEDED = M.OK, M.CORRUPT, M.EOF, M.HEADER, M.CHECKSUM, M.SIZE_EXCEEDED
DICTIONARY = 6
NAMES = dict(M.NAMES)
NAMES[DICTIONARY] = "DICTIONARY"


def inflate(data, dict=b"", stale_tables=False, body=None):
    d, zd = bytes(data), bytes(dict)
    M.fired.clear()                             # (flate_model.fired then names the rules of the body, if it was reached)
    if body is None:
        def body(stream, hist):
            return M.inflate(stream, hist, stale_tables=stale_tables)
    # Reset, reader.go:142-169
    if len(d) < 2:
        return b"", EOF, len(d)                 # io.ReadFull: io.EOF and a short read both become io.ErrUnexpectedEOF
    if d[0] & 0x0F != 8 or d[0] >> 4 > 7 or (d[0] << 8 | d[1]) % 31 != 0:
        return b"", HEADER, 2
    pos = 2
    have_dict = d[1] & 0x20 != 0
    if have_dict:
        if len(d) - pos < 4:
            return b"", EOF, len(d)
        if int.from_bytes(d[pos:pos + 4], "big") != zlib.adler32(zd):
            return b"", DICTIONARY, pos + 4
        pos += 4
    # :171-176: flate.NewReaderDict(z.r, dict) with FDICT, flate.NewReader(z.r) without
    out, cls, used = body(d[pos:], zd if have_dict else b"")
    pos += used
    if cls != OK:                               # Read, :99-104: an error of the decompressor is returned as it is
        return out, cls, pos
    # :106-120 (also behind the raw io.EOF of flate_model's rule R3: the trailer read then finds nothing)
    if len(d) - pos < 4:
        return out, EOF, len(d)
    if int.from_bytes(d[pos:pos + 4], "big") != zlib.adler32(out):
        return out, CHECKSUM, pos + 4
    return out, OK, pos + 4
