"""compress/gzip's reader on the device: gzip files (RFC 1952), any number of members, inflated in batches of independent inputs
(include/kcgpu.h kc_gzip_inflate*).  Headers, trailers, ISIZE and CRC-32 are checked on the device; the Header fields of the first
member are parsed here, on the host.  There is no CPU fallback."""
from . import flate
from .flate import InflateError, CorruptInputError, ErrUnexpectedEOF  # noqa: F401


class ErrHeader(InflateError):
    """gzip.ErrHeader: "gzip: invalid header"."""

    def __init__(self, status=flate.FL_HEADER):
        super().__init__(status)


class ErrChecksum(InflateError):
    """gzip.ErrChecksum: "gzip: invalid checksum" — the CRC-32 or the ISIZE of a member."""

    def __init__(self, status=flate.FL_CHECKSUM):
        super().__init__(status)


_ERRORS = dict(flate._ERRORS)
_ERRORS.update({flate.FL_HEADER: ErrHeader, flate.FL_CHECKSUM: ErrChecksum})


class Header:
    """gzip.Header (gunzip.go:52-58) of a file's first member."""

    def __init__(self):
        self.Comment, self.Extra, self.ModTime, self.Name, self.OS = "", None, 0, "", 0


def parse_header(data):
    """The fields readHeader (gunzip.go:183-253) fills, from the front of data; ModTime in seconds since 1970.  None when the device
    will refuse the header: validity is its verdict, this only extracts."""
    d = bytes(data[:10])
    if len(d) < 10 or d[0] != 0x1F or d[1] != 0x8B or d[2] != 8:
        return None
    h = Header()
    flg = d[3]
    h.ModTime = int.from_bytes(d[4:8], "little")
    h.OS = d[9]
    pos = 10
    if flg & 4:
        n = int.from_bytes(data[pos:pos + 2], "little")
        h.Extra = bytes(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    for bit, key in ((8, "Name"), (16, "Comment")):
        if flg & bit:
            end = bytes(data[pos:pos + 513]).find(b"\0")
            if end < 0:
                return None
            setattr(h, key, bytes(data[pos:pos + end]).decode("latin-1"))
            pos += end + 1
    return h


def GunzipAll(src, in_off, multistream=True, device=0):
    """N x io.ReadAll(gzip.NewReader(input_i)) in one batch (host buffers): a list of bytes or the InflateError per input."""
    b = flate.Batch("kc_gzip_inflate", _ERRORS, multistream=multistream, device=device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def GunzipBounds(src, in_off, multistream=True, device=0):
    """The sizing pass alone (kc_gzip_inflate_bound): (sizes, status short of the CRC-32, consumed)."""
    import numpy as np
    b = flate.Batch("kc_gzip_inflate", _ERRORS, multistream=multistream, device=device)
    try:
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        return b.bounds(src.ctypes.data, in_off, False)
    finally:
        b.close()


def GunzipAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, multistream=True, device=0, stream=None):
    """Device-resident form: (uint64[n + 1] offsets, uint32[n] status, uint64[n] consumed).  A failed input's range is empty or
    zero-filled."""
    b = flate.Batch("kc_gzip_inflate", _ERRORS, multistream=multistream, device=device, stream=stream)
    try:
        return b.inflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


class Reader(flate.Reader):
    """gzip.Reader (gunzip.go:74-124): Multistream, Read, WriteTo, Reset, Close and .Header of the first member.  Like flate.Reader
    the whole input is read and decoded on the device on first use."""

    _prefix, _errors = "kc_gzip_inflate", _ERRORS

    def __init__(self, r, device=0):
        self._multistream = True
        super().__init__(r, None, device=device)

    def Reset(self, r, dict=None):
        """Reader.Reset (gunzip.go:105-124): read from r from now on; Multistream is on again."""
        super().Reset(r, None)
        self._multistream = True
        self._header = None

    def Multistream(self, ok):
        """Reader.Multistream (gunzip.go:142-144)."""
        self._multistream = bool(ok)

    def _options(self):
        return {"multistream": self._multistream}

    @property
    def Header(self):
        self._decode()
        if self._header is None:
            self._header = parse_header(self._data)
        return self._header


def NewReader(r, device=0):
    """gzip.NewReader(r)."""
    return Reader(r, device=device)


# ---- the writers: gzip.NewWriterLevel(w, gzip.HuffmanOnly) and (w, gzip.StatelessCompression) on the device (include/kcgpu.h
# kc_gzip_deflate*, kc_gzip_stateless_deflate*) ----
HuffmanOnly = flate.HuffmanOnly
StatelessCompression = -3  # gzip/gzip.go:26-31: every Write one flate.StatelessDeflate, nothing kept between them


def _batch(level, flush, block, penalty, device, stream=None):
    if level == StatelessCompression:
        if flush or block is not None or penalty is not None:
            raise flate._lib.KcError(flate._lib.KC_ERR_UNSUPPORTED, "gzip: StatelessCompression has no flush ending, block size or penalty (Flush does nothing at this level)")
        return flate.StatelessBatch("kc_gzip_stateless_deflate", device=device, stream=stream)
    return flate.WriteBatch("kc_gzip_deflate", level, flush, block, penalty, device=device, stream=stream)


def GzipAll(src, in_off, level=HuffmanOnly, flush=False, device=0, block=None, penalty=None):
    """N x (w = gzip.NewWriterLevel(buf, level); w.Write(input_i); w.Close()) in one batch, byte for byte: the default Header (no
    name, no time, OS 255), the stream, CRC-32 and size.  level: gzip.HuffmanOnly or gzip.StatelessCompression (KcError
    KC_ERR_UNSUPPORTED otherwise).  flush=True (HuffmanOnly): w.Flush() in Close's place — no trailer."""
    b = _batch(level, flush, block, penalty, device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def GzipAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, level=HuffmanOnly, flush=False, device=0, stream=None, block=None, penalty=None):
    """Device-resident form: uint64[n + 1] offsets into d_dst (see flate.DeflateAllDevice)."""
    b = _batch(level, flush, block, penalty, device, stream)
    try:
        return b.deflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


class Writer(flate.Writer):
    """gzip.Writer (gzip.go:32-47) with the default Header: Write buffers, Close encodes one input on the device."""

    _prefix = "kc_gzip_deflate"


class StatelessWriter(flate.StatelessWriter):
    """gzip.Writer at StatelessCompression (gzip.go:171-235 Write, :264-290 Close): the header goes out with the first Write, every
    Write is one non-eof flate.StatelessDeflate on the device, Close is the eof call on nothing, then CRC-32 and size.  Flush does
    nothing at this level (:249-251)."""

    _HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])

    def Reset(self, w):
        self._w, self._closed, self._wrote_header, self._crc, self._size = w, False, False, 0, 0

    def Write(self, p):
        import zlib as host_zlib
        if self._closed:
            raise ValueError("gzip: write to closed writer")
        p = bytes(p)
        if not self._wrote_header:
            self._wrote_header = True
            self._w.write(self._HEADER)
        self._size = (self._size + len(p)) & 0xFFFFFFFF
        self._crc = host_zlib.crc32(p, self._crc) & 0xFFFFFFFF
        self._write_call(p)
        return len(p)

    def Flush(self):
        return None

    def Close(self):
        if self._closed:
            return
        if not self._wrote_header:
            self.Write(b"")
        flate.StatelessWriter.Close(self)
        self._w.write(self._crc.to_bytes(4, "little") + self._size.to_bytes(4, "little"))


def NewWriterLevel(w, level=HuffmanOnly, device=0):
    """gzip.NewWriterLevel(w, level): gzip.HuffmanOnly and gzip.StatelessCompression are the levels served."""
    if level == StatelessCompression:
        return StatelessWriter(w, device=device)
    return Writer(w, level, device=device)
