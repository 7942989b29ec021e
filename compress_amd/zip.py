"""archive/zip's reader on the device (the reference's zip package: zip/reader.go, zip/struct.go): the central directory is read on
the host (include/kcgpu.h kc_zip_dir_*), the members are inflated or copied and their CRC-32s checked on the device, a whole
archive — or the members of several — in one batch (kc_zip_read*; kernels compress_amd/csrc/kc_zip.hip).  The directory states
every member's decoded size, so every member is decoded once, straight to its place: there is no sizing pass.  There is no CPU
fallback.

    r = zip.NewReader(data)            # bytes, a numpy array, or an object with read / seek; OpenReader(path)
    r.File[i].Name, .UncompressedSize64, ...
    r.File[i].Open().Read(p)           # that one member, decoded on first use
    r.ReadAll()                        # every member in one batch: a list of bytes, or the error per member

Not built: the fs.FS side (Reader.Open(name), ReadDir), FileHeader.Modified and its time zone rules (ModifiedTime / ModifiedDate
are the raw MS-DOS values), RegisterDecompressor and NewReaderWithOptions, ErrInsecurePath (off by default in the reference), the
Writer (the reference deflates at level 5, for which there is no device writer), and shim/go."""
import ctypes as C

from . import _lib, flate
from .flate import CorruptInputError, ErrUnexpectedEOF  # noqa: F401

Store, Deflate = 0, 8
ZIP_OK, ZIP_FORMAT, ZIP_EOF, ZIP_COMMENT, ZIP_ALGORITHM, ZIP_CHECKSUM, ZIP_READAT, ZIP_SIZE = 0, 16, 17, 18, 19, 20, 21, 22


class ZipError(ValueError):
    """A member or an archive was refused.  `status` is its KC_ZIP_* / KC_FL_* class."""

    def __init__(self, status, text):
        self.status = int(status)
        super().__init__(text)


class ErrFormat(ZipError):
    def __init__(self, status=ZIP_FORMAT):
        super().__init__(status, "zip: not a valid zip file")


class ErrAlgorithm(ZipError):
    def __init__(self, status=ZIP_ALGORITHM):
        super().__init__(status, "zip: unsupported compression algorithm")


class ErrChecksum(ZipError):
    def __init__(self, status=ZIP_CHECKSUM):
        super().__init__(status, "zip: checksum error")


class ErrComment(ZipError):
    def __init__(self, status=ZIP_COMMENT):
        super().__init__(status, "zip: invalid comment length")


class ErrReadAt(ZipError, EOFError):
    """What the io.ReaderAt returns for the thirty bytes of a local header that are not all there: io.EOF."""

    def __init__(self, status=ZIP_READAT):
        super().__init__(status, "EOF")


class ErrSize(ZipError):
    """A limit of this library, not an error of the reference: a member above 1 GiB."""

    def __init__(self, status=ZIP_SIZE):
        super().__init__(status, "zip: member above this library's limit of 1 GiB")


_ERRORS = {flate.FL_CORRUPT: CorruptInputError, flate.FL_EOF: ErrUnexpectedEOF, ZIP_FORMAT: ErrFormat, ZIP_EOF: ErrUnexpectedEOF, ZIP_COMMENT: ErrComment,
           ZIP_ALGORITHM: ErrAlgorithm, ZIP_CHECKSUM: ErrChecksum, ZIP_READAT: ErrReadAt, ZIP_SIZE: ErrSize}


def error_of(status):
    cls = _ERRORS.get(int(status))
    return cls(int(status)) if cls else ZipError(status, "zip: status %d" % status)


class _MemberReader:
    """The io.ReadCloser of File.Open: Read, WriteTo, Close.  The member is decoded on first use; one that fails raises then, and no
    byte of it is handed out."""

    def __init__(self, f):
        self._f, self._out, self._at = f, None, 0

    def _decode(self):
        if self._out is None:
            res = self._f._zip.ReadAll([self._f])[0]
            if isinstance(res, Exception):
                raise res
            self._out = res

    def Read(self, p):
        """Fills p (a writable buffer) and returns the count; 0 at the end."""
        self._decode()
        m = memoryview(p).cast("B")
        n = min(len(m), len(self._out) - self._at)
        m[:n] = self._out[self._at:self._at + n]
        self._at += n
        return n

    def WriteTo(self, w):
        self._decode()
        n = len(self._out) - self._at
        if n:
            w.write(self._out[self._at:])
        self._at = len(self._out)
        return n

    def Close(self):
        self._out, self._at = b"", 0


class File:
    """zip.File: the FileHeader fields of the central directory (struct.go:86-160) and Open / OpenRaw / DataOffset."""

    def __init__(self, z, e, index):
        s = lambda p, n: C.string_at(p, n) if n else b""   # noqa: E731
        self._zip, self._index = z, index
        self.NameBytes, self.CommentBytes, self.Extra = s(e.name, e.name_len), s(e.comment, e.comment_len), s(e.extra, e.extra_len)
        self.NonUTF8 = bool(e.non_utf8)
        enc = "cp437" if self.NonUTF8 else "utf-8"
        self.Name, self.Comment = self.NameBytes.decode(enc, "replace"), self.CommentBytes.decode(enc, "replace")
        self.CreatorVersion, self.ReaderVersion, self.Flags, self.Method = e.creator_version, e.reader_version, e.flags, e.method
        self.ModifiedTime, self.ModifiedDate = e.modified_time, e.modified_date
        self.CRC32, self.CompressedSize64, self.UncompressedSize64 = e.crc32, e.compressed_size64, e.uncompressed_size64
        self.CompressedSize, self.UncompressedSize = min(e.compressed_size64, 0xFFFFFFFF), min(e.uncompressed_size64, 0xFFFFFFFF)
        self.ExternalAttrs, self.headerOffset = e.external_attrs, e.header_offset

    def DataOffset(self):
        """File.DataOffset (reader.go:237-243): where the possibly compressed data starts in the archive."""
        d, off = self._zip._data, self.headerOffset
        if off < 0 or off + 30 > len(d):
            raise ErrReadAt()
        if bytes(d[off:off + 4]) != b"PK\x03\x04":
            raise ErrFormat()
        return off + 30 + int.from_bytes(bytes(d[off + 26:off + 28]), "little") + int.from_bytes(bytes(d[off + 28:off + 30]), "little")

    def OpenRaw(self):
        """File.OpenRaw (:290-297): the bytes of the member without decompression, as an io.BytesIO."""
        import io
        at = self.DataOffset()
        return io.BytesIO(bytes(self._zip._data[at:at + self.CompressedSize64]))

    def Open(self):
        """File.Open (:247-286)."""
        return _MemberReader(self)


class Reader:
    """zip.Reader: File, Comment, and the batch forms ReadAll / ReadAllDevice."""

    def __init__(self, data, device=0):
        import numpy as np
        self._device, self._ctx = device, None
        self._data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        if len(self._data) == 0:
            raise ErrFormat()
        L = _lib.load()
        h = C.c_void_p()
        rc = L.kc_zip_dir_load(self._data.ctypes.data, len(self._data), C.byref(h))
        if rc != ZIP_OK:
            raise error_of(rc)
        try:
            n = L.kc_zip_dir_count(h)
            ln = C.c_uint32()
            p = L.kc_zip_dir_comment(h, C.byref(ln))
            self.CommentBytes = C.string_at(p, ln.value) if ln.value else b""
            self.Comment = self.CommentBytes.decode("utf-8", "replace")
            self.baseOffset = L.kc_zip_dir_base_offset(h)
            self.File = []
            e = _lib.ZipEntry()
            for i in range(n):
                L.kc_zip_dir_entry(h, i, C.byref(e))
                self.File.append(File(self, e, i))
            self._members = (_lib.ZipMember * max(n, 1))()
            L.kc_zip_dir_members(h, 0, n, self._members)
        finally:
            L.kc_zip_dir_free(h)

    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device, None)
        return self._ctx

    def _table(self, files):
        if files is None:
            return self._members, len(self.File)
        t = (_lib.ZipMember * max(len(files), 1))()
        for k, f in enumerate(files):
            if f._zip is not self:
                raise ValueError("zip: a File of another Reader")
            t[k] = self._members[f._index]
        return t, len(files)

    def ReadAll(self, files=None):
        """N x (f.Open(); io.ReadAll; Close) in one batch over every member, or the given ones: a list of bytes, or the error per member."""
        import numpy as np
        t, n = self._table(files)
        ctx = self.ctx()
        out_off, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        ctx.check(ctx.L.kc_zip_read_bound(ctx.h, self._data.ctypes.data, len(self._data), C.addressof(t), n, out_off.ctypes.data, status.ctypes.data))
        cap = int(out_off[n])
        dst = np.empty(cap + 64, dtype=np.uint8)
        ctx.check(ctx.L.kc_zip_read(ctx.h, self._data.ctypes.data, len(self._data), C.addressof(t), n, dst.ctypes.data, cap, out_off.ctypes.data, status.ctypes.data))
        return [error_of(status[i]) if status[i] else dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)]

    def ReadAllDevice(self, d_src_ptr, d_dst_ptr, dst_cap, files=None, stream=None):
        """Device-resident form: the archive's bytes at d_src_ptr, the members decoded to d_dst_ptr.  Returns (uint64[n + 1] offsets,
        uint32[n] status), host numpy.  Raises KcError KC_ERR_DST_TOO_SMALL when the layout does not fit dst_cap (nothing is written)."""
        import numpy as np
        t, n = self._table(files)
        ctx = self.ctx() if stream is None else _lib.Context(self._device, stream)
        try:
            out_off, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
            ctx.check(ctx.L.kc_zip_read_dev(ctx.h, d_src_ptr, len(self._data), C.addressof(t), n, d_dst_ptr, int(dst_cap), out_off.ctypes.data,
                                            status.ctypes.data))
            return out_off, status[:n]
        finally:
            if stream is not None:
                ctx.close()

    def Close(self):
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


def NewReader(r, size=None, device=0):
    """zip.NewReader(r, size): r is bytes, a numpy uint8 array, or an object with read / seek (its first `size` bytes, or all of it)."""
    if hasattr(r, "read"):
        if hasattr(r, "seek"):
            r.seek(0)
        r = r.read() if size is None else r.read(size)
    elif size is not None:
        if size < 0:
            raise ValueError("zip: size cannot be negative")
        r = r[:size]
    return Reader(r, device=device)


def OpenReader(path, device=0):
    """zip.OpenReader(name)."""
    with open(path, "rb") as f:
        return Reader(f.read(), device=device)
