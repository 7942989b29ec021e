"""compress/flate on the device: raw DEFLATE (RFC 1951) inflated in batches of independent inputs, one wave per input
(include/kcgpu.h kc_flate_inflate*; kernels compress_amd/csrc/kc_flate_inflate.hip), and written at flate.HuffmanOnly, the one level
with a device writer (kc_flate_deflate*; kc_flate_deflate.hip: the writer is at the end of this file).  There is no CPU fallback."""
import ctypes as C

from . import _lib

FL_OK, FL_CORRUPT, FL_EOF, FL_HEADER, FL_CHECKSUM, FL_SIZE_EXCEEDED = 0, 1, 2, 3, 4, 5
FL_DICTIONARY = 6
FL_NAMES = {0: "KC_FL_OK", 1: "KC_FL_CORRUPT", 2: "KC_FL_EOF", 3: "KC_FL_HEADER", 4: "KC_FL_CHECKSUM", 5: "KC_FL_SIZE_EXCEEDED",
            6: "KC_FL_DICTIONARY"}


class InflateError(ValueError):
    """An input was refused.  `status` is its KC_FL_* class, `name` that class's name."""

    def __init__(self, status):
        self.status = int(status)
        self.name = FL_NAMES.get(self.status, str(self.status))
        super().__init__("flate: %s" % self.name)


class CorruptInputError(InflateError):
    """flate.CorruptInputError (inflate.go:33-38); the offset is not reported."""

    def __init__(self, status=FL_CORRUPT):
        super().__init__(status)


class ErrUnexpectedEOF(InflateError, EOFError):
    """io.ErrUnexpectedEOF: the input ended inside a block."""

    def __init__(self, status=FL_EOF):
        super().__init__(status)


_ERRORS = {FL_CORRUPT: CorruptInputError, FL_EOF: ErrUnexpectedEOF}


def error_of(status, table=_ERRORS):
    return table.get(int(status), InflateError)(int(status))


class Batch:
    """The batch entry points of one format over one options object and one device context (gzip.py shares it)."""

    def __init__(self, prefix, errors, dict=None, multistream=True, device=0, stream=None):
        L = _lib.load()
        self._prefix, self._errors = prefix, errors
        self._o = C.c_void_p(L.kc_flate_ropts_default())
        if not self._o:
            raise MemoryError("kc_flate_ropts_default")
        if dict:
            d = bytes(dict)
            if L.kc_flate_ropts_dict(self._o, d, len(d)) != 0:
                raise ValueError("flate: dictionary rejected")
        L.kc_flate_ropts_multistream(self._o, 1 if multistream else 0)
        self._device, self._stream, self._ctx = device, stream, None

    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device, self._stream)
        return self._ctx

    def error(self, status):
        return error_of(status, self._errors)

    def bounds(self, src_ptr, in_off, dev):
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        bound, status, used = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        fn = getattr(ctx.L, self._prefix + "_bound" + ("_dev" if dev else ""))
        ctx.check(fn(ctx.h, self._o, src_ptr, in_off.ctypes.data, n, bound.ctypes.data, status.ctypes.data, used.ctypes.data))
        return bound[:n], status[:n], used[:n]

    def inflate(self, src_ptr, in_off, dst_ptr, dst_cap, dev):
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        out_off, status, used = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        fn = getattr(ctx.L, self._prefix + ("_dev" if dev else ""))
        ctx.check(fn(ctx.h, self._o, src_ptr, in_off.ctypes.data, n, dst_ptr, int(dst_cap), out_off.ctypes.data, status.ctypes.data, used.ctypes.data))
        return out_off, status[:n], used[:n]

    def all_host(self, src, in_off, with_consumed=False):
        """The host-buffer form into a buffer of this call's own.  Its size is a guess first (four times the input): when the
        planned layout does not fit, the call has written nothing and out_off[n] says what it takes (include/kcgpu.h), so the call
        is made once more with exactly that — the usual input is walked twice, as a call with a known capacity is, never more than
        three times."""
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        out_off, status, used = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        fn = getattr(ctx.L, self._prefix)
        cap = 4 * int(in_off[-1] - in_off[0]) + (64 << 10)
        while True:
            dst = np.empty(cap + 64, dtype=np.uint8)
            rc = fn(ctx.h, self._o, src.ctypes.data, in_off.ctypes.data, n, dst.ctypes.data, cap, out_off.ctypes.data, status.ctypes.data, used.ctypes.data)
            if rc != _lib.KC_ERR_DST_TOO_SMALL or int(out_off[n]) <= cap:
                break
            cap = int(out_off[n])
        ctx.check(rc)
        res = [self.error(status[i]) if status[i] else dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)]
        return (res, used[:n]) if with_consumed else res

    def close(self):
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self.close()
            if getattr(self, "_o", None):
                _lib.load().kc_flate_ropts_free(self._o)
                self._o = None
        except Exception:
            pass


def InflateAll(src, in_off, dict=None, device=0):
    """N x io.ReadAll(flate.NewReaderDict(input_i, dict)) in one batch.  src: numpy uint8 (host), the inputs concatenated; in_off:
    uint64[n + 1].  Returns a list with, per input, its bytes or the InflateError that refused it."""
    b = Batch("kc_flate_inflate", _ERRORS, dict=dict, device=device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def InflateBounds(src, in_off, dict=None, device=0):
    """The sizing pass alone (kc_flate_inflate_bound): (uint64[n] exact decoded sizes, uint32[n] KC_FL_* status, uint64[n] consumed)."""
    import numpy as np
    b = Batch("kc_flate_inflate", _ERRORS, dict=dict, device=device)
    try:
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        return b.bounds(src.ctypes.data, in_off, False)
    finally:
        b.close()


def InflateAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, dict=None, device=0, stream=None):
    """Device-resident form (pointers are ints): returns (uint64[n + 1] offsets, uint32[n] status, uint64[n] consumed), host numpy.
    A failed input's range is empty.  Raises KcError KC_ERR_DST_TOO_SMALL when the layout does not fit dst_cap (nothing is written)."""
    b = Batch("kc_flate_inflate", _ERRORS, dict=dict, device=device, stream=stream)
    try:
        return b.inflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


class Reader:
    """flate.NewReader / NewReaderDict (inflate.go:929-957) as a reader object: Read, WriteTo, Reset, Close.

    The WHOLE input is read from r and decoded on the device on first use (one input is one wave's work; there is no
    bounded-memory stream reader yet): Read and WriteTo then hand out the decoded bytes.  An input that fails raises on first use;
    no byte of it is handed out."""

    _prefix, _errors = "kc_flate_inflate", _ERRORS

    def __init__(self, r, dict=None, device=0):
        self._device = device
        self.Reset(r, dict)

    def Reset(self, r, dict=None):
        """Resetter.Reset (inflate.go:68-75): read from r, with the preset dictionary dict, from now on."""
        self._r, self._dict, self._out, self._at, self._err = r, dict, None, 0, None

    def _options(self):
        return {"dict": self._dict}

    def _decode(self):
        if self._out is None and self._err is None:
            import numpy as np
            data = self._r.read() if hasattr(self._r, "read") else bytes(self._r)
            self._data = data
            b = Batch(self._prefix, self._errors, device=self._device, **self._options())
            try:
                res, used = b.all_host(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.uint64), with_consumed=True)
            finally:
                b.close()
            self.consumed = int(used[0])
            if isinstance(res[0], InflateError):
                self._err = res[0]
            else:
                self._out = res[0]
        if self._err is not None:
            raise self._err

    def Read(self, p):
        """Fills p (a writable buffer) and returns the count; 0 at the end."""
        self._decode()
        m = memoryview(p).cast("B")
        n = min(len(m), len(self._out) - self._at)
        m[:n] = self._out[self._at:self._at + n]
        self._at += n
        return n

    def WriteTo(self, w):
        """Writes the rest of the decoded bytes to w and returns their count."""
        self._decode()
        n = len(self._out) - self._at
        if n:
            w.write(self._out[self._at:])
        self._at = len(self._out)
        return n

    def Close(self):
        self._out, self._err = b"", None
        self._at = 0


def NewReader(r, device=0):
    """flate.NewReader(r)."""
    return Reader(r, None, device=device)


def NewReaderDict(r, dict, device=0):
    """flate.NewReaderDict(r, dict): only the dictionary's last 32 KiB count."""
    return Reader(r, dict, device=device)


# ---- the writer: flate.NewWriter(w, flate.HuffmanOnly) on the device (include/kcgpu.h kc_flate_deflate*; kernels
# compress_amd/csrc/kc_flate_deflate.hip).  HuffmanOnly is the one level with a device writer; there is no CPU fallback. ----
HuffmanOnly = -2
ConstantCompression = HuffmanOnly  # flate/deflate.go:31-38: the older name of the same level


class WriteBatch:
    """The batch entry points of one writer format over one options object and one device context (gzip.py shares it).
    block / penalty: the two values compressor.init fixes per level (deflate.go:795-799); None keeps HuffmanOnly's 32768 and 10."""

    def __init__(self, prefix, level=HuffmanOnly, flush=False, block=None, penalty=None, device=0, stream=None):
        L = _lib.load()
        self._prefix = prefix
        self._o = C.c_void_p(L.kc_flate_wopts_default())
        if not self._o:
            raise MemoryError("kc_flate_wopts_default")
        rc = L.kc_flate_wopts_level(self._o, int(level))
        if rc != 0:
            raise _lib.KcError(rc, "flate: level %d has no device writer (flate.HuffmanOnly, -2, is the one served)" % level)
        rc = L.kc_flate_wopts_end(self._o, 1 if flush else 0)
        if rc == 0 and (block is not None or penalty is not None):
            rc = L.kc_flate_wopts_block(self._o, 32768 if block is None else int(block), 10 if penalty is None else int(penalty))
        if rc != 0:
            raise _lib.KcError(rc, "flate: writer options rejected")
        self.block = 32768 if block is None else int(block)
        self._device, self._stream, self._ctx = device, stream, None

    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device, self._stream)
        return self._ctx

    def bound(self, in_off):
        """The capacity that holds any output of these inputs (kc_flate_deflate_bound per input; gzip adds 18)."""
        L = _lib.load()
        extra = 18 if "gzip" in self._prefix else 0
        return sum(int(L.kc_flate_deflate_bound(int(in_off[i + 1] - in_off[i]), self.block)) + extra for i in range(len(in_off) - 1))

    def deflate(self, src_ptr, in_off, dst_ptr, dst_cap, dev):
        """One call of the C entry point: uint64[n + 1] out_off.  Raises KcError KC_ERR_DST_TOO_SMALL when the exact total is above
        dst_cap (`.out_off` of the error holds the layout of the device form)."""
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        fn = getattr(ctx.L, self._prefix + ("_dev" if dev else ""))
        try:
            ctx.check(fn(ctx.h, self._o, src_ptr, in_off.ctypes.data, n, dst_ptr, int(dst_cap), out_off.ctypes.data))
        except _lib.KcError as e:
            e.out_off = out_off
            raise
        return out_off

    def all_host(self, src, in_off):
        """The host-buffer form into a buffer of this call's own, sized by the bound: a list of bytes, one per input."""
        import numpy as np
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        cap = self.bound(in_off)
        dst = np.empty(cap + 64, dtype=np.uint8)
        out_off = self.deflate(src.ctypes.data, in_off, dst.ctypes.data, cap, False)
        return [dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)]

    def close(self):
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self.close()
            if getattr(self, "_o", None):
                _lib.load().kc_flate_wopts_free(self._o)
                self._o = None
        except Exception:
            pass


def DeflateBound(n, block=32768):
    """kc_flate_deflate_bound: the most bytes an input of n bytes becomes."""
    return int(_lib.load().kc_flate_deflate_bound(int(n), int(block)))


def DeflateAll(src, in_off, level=HuffmanOnly, flush=False, device=0, block=None, penalty=None):
    """N x (w = flate.NewWriter(buf, level); w.Write(input_i); w.Close()) in one batch, byte for byte; flush=True: w.Flush() in
    Close's place (the stream stays open).  src: numpy uint8 (host), the inputs concatenated; in_off: uint64[n + 1].  Returns a list
    of bytes.  level: flate.HuffmanOnly only (KcError KC_ERR_UNSUPPORTED otherwise)."""
    b = WriteBatch("kc_flate_deflate", level, flush, block, penalty, device=device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def DeflateAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, level=HuffmanOnly, flush=False, device=0, stream=None, block=None, penalty=None):
    """Device-resident form (pointers are ints): returns uint64[n + 1] offsets into d_dst (host numpy).  Raises KcError
    KC_ERR_DST_TOO_SMALL when the exact total is above dst_cap: nothing is written, and the error's .out_off holds the layout."""
    b = WriteBatch("kc_flate_deflate", level, flush, block, penalty, device=device, stream=stream)
    try:
        return b.deflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


class Writer:
    """flate.NewWriter(w, level) (deflate.go:890-897) as a writer object: Write, Close, Reset.

    Write buffers; Close encodes everything written as ONE input on the device and writes the stream to w.  Flush in mid-stream
    would need the writer's state kept across device calls and is not served: it raises."""

    _prefix = "kc_flate_deflate"

    def __init__(self, w, level=HuffmanOnly, device=0):
        if level != HuffmanOnly:
            raise _lib.KcError(_lib.KC_ERR_UNSUPPORTED, "flate: level %d has no device writer (flate.HuffmanOnly, -2, is the one served)" % level)
        self._level, self._device = level, device
        self.Reset(w)

    def Reset(self, w):
        """Writer.Reset (deflate.go:998-1023): what was buffered is dropped; write to w from now on."""
        self._w, self._buf, self._closed = w, bytearray(), False

    def Write(self, p):
        if self._closed:
            raise ValueError("flate: write to closed writer")
        self._buf += bytes(p)
        return len(p)

    def Flush(self):
        raise NotImplementedError("flate: Writer.Flush in mid-stream is not served on the device; DeflateAll(flush=True) ends a whole input with a flush")

    def Close(self):
        if self._closed:
            return
        import numpy as np
        b = WriteBatch(self._prefix, self._level, False, device=self._device)
        try:
            out = b.all_host(np.frombuffer(bytes(self._buf), dtype=np.uint8), np.array([0, len(self._buf)], dtype=np.uint64))[0]
        finally:
            b.close()
        self._closed, self._buf = True, bytearray()
        self._w.write(out)


def NewWriter(w, level=HuffmanOnly, device=0):
    """flate.NewWriter(w, level)."""
    return Writer(w, level, device=device)


# ---- the stateless writer: flate.StatelessDeflate / flate.NewStatelessWriter on the device (include/kcgpu.h kc_flate_stateless_*;
# kernels compress_amd/csrc/kc_flate_stateless.hip): the reference's one LZ77 writer whose blocks are found independently.  It is not a
# level of NewWriter, in the reference or here.  There is no CPU fallback. ----
class StatelessBatch(WriteBatch):
    """The batch entry points of the stateless writers over one options object and one device context (gzip.py shares it)."""

    def __init__(self, prefix="kc_flate_stateless_deflate", eof=True, dict=None, device=0, stream=None):
        L = _lib.load()
        # every field close() and __del__ look at stands before anything can raise
        self._prefix, self._device, self._stream, self._ctx, self._o = prefix, device, stream, None, None
        self._o = C.c_void_p(L.kc_flate_swopts_default())
        if not self._o:
            raise MemoryError("kc_flate_swopts_default")
        dict = bytes(dict) if dict else b""
        rc = L.kc_flate_swopts_eof(self._o, 1 if eof else 0)
        if rc == 0 and dict:
            rc = L.kc_flate_swopts_dict(self._o, dict, len(dict))
        if rc != 0:
            raise _lib.KcError(rc, "flate: stateless writer options rejected")
        self._dict_len = 0 if "gzip" in prefix else len(dict)

    def bound(self, in_off):
        """The capacity that holds any output of these inputs (kc_flate_stateless_bound per input; gzip adds 20)."""
        L = _lib.load()
        extra = 20 if "gzip" in self._prefix else 0
        return sum(int(L.kc_flate_stateless_bound(int(in_off[i + 1] - in_off[i]), self._dict_len)) + extra for i in range(len(in_off) - 1))

    def __del__(self):
        try:
            self.close()
            if getattr(self, "_o", None):
                _lib.load().kc_flate_swopts_free(self._o)
                self._o = None
        except Exception:
            pass


def StatelessBound(n, dict_len=0):
    """kc_flate_stateless_bound: the most bytes an input of n bytes becomes behind a dictionary of dict_len bytes."""
    return int(_lib.load().kc_flate_stateless_bound(int(n), int(dict_len)))


def StatelessDeflateAll(src, in_off, eof=True, dict=None, device=0):
    """N x flate.StatelessDeflate(buf, input_i, eof, dict) in one batch, byte for byte.  src: numpy uint8 (host), the inputs
    concatenated; in_off: uint64[n + 1]; dict: one dictionary for the whole call (its last 8192 bytes count).  Returns a list of
    bytes.  eof=False: every stream ends with an empty stored block and stays open."""
    b = StatelessBatch("kc_flate_stateless_deflate", eof, dict, device=device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def StatelessDeflateAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, eof=True, dict=None, device=0, stream=None):
    """Device-resident form (pointers are ints): returns uint64[n + 1] offsets into d_dst (host numpy).  Raises KcError
    KC_ERR_DST_TOO_SMALL when the exact total is above dst_cap: nothing is written, and the error's .out_off holds the layout."""
    b = StatelessBatch("kc_flate_stateless_deflate", eof, dict, device=device, stream=stream)
    try:
        return b.deflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


def _one(batch, data):
    import numpy as np
    data = bytes(data)
    return batch.all_host(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.uint64))[0]


def StatelessDeflate(out, data, eof, dict=None, device=0):
    """flate.StatelessDeflate(out, in, eof, dict) (stateless.go:76-162): one input, written to out."""
    b = StatelessBatch("kc_flate_stateless_deflate", eof, dict, device=device)
    try:
        out.write(_one(b, data))
    finally:
        b.close()


class StatelessWriter:
    """flate.NewStatelessWriter(w) (stateless.go:21-55): every Write is one non-eof StatelessDeflate on the device, written to w at
    once; Close is the eof call on nothing.  Nothing of the stream is kept between the calls, so the sizes of the Writes shape the
    output.  The object keeps one device context for all its Writes; Close releases it."""

    def __init__(self, w, device=0):
        self._device, self._batch = device, None
        self.Reset(w)

    def Reset(self, w):
        self._w, self._closed = w, False

    def _write_call(self, p):
        if self._batch is None:
            self._batch = StatelessBatch("kc_flate_stateless_deflate", False, None, device=self._device)
        self._w.write(_one(self._batch, p))

    def _release(self):
        b, self._batch = self._batch, None
        if b is not None:
            b.close()

    def Write(self, p):
        self._write_call(p)
        return len(p)

    def Close(self):
        if self._closed:
            return
        self._closed = True
        self._release()
        StatelessDeflate(self._w, b"", True, None, device=self._device)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def NewStatelessWriter(w, device=0):
    """flate.NewStatelessWriter(w)."""
    return StatelessWriter(w, device=device)
