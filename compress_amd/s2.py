"""Host mirror of the reference's S2 API over include/kcgpu.h: the block encoders (s2/encode.go), s2.Writer (s2/writer.go) and, for
reading, s2.Decode / s2.DecodedLen (s2/decode.go) and s2.Reader's DecodeConcurrent with its batched forms (s2/reader.go)."""
import ctypes as C
import threading

from . import _lib


def MaxEncodedLen(src_len):
    """s2.MaxEncodedLen (s2/encode.go:389)."""
    return int(_lib.load().kc_s2_max_encoded_len(int(src_len)))


LevelDefault, LevelBetter, LevelSnappy, LevelSnappyBetter = 0, 1, 2, 3  # s2.Encode / EncodeBetter / EncodeSnappy / EncodeSnappyBetter (s2/encode.go:29, 117, 204, 248)
LevelBest, LevelSnappyBest = 4, 5  # s2.EncodeBest / EncodeSnappyBest (s2/encode.go:146, 278)
LevelUncompressed = 6              # s2.WriterUncompressed (writer.go:951): a level of the stream writer only — every block an uncompressed chunk


class BlockEncoder:
    def __init__(self, device=0, stream=None, level=LevelDefault, path=None, variant=None):
        """path: None / 'auto' (by blocks in flight), 'hbm' or 'lds' — the kernel family of s2.Encode / s2.EncodeSnappy
        (KC_OPT_MATCH_PATH, include/kcgpu.h); both give the reference's bytes.
        variant: None / 'go' — the bytes of the reference's portable Go block encoders (arm64, noasm builds); 'amd64' — the bytes
        of its amd64 assembly encoders (KC_OPT_S2_VARIANT; s2.Encode and s2.EncodeSnappy)."""
        self._ctx = _lib.Context(device, stream)
        if path is not None:
            self._ctx.set_path(path)
        if variant not in (None, "go", "amd64"):
            raise ValueError("variant must be 'go' or 'amd64'")
        if variant == "amd64":
            self._ctx.set_option(20, 1)
        self.level = int(level)
        # the batched calls use the context's stream and scratch: one at a time per encoder (the Go shim's Ctx.mu); the
        # CustomEncoder hook does not take it — the library batches its concurrent callers itself
        self._mu = threading.Lock()

    def ctx(self):
        return self._ctx

    def EncodeBlocks(self, src, blk_off):
        """N x s2.Encode(nil, block).  Returns (numpy uint8, uint64[n+1] offsets)."""
        import numpy as np
        ctx = self._ctx
        src = np.ascontiguousarray(src, dtype=np.uint8)
        blk_off = np.ascontiguousarray(blk_off, dtype=np.uint64)
        n = len(blk_off) - 1
        cap = sum(((MaxEncodedLen(int(blk_off[i + 1] - blk_off[i])) + 15) & ~15) for i in range(n)) + 64
        dst = np.empty(cap, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        with self._mu:
            ctx.check(ctx.L.kc_s2_encode_blocks_lvl(ctx.h, self.level, src.ctypes.data, blk_off.ctypes.data, n, dst.ctypes.data, cap, out_off.ctypes.data))
        return dst[:int(out_off[n])], out_off

    def EncodeBlocksDevice(self, d_src_ptr, blk_off, d_dst_ptr, dst_cap):
        import numpy as np
        ctx = self._ctx
        blk_off = np.ascontiguousarray(blk_off, dtype=np.uint64)
        n = len(blk_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        with self._mu:
            ctx.check(ctx.L.kc_s2_encode_blocks_lvl_dev(ctx.h, self.level, d_src_ptr, blk_off.ctypes.data, n, d_dst_ptr, int(dst_cap), out_off.ctypes.data))
        return out_off

    def EncodeBlocksDeviceBegin(self, d_src_ptr, blk_off):
        """First half of EncodeBlocksDevice (one device batch, bare blocks): enqueue up to and including the encoder kernel, no wait
        (kc_s2_encode_blocks_lvl_dev_begin)."""
        import numpy as np
        ctx = self._ctx
        blk_off = np.ascontiguousarray(blk_off, dtype=np.uint64)
        self._pending_n = len(blk_off) - 1
        with self._mu:
            ctx.check(ctx.L.kc_s2_encode_blocks_lvl_dev_begin(ctx.h, self.level, d_src_ptr, blk_off.ctypes.data, self._pending_n))

    def EncodeBlocksDeviceEnd(self, d_dst_ptr, dst_cap):
        """Second half: the blocks are compacted to d_dst_ptr (named only now: the parts of one batch run as several launches, each part
        right behind the previous one), offsets relative to it (uint64[n+1]), wait."""
        import numpy as np
        ctx = self._ctx
        out_off = np.zeros(self._pending_n + 1, dtype=np.uint64)
        with self._mu:
            ctx.check(ctx.L.kc_s2_encode_blocks_lvl_dev_end_at(ctx.h, d_dst_ptr, int(dst_cap), out_off.ctypes.data))
        return out_off

    def EncodeStreamDevice(self, d_src_ptr, blk_off, d_dst_ptr, dst_cap, with_stream_id=True):
        """s2.Writer framing of the blocks (stream identifier + chunks).  Returns uint64[n+1] chunk offsets."""
        import numpy as np
        ctx = self._ctx
        blk_off = np.ascontiguousarray(blk_off, dtype=np.uint64)
        n = len(blk_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        with self._mu:
            ctx.check(ctx.L.kc_s2_encode_stream_lvl_dev(ctx.h, self.level, d_src_ptr, blk_off.ctypes.data, n, d_dst_ptr, int(dst_cap), out_off.ctypes.data,
                                                        int(with_stream_id)))
        return out_off

    def DecodeBlocksDevice(self, d_enc_ptr, enc_off, d_dst_ptr, dst_off):
        """N x s2.Decode on the device (verifier): returns uint32[n] status, 0 = block decoded to exactly its stated size."""
        import numpy as np
        ctx = self._ctx
        enc_off = np.ascontiguousarray(enc_off, dtype=np.uint64)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.uint64)
        n = len(enc_off) - 1
        status = np.zeros(max(n, 1), dtype=np.uint32)
        with self._mu:
            ctx.check(ctx.L.kc_s2_decode_blocks_dev(ctx.h, d_enc_ptr, enc_off.ctypes.data, n, d_dst_ptr, dst_off.ctypes.data, status.ctypes.data))
        return status[:n]

    def Encode(self, dst, src):
        """s2.Encode(dst, src) (s2/encode.go:29) — or s2.EncodeBetter (:117) for a LevelBetter encoder: uvarint length + block body."""
        import numpy as np
        src = bytes(src)
        out, _ = self.EncodeBlocks(np.frombuffer(src, dtype=np.uint8), np.array([0, len(src)], dtype=np.uint64))
        return out.tobytes()

    def CustomEncoder(self, host_first=0):
        """The function to hand to s2.WriterCustomEncoder (s2/writer.go:1053): fn(dst, src) -> int.  The hook (kc_s2_encode_block)
        encodes at the default level, like the reference's built-in encodeBlock of a default Writer.
        host_first: KC_OPT_S2_HOOK_HOST_FIRST — how many callers at a time the hook leaves to the caller's built-in encoder (fn returns
        -1 for them) before the overflow goes to the device.  This Python façade has no built-in encoder, so its default is 0 (every
        caller to the device); the library's own default (None here: the CPUs of the process) is what the Go shim gets."""
        if self.level != LevelDefault:
            raise ValueError("the WriterCustomEncoder hook serves the default level only (s2.Encode); use EncodeBlocks for level %d" % self.level)
        ctx = self._ctx
        if host_first is not None:
            ctx.set_option(_lib.OPT_S2_HOOK_HOST_FIRST, int(host_first))

        def fn(dst, src):
            src = bytes(src)
            r = ctx.L.kc_s2_encode_block(ctx.h, (C.c_char * len(dst)).from_buffer(dst), len(dst), src, len(src))
            return int(r)
        return fn

    def HookStats(self):
        """(calls, device batches) served by the CustomEncoder hook of this encoder so far."""
        a, b = C.c_uint64(), C.c_uint64()
        self._ctx.L.kc_s2_hook_stats(self._ctx.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def Close(self):
        self._ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# s2.Writer (s2/writer.go) over the device path: the reference's chunking rules decide WHERE the stream is cut (they
# depend on the Write/Flush/EncodeBuffer call pattern), the GPU encodes and frames the chunks in batches.
# ---------------------------------------------------------------------------------------------------------------------
_MIN_BLOCK, _MAX_BLOCK, _DEFAULT_BLOCK = 4 << 10, 4 << 20, 1 << 20  # s2/encode.go minBlockSize/maxBlockSize, writer.go defaultBlockSize
_MAGIC = b"\xff\x06\x00\x00S2sTwO"                                   # magicChunk (s2/s2.go)
_MAGIC_SNAPPY = b"\xff\x06\x00\x00sNaPpY"                            # magicChunkSnappy (s2/s2.go:79-80)


def WriterBlockSize(n):
    def apply(w):
        if n > _MAX_BLOCK or n < _MIN_BLOCK:
            raise ValueError("s2: block size too large. Must be <= 4MB and >=4KB")  # writer.go:985
        w.blockSize = int(n)
    return apply


def WriterConcurrency(n):
    def apply(w):
        if n <= 0:
            raise ValueError("concurrency must be at least 1")  # writer.go:911
        w.concurrency = int(n)  # no effect on bytes: the device batches chunks regardless
    return apply


def WriterFlushOnWrite():
    return lambda w: setattr(w, "flushOnWrite", True)


def _unsupported(name, what="writer"):
    def opt(*a, **k):
        def apply(w):
            raise NotImplementedError("s2.%s is not served by the device path; use the reference %s" % (name, what))
        return apply
    return opt


def WriterBetterCompression():
    """s2.WriterBetterCompression (writer.go:931): blocks are encoded with encodeBlockBetter."""
    return lambda w: setattr(w, "level", LevelBetter)


def WriterBestCompression():
    """s2.WriterBestCompression (writer.go:945): blocks are encoded with encodeBlockBest."""
    return lambda w: setattr(w, "level", LevelBest)


def WriterSnappyCompat():
    """s2.WriterSnappyCompat (writer.go:1025-1037): Snappy-compatible output — the blocks through encodeBlockSnappy /
    encodeBlockBetterSnappy / encodeBlockBestSnappy (no repeat codes), the "sNaPpY" stream identifier, blocks of at most 64 KiB - 8."""
    def apply(w):
        w.snappy = True
        if w.blockSize > (64 << 10):
            w.blockSize = (64 << 10) - 8
    return apply


def WriterUncompressed():
    """s2.WriterUncompressed (writer.go:948-956): bypass compression — the stream is uncompressed chunks only (type 0x01 | length |
    masked CRC32C | bytes; the checksum and the copy run on the device).  A level like the others: a later level option replaces it."""
    return lambda w: setattr(w, "level", LevelUncompressed)


def WriterAddIndex():
    """s2.WriterAddIndex (writer.go:921): append the seek index to the stream on Close."""
    return lambda w: setattr(w, "appendIndex", True)


def WriterPadding(n):
    """s2.WriterPadding (writer.go:999): pad the output to a multiple of n with a skippable 0xfe chunk on Close."""
    def apply(w):
        if n <= 0:
            raise ValueError("s2: padding must be at least 1")
        if n > _MAX_BLOCK:
            raise ValueError("s2: padding must less than 4MB")
        w.pad = int(n)
    return apply


def WriterPaddingSrc(reader):
    """s2.WriterPaddingSrc (writer.go:1018): where the padding bytes come from (default: os.urandom, like crypto/rand)."""
    return lambda w: setattr(w, "randSrc", reader)


def calc_skippable_frame(written, want_multiple):
    """calcSkippableFrame (writer.go:858): bytes to add so that `written` becomes a multiple; 0 or >= 4."""
    left = written % want_multiple
    if left == 0:
        return 0
    add = want_multiple - left
    while add < 4:
        add += want_multiple
    return add


class Index:
    """s2.Index (s2/index.go).  The writer side — add / reduce / appendTo (:17-236) — is Python; the reader side — Load, LoadStream,
    Find (:97-127, 238-413) — runs in the library's host code (kc_s2_index.cpp), which checks every read of the untrusted bytes."""
    MAX_ENTRIES, MIN_DIST = 1 << 16, 1 << 20

    def __init__(self, max_block=0):
        self.est = int(max_block)
        self.info = []  # [compressedOffset, uncompressedOffset]
        self.TotalUncompressed = -1
        self.TotalCompressed = -1
        self._h = None

    def _adopt(self, h, rc):
        L = _lib.load()
        if rc:
            L.kc_s2_index_free(h)
            raise S2DecodeError(rc)
        import numpy as np
        n = L.kc_s2_index_entries(h, None, None, 0)
        c, u = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        L.kc_s2_index_entries(h, c.ctypes.data, u.ctypes.data, n)
        self.info = [[int(c[k]), int(u[k])] for k in range(n)]
        self.TotalUncompressed = int(L.kc_s2_index_total_uncompressed(h))
        self.TotalCompressed = int(L.kc_s2_index_total_compressed(h))
        self.est = int(L.kc_s2_index_est_block_uncompressed(h))
        self._drop()
        self._h = C.c_void_p(h)

    def _drop(self):
        h, self._h = self._h, None
        if h:
            _lib.load().kc_s2_index_free(h)

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def Load(self, b):
        """Index.Load (index.go:238): read a binary index from the front of b and return the rest.  Raises S2DecodeError with the class
        of the reference's error (KC_S2D_UNEXPECTED_EOF, KC_S2D_CORRUPT, KC_S2D_UNSUPPORTED)."""
        b = bytes(b)
        L = _lib.load()
        h = L.kc_s2_index_new()
        used = C.c_uint64(0)
        self._adopt(h, L.kc_s2_index_load(h, b, len(b), C.byref(used)))
        return b[used.value:]

    def LoadStream(self, stream):
        """Index.LoadStream (index.go:381) over the bytes of a whole stream: the index is looked for at its end."""
        stream = bytes(stream)
        L = _lib.load()
        h = L.kc_s2_index_new()
        self._adopt(h, L.kc_s2_index_load_stream(h, stream, len(stream)))

    def _handle(self):
        """The library's copy of this index (made by Load / LoadStream, else from the bytes appendTo would write)."""
        if self._h is None:
            w = Index(self.est)
            w.info = [list(e) for e in self.info]
            self.Load(w.append_to(self.TotalUncompressed, self.TotalCompressed))
        return self._h

    def Find(self, offset):
        """Index.Find (index.go:97): (compressed offset, uncompressed offset) of the entry at or before `offset`; a negative offset counts
        from the end.  Raises S2DecodeError (KC_S2D_UNEXPECTED_EOF outside the stream, KC_S2D_CORRUPT without a known total)."""
        c, u = C.c_int64(0), C.c_int64(0)
        rc = _lib.load().kc_s2_index_find(self._handle(), int(offset), C.byref(c), C.byref(u)) if self.TotalUncompressed >= 0 else 1
        if rc:
            raise S2DecodeError(rc)
        return c.value, u.value

    def JSON(self):
        """Index.JSON (index.go:519): the index as JSON text, in the reference's field names and two-space indent."""
        import json
        x = {"total_uncompressed": self.TotalUncompressed, "total_compressed": self.TotalCompressed,
             "offsets": [{"compressed": c, "uncompressed": u} for c, u in self.info] or None, "est_block_uncompressed": self.est}
        return json.dumps(x, indent=2).encode()

    def add(self, comp, unc):
        if self.info:
            latest = self.info[-1]
            if latest[1] == unc:
                latest[0] = comp
                return
            if latest[1] > unc or latest[0] > comp:
                raise ValueError("internal error: earlier offset received")
            if latest[1] + self.MIN_DIST > unc:
                return
        self.info.append([comp, unc])

    def _reduce(self):
        if len(self.info) < self.MAX_ENTRIES and self.est >= self.MIN_DIST:
            return
        remove_n = (len(self.info) + 1) // self.MAX_ENTRIES
        while self.est * (remove_n + 1) < self.MIN_DIST and len(self.info) // (remove_n + 1) > 1000:
            remove_n += 1
        self.info = self.info[::remove_n + 1]
        self.est += self.est * remove_n

    @staticmethod
    def _varint(x):
        ux = (x << 1) ^ (x >> 63) if x >= 0 else ((~x) << 1) | 1
        ux &= (1 << 64) - 1
        out = bytearray()
        while ux >= 0x80:
            out.append((ux & 0x7F) | 0x80)
            ux >>= 7
        out.append(ux)
        return bytes(out)

    def append_to(self, uncomp_total, comp_total):
        self._reduce()
        b = bytearray(b"\x99\x00\x00\x00s2idx\x00")
        for v in (uncomp_total, comp_total, self.est, len(self.info)):
            b += self._varint(v)
        has_unc = 0
        for i, (_, u) in enumerate(self.info):
            if (i == 0 and u != 0) or (i > 0 and u != self.info[i - 1][1] + self.est):
                has_unc = 1
                break
        b.append(has_unc)
        if has_unc:
            for i, (_, u) in enumerate(self.info):
                b += self._varint(u - (self.info[i - 1][1] + self.est) if i else u)
        c_predict = self.est // 2
        for i, (c, _) in enumerate(self.info):
            c_off = c
            if i:
                c_off -= self.info[i - 1][0] + c_predict
                c_predict += c_off // 2 if c_off >= 0 else -((-c_off) // 2)  # Go integer division truncates toward zero
            b += self._varint(c_off)
        b += (len(b) + 4 + 6).to_bytes(4, "little")
        b += b"\x00xdi2s"
        n = len(b) - 4
        b[1:4] = bytes([n & 0xFF, (n >> 8) & 0xFF, (n >> 16) & 0xFF])
        return bytes(b)


class Writer:
    """s2.Writer: Write / ReadFrom / EncodeBuffer / AddSkippableBlock / Flush / Close / Reset with the reference's chunk
    boundaries (writer.go:182-218, 357-453, 483-571, 741-857); default, better or best level (WriterBetterCompression / WriterBestCompression).  Chunks are queued and
    encoded on the GPU in batches of `batch_bytes`; the bytes written equal the reference's for the same call sequence."""

    def __init__(self, w, *opts, device=0, stream=None, batch_bytes=256 << 20, variant=None):
        self.blockSize = _DEFAULT_BLOCK
        self.concurrency = 1
        self.flushOnWrite = False
        self.appendIndex = False
        self.pad = 0
        self.randSrc = None
        self.level = LevelDefault
        self.snappy = False
        for o in opts:
            o(self)
        if self.snappy:  # (*Writer).encodeBlock, writer.go:1053-1091: the Snappy-compatible block encoder of the level
            if self.blockSize > (64 << 10):
                raise ValueError("s2: block size too large. Must be <= 64K and >=4KB on for snappy compatible output")  # writer.go:982
            self.level = {LevelDefault: LevelSnappy, LevelBetter: LevelSnappyBetter, LevelBest: LevelSnappyBest, LevelUncompressed: LevelUncompressed}[self.level]
        self._enc = BlockEncoder(device, stream, level=self.level, variant=variant)  # variant: see BlockEncoder
        self._device = device
        self._batch = int(batch_bytes)
        self.Reset(w)

    def Reset(self, w):
        self.writer = w
        self._ibuf = bytearray()
        self._queue = []       # ("c", bytes) data chunk | ("r", bytes) raw bytes to pass through (skippable blocks)
        self._queued = 0
        self._wroteHeader = False
        self._closed = False
        self.written = 0
        self.uncompWritten = 0
        self._index = Index(self.blockSize)
        self._flushedUncomp = 0  # uncompressed start offset of the next chunk to be written out

    # -- chunk cutting, exactly as writer.go --
    def _write(self, p):  # writer.go:483 write(): everything in p becomes chunks now, the last one may be short
        mv = memoryview(p)
        for i in range(0, len(mv), self.blockSize):
            self._queue.append(("c", bytes(mv[i:i + self.blockSize])))
        self._queued += len(mv)
        self.uncompWritten += len(mv)
        if self._queued >= self._batch:
            self._drain()

    def Write(self, p):
        if self._closed:
            raise IOError("s2: Writer is closed")
        p = bytes(p)
        if self.flushOnWrite:
            self._write(p)
            return len(p)
        n_ret = 0
        while len(p) > self.blockSize - len(self._ibuf):  # writer.go:190
            if len(self._ibuf) == 0:
                self._write(p)  # large write, empty buffer: all of p, including its tail
                n = len(p)
            else:
                n = self.blockSize - len(self._ibuf)
                self._ibuf += p[:n]
                self._write(self._ibuf)
                self._ibuf = bytearray()
            n_ret += n
            p = p[n:]
        self._ibuf += p
        return n_ret + len(p)

    def EncodeBuffer(self, buf):  # writer.go:357
        if self._closed:
            raise IOError("s2: Writer is closed")
        if self.flushOnWrite:
            self._write(bytes(buf))
            return
        if self._ibuf:
            self._async_flush()
        self._write(bytes(buf))

    def ReadFrom(self, r):  # writer.go:220: blockSize reads until EOF
        if self._closed:
            raise IOError("s2: Writer is closed")
        if self._ibuf:
            self._async_flush()
        n = 0
        while True:
            b = r.read(self.blockSize)
            while b and len(b) < self.blockSize:  # io.ReadFull
                more = r.read(self.blockSize - len(b))
                if not more:
                    break
                b += more
            if not b:
                break
            n += len(b)
            self._write(b)
            if len(b) < self.blockSize:
                break
        return n

    def AddSkippableBlock(self, id, data):  # writer.go:272
        data = bytes(data)
        if len(data) == 0:
            return
        if id < 0x80 or id > 0xfe:
            raise ValueError("invalid skippable block id %x" % id)
        if len(data) > 0xFFFFFF:
            raise ValueError("skippable block excessed maximum size")
        self._queue.append(("r", bytes([id, len(data) & 0xFF, (len(data) >> 8) & 0xFF, (len(data) >> 16) & 0xFF]) + data))

    def _async_flush(self):  # writer.go:741
        if self._ibuf:
            b = bytes(self._ibuf)
            self._ibuf = bytearray()
            self._write(b)

    def Flush(self):
        if self._closed:
            return
        self._async_flush()
        self._drain()

    def Close(self):
        """writer.go:787: Flush, then the index chunk if WriterAddIndex was given."""
        self._close_index(self.appendIndex)

    def CloseIndex(self):
        """writer.go:794: Close and return the index (it is also appended to the stream only with WriterAddIndex)."""
        return self._close_index(True)

    def _close_index(self, want):
        if self._closed:
            return None
        self.Flush()
        self._closed = True
        index = None
        if want:  # writer.go:808-818: the compressed total is unknown to the index when padding follows
            index = self._index.append_to(self.uncompWritten, self.written if self.pad <= 1 else -1)
            if self.appendIndex:
                self.written += len(index)
        if self.pad > 1:  # writer.go:820-836: the padding chunk goes out BEFORE the index, sized as if the index were written
            add = calc_skippable_frame(self.written, self.pad)
            if add:
                if add >= _MAX_BLOCK + 4:
                    raise ValueError("s2: requested skippable frame (%d) >= max 1<<24" % add)
                f = add - 4
                fill = self.randSrc.read(f) if self.randSrc is not None else __import__("os").urandom(f)
                if len(fill) != f:
                    raise IOError("short read from the padding source")
                self.writer.write(bytes([0xfe, f & 0xFF, (f >> 8) & 0xFF, (f >> 16) & 0xFF]) + fill)
        if index is not None and self.appendIndex:
            self.writer.write(index)
        return index

    # -- device batch --
    def _drain(self):
        import numpy as np
        import torch
        out = []  # (bytes, uncompressed start offset) per write to the underlying writer, in stream order
        i = 0
        q = self._queue
        while i < len(q):
            if q[i][0] == "r":
                if not self._wroteHeader:  # the stream identifier precedes the first output of any kind
                    out.append((_MAGIC_SNAPPY if self.snappy else _MAGIC, self._flushedUncomp))
                    self._wroteHeader = True
                out.append((q[i][1], self._flushedUncomp))
                i += 1
                continue
            j = i
            while j < len(q) and q[j][0] == "c":
                j += 1
            chunks = [c[1] for c in q[i:j]]
            off = np.zeros(len(chunks) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(c) for c in chunks])
            src = np.frombuffer(b"".join(chunks), dtype=np.uint8)
            d_src = torch.from_numpy(src.copy()).cuda(self._device)
            cap = sum(((MaxEncodedLen(len(c)) + 8 + 15) & ~15) for c in chunks) + 64
            d_dst = torch.empty(cap, dtype=torch.uint8, device=d_src.device)
            with_id = not self._wroteHeader
            oo = self._enc.EncodeStreamDevice(d_src.data_ptr(), off, d_dst.data_ptr(), cap, with_stream_id=with_id and not self.snappy)
            self._wroteHeader = True
            blob = d_dst[:int(oo[-1])].cpu().numpy().tobytes()
            if with_id and self.snappy:
                out.append((_MAGIC_SNAPPY, self._flushedUncomp))
            elif with_id:
                out.append((blob[:int(oo[0])], self._flushedUncomp))
            for k, c in enumerate(chunks):
                out.append((blob[int(oo[k]):int(oo[k + 1])], self._flushedUncomp))
                self._flushedUncomp += len(c)
            i = j
        self._queue = []
        self._queued = 0
        for b, start in out:  # the writer goroutine of writer.go:146-170: index entry, then the bytes
            self._index.add(self.written, start)
            self.writer.write(b)
            self.written += len(b)

    def CloseDevice(self):
        self._enc.Close()


def NewWriter(w, *opts, **kw):
    return Writer(w, *opts, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# s2.Reader / s2.Decode (s2/reader.go, s2/decode.go) over the device path: whole inputs, in batches.  Every input is decoded
# as io.ReadAll(s2.NewReader(input)) would; ranged reads go through Reader.ReadRanges and the cursor s2.NewReadSeeker returns.
# The methods Read, Skip, ReadSeeker, ReadByte of Reader itself raise; reading one stream piece by piece, with skippable-chunk
# callbacks, is StreamReader (NewStreamReader) further down.
# ---------------------------------------------------------------------------------------------------------------------
class S2DecodeError(ValueError):
    """The reader refused an input.  `name` is the class of the reference's error: KC_S2D_CORRUPT (ErrCorrupt), KC_S2D_CRC (ErrCRC),
    KC_S2D_UNSUPPORTED (ErrUnsupported), KC_S2D_SIZE_EXCEEDED (an input too large for the scratch ceiling of a host-buffer call),
    KC_S2D_EOF / KC_S2D_UNEXPECTED_EOF (ranged reads, Skip), or KC_S2D_CALLBACK (the stream reader: a skippable-chunk callback failed)."""

    def __init__(self, status):
        self.status = int(status)
        self.name = _lib.S2D_NAMES.get(self.status, str(self.status))
        super().__init__("s2: %s" % self.name)


def DecodedLen(src):
    """s2.DecodedLen (s2/decode.go:29-47), on the host: the uvarint in front of a block, at most 5 bytes and 32 bits."""
    src = bytes(src[:6])
    v = 0
    for i, b in enumerate(src[:5]):
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            if v > 0xFFFFFFFF:
                break
            return v
    raise S2DecodeError(1)


def _ropt(name, *args):
    def apply(r):
        if getattr(_lib.load(), "kc_s2_ropts_" + name)(r._o, *args) != 0:
            raise ValueError("s2 reader option %s rejected" % name)
    return apply


def ReaderMaxBlockSize(n):
    """s2.ReaderMaxBlockSize (reader.go:64): larger blocks are refused as corrupt.  Default and maximum 4 MiB."""
    if n > _MAX_BLOCK or n <= 0:
        raise ValueError("s2: block size too large. Must be <= 4MB and > 0")
    return _ropt("max_block_size", int(n))


def ReaderAllocBlock(n):
    """s2.ReaderAllocBlock (reader.go:82): validated like the reference's; the device path has no buffer of that kind to size."""
    if n > _MAX_BLOCK or n < 1024:
        raise ValueError("s2: invalid ReaderAllocBlock. Must be <= 4MB and >= 1024")
    return lambda r: None


def ReaderIgnoreCRC():
    """s2.ReaderIgnoreCRC (reader.go:120)."""
    return _ropt("ignore_crc", 1)


def ReaderIgnoreStreamIdentifier():
    """s2.ReaderIgnoreStreamIdentifier (reader.go:95)."""
    return _ropt("ignore_stream_identifier", 1)


ReaderSkippableCB = _unsupported("ReaderSkippableCB", "reader")


class Reader:
    """s2.Reader for whole inputs: DecodeConcurrent, and its batched forms DecodeStreams (host buffers) / DecodeStreamsDevice
    (device-resident) and DecodeBlocks / DecodeBlocksDevice for bare blocks.  An input is what s2.NewReader reads: any concatenation
    of .s2 or Snappy-framed streams.  A failed input keeps its planned range in the output, zero-filled (include/kcgpu.h)."""

    def __init__(self, r, *opts, device=0, stream=None):
        L = _lib.load()
        self._o = C.c_void_p(L.kc_s2_ropts_default())
        if not self._o:
            raise MemoryError("kc_s2_ropts_default")
        for op in opts:
            op(self)
        self._device, self._stream = device, stream
        self._ctx = None
        self._r = r

    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device, self._stream)
        return self._ctx

    def Reset(self, r):
        """Reader.Reset (reader.go:177): read from r from now on; the options stay."""
        self._r = r

    def DecodeConcurrent(self, w, concurrent=0):
        """Reader.DecodeConcurrent (reader.go:413): decode the whole of r to w, as one call.  Returns the bytes written; raises
        S2DecodeError with the class of the reference's error (nothing is written then)."""
        import numpy as np
        data = self._r.read() if hasattr(self._r, "read") else bytes(self._r)
        out = self.DecodeStreams(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.uint64))[0]
        if isinstance(out, S2DecodeError):
            raise out
        w.write(out)
        return len(out)

    def _host(self, fn_bound, fn, with_opts, src, in_off):
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        o = (self._o,) if with_opts else ()
        bound = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        ctx.check(getattr(ctx.L, fn_bound)(ctx.h, *o, src.ctypes.data, in_off.ctypes.data, n, bound.ctypes.data, status.ctypes.data))
        if fn is None:
            return bound[:n], status[:n]
        cap = int(bound[:n].sum())
        dst = np.empty(cap + 64, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        ctx.check(getattr(ctx.L, fn)(ctx.h, *o, src.ctypes.data, in_off.ctypes.data, n, dst.ctypes.data, cap, out_off.ctypes.data, status.ctypes.data))
        return [S2DecodeError(status[i]) if status[i] else dst[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)]

    def _dev(self, fn, with_opts, d_src_ptr, in_off, d_dst_ptr=None, dst_cap=0):
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        o = (self._o,) if with_opts else ()
        first = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        if d_dst_ptr is None:
            ctx.check(getattr(ctx.L, fn)(ctx.h, *o, d_src_ptr, in_off.ctypes.data, n, first.ctypes.data, status.ctypes.data))
            return first[:n], status[:n]
        ctx.check(getattr(ctx.L, fn)(ctx.h, *o, d_src_ptr, in_off.ctypes.data, n, d_dst_ptr, int(dst_cap), first.ctypes.data, status.ctypes.data))
        return first, status[:n]

    def DecodeBounds(self, src, in_off, blocks=False):
        """The plan alone (kc_s2_decode_streams_bound): per input the bytes it decodes to — from the chunk headers, exact if the input
        stands — and the first header-level error.  blocks=True: the inputs are bare blocks (N x s2.DecodedLen).  Returns (uint64[n],
        uint32[n])."""
        if blocks:
            return self._host("kc_s2_decode_blocks_all_bound", None, False, src, in_off)
        return self._host("kc_s2_decode_streams_bound", None, True, src, in_off)

    def DecodeStreams(self, src, in_off):
        """N x io.ReadAll(s2.NewReader(input_i)) in one batch.  src: numpy uint8 (host), in_off: uint64[n+1].  Returns a list with, per
        input, its bytes or the S2DecodeError that refused it."""
        return self._host("kc_s2_decode_streams_bound", "kc_s2_decode_streams", True, src, in_off)

    def DecodeBlocks(self, src, in_off):
        """N x s2.Decode(nil, block_i) in one batch (bare blocks, S2 or Snappy): a list of bytes or S2DecodeError."""
        return self._host("kc_s2_decode_blocks_all_bound", "kc_s2_decode_blocks_all", False, src, in_off)

    def DecodeBoundsDevice(self, d_src_ptr, in_off, blocks=False):
        """DecodeBounds over device-resident inputs (kc_s2_decode_streams_bound_dev): their sum is what d_dst must hold."""
        if blocks:
            return self._dev("kc_s2_decode_blocks_all_bound_dev", False, d_src_ptr, in_off)
        return self._dev("kc_s2_decode_streams_bound_dev", True, d_src_ptr, in_off)

    def DecodeStreamsDevice(self, d_src_ptr, in_off, d_dst_ptr, dst_cap):
        """Device-resident form (pointers are ints): returns (uint64[n+1] planned offsets, uint32[n] status), host numpy.  A failed
        input's range is zero-filled.  Raises KcError KC_ERR_DST_TOO_SMALL when the layout does not fit dst_cap (nothing is written)."""
        return self._dev("kc_s2_decode_streams_dev", True, d_src_ptr, in_off, d_dst_ptr, dst_cap)

    def DecodeBlocksDevice(self, d_src_ptr, in_off, d_dst_ptr, dst_cap):
        """DecodeBlocks over device-resident blocks (kc_s2_decode_blocks_all_dev): (uint64[n+1] offsets, uint32[n] status)."""
        return self._dev("kc_s2_decode_blocks_all_dev", False, d_src_ptr, in_off, d_dst_ptr, dst_cap)

    def _ranges(self, fn, src_ptr, in_off, requests, indexes, dst_ptr, dst_cap):
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        ns = len(in_off) - 1
        m = len(requests)
        rs = np.ascontiguousarray([r[0] for r in requests] + [0], dtype=np.uint32)
        ro = np.ascontiguousarray([r[1] for r in requests] + [0], dtype=np.uint64)
        rl = np.ascontiguousarray([r[2] for r in requests] + [0], dtype=np.uint64)
        keep = []
        ix = None
        if indexes is not None:
            if len(indexes) != ns:
                raise ValueError("s2: one index (or None) per input")
            ix = (C.c_void_p * max(ns, 1))()
            for k, i in enumerate(indexes):
                if i is None:
                    continue
                if not isinstance(i, Index):  # the bytes of an index
                    b, i = i, Index()
                    i.Load(b)
                keep.append(i)
                ix[k] = i._handle()
        out_off = np.zeros(m + 1, dtype=np.uint64)
        got = np.zeros(max(m, 1), dtype=np.uint64)
        status = np.zeros(max(m, 1), dtype=np.uint32)
        ctx.check(getattr(ctx.L, fn)(ctx.h, self._o, src_ptr, in_off.ctypes.data, ns, ix, rs.ctypes.data, ro.ctypes.data, rl.ctypes.data, m, dst_ptr,
                                     int(dst_cap), out_off.ctypes.data, got.ctypes.data, status.ctypes.data))
        return out_off, got[:m], status[:m]

    def ReadRangesDevice(self, d_src_ptr, in_off, requests, d_dst_ptr, dst_cap, indexes=None):
        """N x ReadSeeker.ReadAt over device-resident inputs (kc_s2_read_ranges_dev).  requests: (input, offset, length) triples;
        indexes: per input an Index, the bytes of one, or None (the input is then walked from its start).  Request j owns
        d_dst[out_off[j]:out_off[j + 1]], out_off being the prefix sum of the lengths.  Returns (out_off uint64[m + 1], got uint64[m],
        status uint32[m]); status KC_S2D_EOF is a short read (got < length, the rest zero-filled), any other non-zero status leaves
        the range zero-filled.  Raises KcError KC_ERR_DST_TOO_SMALL when the lengths do not fit dst_cap (nothing is written)."""
        return self._ranges("kc_s2_read_ranges_dev", d_src_ptr, in_off, requests, indexes, d_dst_ptr, dst_cap)

    def ReadRanges(self, src, in_off, requests, indexes=None):
        """ReadRangesDevice over host buffers (kc_s2_read_ranges): per request only the compressed bytes its index entry points at are
        staged.  Returns a list with, per request, (bytes, status): the bytes it got (fewer than asked for with KC_S2D_EOF, b"" with
        any other non-zero status)."""
        import numpy as np
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        cap = sum(int(r[2]) for r in requests)
        dst = np.empty(cap + 64, dtype=np.uint8)
        out_off, got, status = self._ranges("kc_s2_read_ranges", src.ctypes.data, in_off, requests, indexes, dst.ctypes.data, cap)
        return [(dst[int(out_off[j]):int(out_off[j]) + int(got[j])].tobytes(), int(status[j])) for j in range(len(requests))]

    def Read(self, p):
        _unsupported("Reader.Read", "reader")()(self)

    def Skip(self, n):
        _unsupported("Reader.Skip", "reader")()(self)

    def ReadSeeker(self, random=False, index=None):
        _unsupported("Reader.ReadSeeker", "reader")()(self)

    def ReadByte(self):
        _unsupported("Reader.ReadByte", "reader")()(self)

    def Close(self):
        """The device context is released (and re-created on the next use)."""
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self.Close()
            if getattr(self, "_o", None):
                _lib.load().kc_s2_ropts_free(self._o)
                self._o = None
        except Exception:
            pass


def NewReader(r, *opts, **kw):
    """s2.NewReader(r, opts...) (reader.go:31)."""
    return Reader(r, *opts, **kw)


class StreamReader:
    """s2.NewReader(r) as a stream reader (reader.go:249-405, :674-842, :1044): Read / Skip / ReadByte / ReadSeeker decode r piece by
    piece in bounded memory (kc_s2_rstream_feed: up to KC_OPT_S2_RSTREAM_CHUNKS data chunks per launch, one wave per chunk).  It takes
    the reader options of Reader.  skippable: {id: fn} (ReaderSkippableCB, reader.go:109; 0x80 <= id <= 0xfd) — fn(reader) gets a
    file-like object over the chunk's content; an exception it raises aborts the stream and is re-raised.  batch_bytes: how much is
    pulled from r, and decoded, at a time.  s2.Reader stays the reader for whole inputs and batches."""

    def __init__(self, r, *opts, skippable=None, batch_bytes=32 << 20, device=0, stream=None):
        from . import zstd as _zstd
        L = _lib.load()
        self._opts = opts
        self._o = C.c_void_p(L.kc_s2_ropts_default())
        if not self._o:
            raise MemoryError("kc_s2_ropts_default")
        for op in opts:
            op(self)
        for id in (skippable or {}):
            if not 0x80 <= int(id) <= 0xfd:
                raise ValueError("ReaderSkippableCB: Invalid id provided, must be 0x80-0xfd (inclusive)")
        self._skippable = dict(skippable or {})
        self._device, self._stream = device, stream
        self._batch_bytes = batch_bytes
        self._ctx = _lib.Context(device, stream)
        self._cb_err = None
        self._parts = {}
        self._fn = _lib.S2_SKIPPABLE_FN(self._on_piece)  # (kept alive as long as the stream)
        self._r = r
        self._sb = _zstd.StreamBuffer(self._new, L.kc_s2_rstream_feed, L.kc_s2_rstream_free, r, batch_bytes, min_cap=_MAX_BLOCK,
                                      what="s2 stream reader")

    def ctx(self):
        return self._ctx

    def _new(self):
        L = self._ctx.L
        h = L.kc_s2_rstream_new(self._ctx.h, self._o)
        if h:
            for id in self._skippable:
                self._ctx.check(L.kc_s2_rstream_on_skippable(h, int(id), self._fn, None))
        return h

    def _on_piece(self, user, id, piece, n, left):
        try:
            self._parts.setdefault(id, []).append(C.string_at(piece, n) if n else b"")
            if left == 0:
                import io
                content = b"".join(self._parts.pop(id))
                self._skippable[id](io.BytesIO(content))
            return 0
        except BaseException as e:  # noqa: BLE001 (it is raised again where the stream's error surfaces)
            self._cb_err = e
            return 1

    def _buffer(self):
        if self._sb is None:
            raise ValueError("s2: StreamReader used after Close")
        return self._sb

    def _raise(self, status):
        if status == 7 and self._cb_err is not None:
            raise self._cb_err
        raise S2DecodeError(status)

    def Read(self, p):
        """Reader.Read (reader.go:249): fills p from the decoded stream and returns the count (fewer than len(p) only at the stream's
        end or in front of its error); 0 at the end.  S2DecodeError is raised only once the bytes in front of the error have been
        returned.  An empty p with nothing buffered advances to the next data chunk and fires the callbacks on the way."""
        sb = self._buffer()
        if len(p) == 0:
            if not sb.fill() and sb.status:
                self._raise(sb.status)
            return 0
        n = sb.read_into(p)
        if n == 0 and sb.status:
            self._raise(sb.status)
        return n

    def Skip(self, n):
        """Reader.Skip (reader.go:674): n decoded bytes forward — buffered bytes first, the rest by the chunk headers (the bodies of
        the chunks passed are not decoded).  Raises only if the skip could not be completed: KC_S2D_UNEXPECTED_EOF when the input ends
        first, else the class of the error met; an error behind a completed skip waits for the next Read."""
        if n < 0:
            raise ValueError("attempted negative skip")
        sb = self._buffer()
        n -= sb.drop(n)
        if n == 0:
            return
        if sb.status:
            self._raise(sb.status)
        if sb.done:
            raise S2DecodeError(6)
        L = self._ctx.L
        self._ctx.check(L.kc_s2_rstream_skip(sb.handle, int(n)))
        while L.kc_s2_rstream_skip_left(sb.handle) and not sb.buffered() and not sb.status and not sb.done:
            sb.step()
        if L.kc_s2_rstream_skip_left(sb.handle):
            self._raise(sb.status or 6)

    def ReadByte(self):
        """Reader.ReadByte (reader.go:1044); raises EOFError at the end of the stream."""
        p = bytearray(1)
        if self.Read(p) != 1:
            raise EOFError("EOF")
        return p[0]

    def Reset(self, r):
        """Reader.Reset (reader.go:177): read from r from now on; options and callbacks stay, and so do the stream's device buffers and
        the host buffer (kc_s2_rstream_reset, which also takes KC_OPT_S2_RSTREAM_CHUNKS as the context holds it now)."""
        sb = self._buffer()
        self._ctx.check(self._ctx.L.kc_s2_rstream_reset(sb.handle))
        self._cb_err, self._parts, self._r = None, {}, r
        sb.restart(r)

    def ReadSeeker(self, random=False, index=None):
        """Reader.ReadSeeker (reader.go:864-1000).  random=False: a forward-only seeker over this stream (reader.go:968-975).
        random=True: r must be seekable (ErrCantSeek otherwise); the whole-input s2.ReadSeeker over r is returned."""
        if not random:
            ix = None
            if index is not None and len(index) != 0:
                ix = Index()
                try:
                    ix.Load(index)
                except S2DecodeError as e:
                    raise ErrCantSeek("loading index returned: " + str(e))
            return _ForwardSeeker(self, ix)
        if not hasattr(self._r, "seek"):
            raise ErrCantSeek("input stream isn't seekable")
        self._r.seek(0)
        return ReadSeeker(self._r, *self._opts, random=True, index=index, device=self._device, stream=self._stream)

    def Close(self):
        """Releases the stream, its device buffers and the context."""
        sb, self._sb = self._sb, None
        if sb is not None:
            sb.close()
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self.Close()
            if getattr(self, "_o", None):
                _lib.load().kc_s2_ropts_free(self._o)
                self._o = None
        except Exception:
            pass


class _ForwardSeeker:
    """The forward-only ReadSeeker of a StreamReader (reader.go:968-975): Seek forward is Skip, a backward Seek and — without an
    index — SeekEnd are refused with KC_S2D_UNSUPPORTED; ReadAt moves the cursor (reader.go:859)."""

    def __init__(self, rd, index):
        self._rd, self._index, self._pos = rd, index, 0

    def Seek(self, offset, whence=0):
        if whence == SeekStart:
            a = offset
        elif whence == SeekCurrent:
            a = self._pos + offset
        elif whence == SeekEnd:
            if self._index is None:
                raise S2DecodeError(3)  # ErrUnsupported (reader.go:941)
            a = self._index.TotalUncompressed + offset
        else:
            raise S2DecodeError(3)
        if a < 0:
            raise ValueError("seek before start of file")
        if a < self._pos:
            raise S2DecodeError(3)  # forward-only (reader.go:975)
        self._rd.Skip(a - self._pos)
        self._pos = a
        return a

    def Read(self, p):
        n = self._rd.Read(p)
        self._pos += n
        return n

    def ReadAt(self, p, off):
        if off < 0:
            raise ValueError("seek before start of file")
        self.Seek(off, SeekStart)
        return self.Read(p)

    def Skip(self, n):
        self._rd.Skip(n)
        self._pos += n

    def ReadByte(self):
        b = self._rd.ReadByte()
        self._pos += 1
        return b


def NewStreamReader(r, *opts, **kw):
    """s2.NewReader(r, opts...) (reader.go:31) for reading r as a stream: StreamReader."""
    return StreamReader(r, *opts, **kw)


def IndexStream(r):
    """s2.IndexStream (index.go:420): the index of a stream, built from its chunk headers on the host; it can be appended to the stream
    or kept beside it.  r: bytes or a reader.  Raises S2DecodeError with the class of the reference's error."""
    data = r.read() if hasattr(r, "read") else bytes(r)
    L = _lib.load()
    cap = 64 + 20 * (len(data) // (1 << 20) + 2)
    while True:
        out = C.create_string_buffer(cap)
        n, st = C.c_uint64(0), C.c_uint32(0)
        rc = L.kc_s2_index_stream(data, len(data), out, cap, C.byref(n), C.byref(st))
        if rc == _lib.KC_ERR_DST_TOO_SMALL:
            cap = int(n.value)
            continue
        if rc:
            raise _lib.KcError(rc, "kc_s2_index_stream")
        if st.value:
            raise S2DecodeError(st.value)
        return out.raw[:n.value]


class ErrCantSeek(ValueError):
    """s2.ErrCantSeek (reader.go): the reader cannot give random access; `Reason` says why."""

    def __init__(self, reason):
        self.Reason = reason
        super().__init__("s2: Can't seek because " + reason)


SeekStart, SeekCurrent, SeekEnd = 0, 1, 2


class ReadSeeker:
    """s2.ReadSeeker (reader.go:844-1041) over the whole input held in r: a cursor over Reader.ReadRanges.  Seek / Read / ReadAt / Skip /
    ReadByte; every read decodes on the device only the chunks that hold its range, starting from the index entry in front of it.
    random=False (or no index): forward-only — the input is walked from its start and a backward Seek is refused."""

    def __init__(self, r, *opts, random=True, index=None, device=0, stream=None):
        import numpy as np
        data = r.read() if hasattr(r, "read") else bytes(r)
        self._src = np.frombuffer(data, dtype=np.uint8)
        self._off = np.array([0, len(data)], dtype=np.uint64)
        self._rd = Reader(None, *opts, device=device, stream=stream)
        self._pos = 0
        self._index = None
        if index is not None and len(index) != 0:  # a supplied index wins (reader.go:866-873)
            self._index = Index()
            try:
                self._index.Load(index)
            except S2DecodeError as e:
                raise ErrCantSeek("loading index returned: " + str(e))
        else:
            ix = Index()
            try:
                ix.LoadStream(data)
                self._index = ix
            except S2DecodeError as e:
                if e.name != "KC_S2D_UNSUPPORTED":
                    raise ErrCantSeek("reading index returned: " + str(e))
                if random:
                    raise ErrCantSeek("input stream does not contain an index")

    def _read(self, off, n):
        """(bytes, status) of ReadAt(n bytes, off) without moving the cursor."""
        return self._rd.ReadRanges(self._src, self._off, [(0, off, n)], None if self._index is None else [self._index])[0]

    def Seek(self, offset, whence=SeekStart):
        """ReadSeeker.Seek (reader.go:923): returns the new absolute offset."""
        if whence == SeekStart:
            a = offset
        elif whence == SeekCurrent:
            a = self._pos + offset
        elif whence == SeekEnd:
            if self._index is None:
                raise S2DecodeError(3)  # ErrUnsupported (reader.go:941)
            a = self._index.TotalUncompressed + offset
        else:
            raise S2DecodeError(3)
        if a < 0:
            raise ValueError("seek before start of file")
        if self._index is None and a < self._pos:
            raise S2DecodeError(3)  # forward-only (reader.go:975)
        _, st = self._read(a, 0)  # the chunk that holds the target is decoded and checked, as Skip does
        if st:
            raise S2DecodeError(st)
        self._pos = a
        return a

    def ReadAt(self, p, off):
        """ReadSeeker.ReadAt (reader.go:1024): fills p from offset off; returns the bytes read.  A short read at the input's end returns
        what there is (the reference returns it with io.EOF); the cursor moves to the end of what was read (reader.go:859)."""
        if off < 0:
            raise ValueError("seek before start of file")
        if self._index is None and off < self._pos:
            raise S2DecodeError(3)
        b, st = self._read(off, len(p))
        if st and st != 5:
            raise S2DecodeError(st)
        p[:len(b)] = b
        self._pos = off + len(b)
        return len(b)

    def Read(self, p):
        """io.Reader: up to len(p) bytes from the cursor; 0 at the end of the input."""
        b, st = self._read(self._pos, len(p))
        if st and st != 5:
            raise S2DecodeError(st)
        p[:len(b)] = b
        self._pos += len(b)
        return len(b)

    def Skip(self, n):
        """Reader.Skip (reader.go:674): n decoded bytes forward; KC_S2D_UNEXPECTED_EOF when the input ends first."""
        if n < 0:
            raise ValueError("attempted negative skip")
        _, st = self._read(self._pos + n, 0)
        if st:
            raise S2DecodeError(st)
        self._pos += n

    def ReadByte(self):
        """Reader.ReadByte (reader.go:1044); raises EOFError at the end of the input."""
        p = bytearray(1)
        if self.Read(p) != 1:
            raise EOFError("EOF")
        return p[0]

    def Close(self):
        self._rd.Close()


def NewReadSeeker(r, *opts, random=True, index=None, **kw):
    """s2.NewReader(r, opts...).ReadSeeker(random, index) (reader.go:864-920) as one constructor: r holds the whole input.  A supplied
    index is used and none is read from the input; otherwise the index at the input's end is loaded.  Without one, random=True raises
    ErrCantSeek and random=False gives a forward-only seeker."""
    return ReadSeeker(r, *opts, random=random, index=index, **kw)


_decoders = {}


def Decode(dst, src, device=0):
    """s2.Decode(dst, src) (s2/decode.go:58): the decoded block (dst is not reused).  Raises S2DecodeError (KC_S2D_CORRUPT)."""
    import numpy as np
    rd = _decoders.get(device)
    if rd is None:
        rd = _decoders[device] = Reader(None, device=device)
    src = bytes(src)
    out = rd.DecodeBlocks(np.frombuffer(src, dtype=np.uint8), np.array([0, len(src)], dtype=np.uint64))[0]
    if isinstance(out, S2DecodeError):
        raise out
    return out
