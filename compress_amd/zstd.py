"""Host mirror of the reference's zstd encoder API for the EncodeAll hot path, and of its decoder's DecodeAll.

Names, argument meaning and error behaviour follow zstd/encoder.go, zstd/encoder_options.go, zstd/decoder.go and
zstd/decoder_options.go; the bytes come from the HIP engine behind include/kcgpu.h.

    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(zstd.SpeedFastest))
    frame = enc.EncodeAll(src, b"")                     # == reference EncodeAll(src, nil)
    frames, off = enc.EncodeUnits(buf, unit_off)        # N independent EncodeAll calls, one launch
    dec = zstd.NewReader(None)
    plain = dec.DecodeAll(frame, b"")                   # == reference DecodeAll(frame, nil)
    out, out_off, status = dec.DecodeUnits(frames, off) # N independent DecodeAll calls, one batch
    n = zstd.NewReader(open("big.zst", "rb")).WriteTo(w) # == reference NewReader(r) + WriteTo(w): a stream in bounded memory
"""
import contextlib
import ctypes as C
import os
import threading

from . import _lib
from ._lib import KcError

# zstd.EncoderLevel (encoder_options.go:163-179)
SpeedFastest, SpeedDefault, SpeedBetterCompression, SpeedBestCompression = 1, 2, 3, 4
MinWindowSize, MaxWindowSize = 1 << 10, 1 << 29


def EncoderLevelFromString(s):
    """encoder_options.go:181-198: case-insensitive name -> (ok, level)."""
    m = {"fastest": SpeedFastest, "default": SpeedDefault, "better": SpeedBetterCompression, "best": SpeedBestCompression}
    lvl = m.get(s.lower())
    return (lvl is not None), (lvl if lvl is not None else SpeedDefault)


def EncoderLevelFromZstd(level):
    """encoder_options.go:200-218."""
    if level < 3:
        return SpeedFastest
    if level < 6:
        return SpeedDefault
    if level < 10:
        return SpeedBetterCompression
    return SpeedBestCompression


# ---- EOption constructors: each returns a callable applied in order to the options struct ----
def _opt(name, *args):
    def apply(o):
        L = _lib.load()
        st = getattr(L, "kc_zstd_opts_" + name)(C.byref(o), *args)
        if st != 0:
            raise ValueError("zstd option %s%r rejected" % (name, args))
    return apply


def WithEncoderLevel(l):
    return _opt("level", int(l))


def WithWindowSize(n):
    return _opt("window", int(n))


def WithEncoderCRC(b):
    return _opt("crc", int(bool(b)))


def WithZeroFrames(b):
    return _opt("zero_frames", int(bool(b)))


def WithNoEntropyCompression(b):
    return _opt("no_entropy", int(bool(b)))


def WithAllLitEntropyCompression(b):
    return _opt("all_lit_entropy", int(bool(b)))


def WithSingleSegment(b):
    return _opt("single_segment", int(bool(b)))


def WithEncoderDictRaw(id, content):
    content = bytes(content)

    def apply(o):
        L = _lib.load()
        buf = C.create_string_buffer(content, len(content))
        o._dict_keep = buf
        if L.kc_zstd_opts_dict_raw(C.byref(o), id, C.cast(buf, C.c_void_p), len(content)) != 0:
            raise ValueError("dictionary rejected")
    return apply


def WithEncoderDict(dict):
    """zstd.WithEncoderDict (zstd/encoder_options.go:382-391): a dictionary in the `zstd --train` format."""
    blob = bytes(dict)

    def apply(o):
        L = _lib.load()
        buf = C.create_string_buffer(blob, len(blob))
        o._dict_keep = buf  # o.dict points into the blob
        if L.kc_zstd_opts_dict(C.byref(o), C.cast(buf, C.c_void_p), len(blob)) != 0:
            raise ValueError("dictionary rejected (loadDict error)")
    return apply


SKIPPABLE_FRAME_HEADER = 8  # zstd/frameenc.go: skippableFrameHeader = 4 + 4


def calc_skippable_frame(written, want_multiple):
    """calcSkippableFrame (zstd/frameenc.go:100-116): bytes of skippable frame that bring `written` to a multiple of
    `want_multiple`; a frame needs its 8-byte header, so a remainder below that is padded by one more multiple."""
    if want_multiple <= 0:
        raise ValueError("wantMultiple <= 0")
    if written < 0:
        raise ValueError("written < 0")
    left_over = written % want_multiple
    if left_over == 0:
        return 0
    to_add = want_multiple - left_over
    while to_add < SKIPPABLE_FRAME_HEADER:
        to_add += want_multiple
    return to_add


def skippable_frame(total, rand=os.urandom):
    """skippableFrame (zstd/frameenc.go:118-137): a skippable frame of `total` bytes in all — magic 0x184D2A50, the 32-bit size of what
    follows, and that many bytes from `rand` (the reference reads crypto/rand.Reader: the padding is not reproducible by design)."""
    if total == 0:
        return b""
    if total < SKIPPABLE_FRAME_HEADER:
        raise ValueError("requested skippable frame (%d) < 8" % total)
    if total > 0xFFFFFFFF:
        raise ValueError("requested skippable frame (%d) > max uint32" % total)
    f = total - SKIPPABLE_FRAME_HEADER
    return bytes([0x50, 0x2A, 0x4D, 0x18]) + int(f).to_bytes(4, "little") + bytes(rand(f))


def pad_frames(out, out_off, pad, rand=os.urandom):
    """Every frame of a batch followed by the skippable frame that WithEncoderPadding(pad) appends to it — per frame what EncodeAll
    does with an empty dst (zstd/encoder.go:829-837).  A zero-length frame (empty input without WithZeroFrames) stays empty:
    EncodeAll returns before the padding there (zstd/encoder.go:732-752).  Returns (bytes, offsets)."""
    import numpy as np
    n = len(out_off) - 1
    parts, offs, pos = [], [0], 0
    for i in range(n):
        fr = bytes(out[int(out_off[i]):int(out_off[i + 1])])
        if fr:
            fr += skippable_frame(calc_skippable_frame(len(fr), pad), rand)
        parts.append(fr)
        pos += len(fr)
        offs.append(pos)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.asarray(offs, dtype=np.uint64)


def WithEncoderPadding(n):
    """zstd.WithEncoderPadding (encoder_options.go:142-158): the output of EncodeAll / of a stream is padded to a multiple of n with a
    skippable frame of random bytes.  Host-side: the device frames are the unpadded ones."""
    n = int(n)
    if n <= 0:
        raise ValueError("padding must be at least 1")
    if n > 1 << 30:
        raise ValueError("padding must less than 1GB (1<<30 bytes) ")

    def apply(o):
        pass
    apply._kc_pad = 0 if n == 1 else n  # "No need to waste our time."
    return apply


def WithEncoderDictDelete():
    """zstd.WithEncoderDictDelete (encoder_options.go:408-415): no dictionary from here on."""
    def apply(o):  # every field a dictionary sets, back to kc_zstd_opts_default's
        o.dict = None
        o.dict_len = 0
        o.dict_id = 0
        o.dict_offsets[0], o.dict_offsets[1], o.dict_offsets[2] = 1, 4, 8  # blockenc.go:78
        o.dict_huf_len = 0
        o.dict_huf_log = 0
    apply._kc_dict_delete = True
    return apply


def WithMatchPath(path):
    """Not a reference option: which kernel family serves SpeedFastest ('auto' by units in flight, 'hbm', 'lds';
    KC_OPT_MATCH_PATH in include/kcgpu.h).  The bytes are the reference's either way."""
    def apply(o):
        pass
    apply._kc_path = path
    return apply


def WithEncoderConcurrency(n):
    """zstd.WithEncoderConcurrency (zstd/encoder_options.go:76-87).  The device path is batch-parallel; the bytes that depend on
    it are those of WithConcurrentBlocks, which the reference switches off when the concurrency is 1 (zstd/encoder.go:81), and
    those of dictionary streams: with 1 the reference's synchronous nextBlock form drops the dictionary's literal table before
    the first block (zstd/encoder.go:371)."""
    if n <= 0:
        raise ValueError("concurrency must be at least 1")

    def apply(o):
        o.concurrent = int(n)
    apply._kc_concurrency = int(n)
    return apply


def WithConcurrentBlocks(b):
    """zstd.WithConcurrentBlocks (zstd/encoder_options.go:340-353): the stream written through Write / ReadFrom / Flush / Close is
    cut into jobs of max(4 * window, 512 KiB) bytes, each encoded with the tail of the previous job as its history
    (zstd/enc_jobs.go) — independent units for the device (kc_zstd_encode_jobs).  As in the reference it has no effect with a
    dictionary or with WithEncoderConcurrency(1)."""
    def apply(o):
        pass
    apply._kc_conc_blocks = bool(b)
    return apply


def WithLowerEncoderMem(b):
    return lambda o: setattr(o, "low_mem", int(bool(b)))


class Encoder:
    """zstd.Encoder: EncodeAll and its batched forms, plus the streaming surface Write / ReadFrom / Flush / Close / Reset
    (zstd/encoder.go:140-649).  A stream is buffered on the host and encoded on Close as ONE device unit whose bytes equal the
    reference's for the same Write / Flush sequence, dictionaries included; streams of more than 1 GiB are not served
    (the caller falls back to the reference).  EncodeStreams / EncodeStreamsDevice batch many streams per launch."""

    def __init__(self, *opts, device=0, stream=None, w=None, path=None):
        """path: None / 'auto' (by units in flight), 'hbm' or 'lds' — the kernel family of the SpeedFastest match finder
        (KC_OPT_MATCH_PATH, include/kcgpu.h); both give the reference's bytes."""
        self._path = path
        self._w = w
        self._buf = bytearray()
        self._cuts = []
        self._closed = False
        L = _lib.load()
        self.o = _lib.ZstdOpts()
        L.kc_zstd_opts_default(C.byref(self.o))
        self._conc_blocks, self._concurrency = False, os.cpu_count() or 1  # o.concurrent defaults to GOMAXPROCS (encoder_options.go:38)
        self._pad = 0
        for op in opts:
            if hasattr(op, "_kc_pad"):
                self._pad = op._kc_pad
                continue
            if hasattr(op, "_kc_path"):
                self._path = op._kc_path
                continue
            if hasattr(op, "_kc_conc_blocks"):
                self._conc_blocks = op._kc_conc_blocks
                continue
            if hasattr(op, "_kc_concurrency"):
                self._concurrency = op._kc_concurrency
                op(self.o)
                continue
            op(self.o)
        self._device, self._stream = device, stream
        self._ctx = None
        self._lock = threading.Lock()
        self._primary_busy = False
        self._spare = []  # contexts of concurrent EncodeAll / EncodeUnits callers (see _held)

    # -- reference API --
    def MaxEncodedSize(self, size):
        m = int(_lib.load().kc_zstd_max_encoded_size(C.byref(self.o), int(size)))
        if self._pad > 1:  # zstd/encoder.go:867-871
            m += calc_skippable_frame(m, self._pad)
        return m

    def EncodeAll(self, src, dst=b""):
        """Encode all of src as one frame and append to dst (zstd/encoder.go:722)."""
        import numpy as np
        src = bytes(src)
        off = np.array([0, len(src)], dtype=np.uint64)
        out, _ = self._encode_units_unpadded(np.frombuffer(src, dtype=np.uint8), off)
        res = bytes(dst) + out.tobytes()
        if self._pad > 0 and len(out):  # the TOTAL size becomes a multiple (dst included: encoder_options.go:140, encoder.go:829-837)
            res += skippable_frame(calc_skippable_frame(len(res), self._pad))
        return res

    # -- batched form: what the cgo shim calls --
    def _new_ctx(self):
        c = _lib.Context(self._device, self._stream)
        if self._path is not None:
            c.set_path(self._path)
        return c

    def ctx(self):
        """The encoder's own context (options set on it, timings, the streaming / device-resident / asynchronous calls)."""
        if self._ctx is None:
            self._ctx = self._new_ctx()
        return self._ctx

    @contextlib.contextmanager
    def _held(self):
        """EncodeAll "can be called concurrently" on one Encoder (zstd/encoder.go:717): every call takes an encoder state from
        e.encoders and puts it back (encoder.go:90-99, 722-729).  Here the state is a kc_ctx: a lone caller always gets the
        encoder's own context; a caller that finds it taken gets a spare one (created on demand, at most WithEncoderConcurrency
        kept), with the kernel-family choice of the constructor — options set on ctx() afterwards stay with ctx()."""
        with self._lock:
            if not self._primary_busy:
                self._primary_busy = True
                c = self.ctx()
            else:
                c = self._spare.pop() if self._spare else None
        if c is None:
            c = self._new_ctx()
        try:
            yield c
        finally:
            with self._lock:
                if c is self._ctx:
                    self._primary_busy = False
                elif self._ctx is not None and len(self._spare) < max(1, self._concurrency):
                    self._spare.append(c)
                else:
                    c.close()

    def EncodeUnits(self, src, unit_off):
        """src: numpy uint8 (host); unit_off: uint64[n+1].  Returns (numpy uint8 frames, uint64[n+1] offsets).  With
        WithEncoderPadding every frame is followed by its skippable frame (N x EncodeAll(unit, nil))."""
        out, out_off = self._encode_units_unpadded(src, unit_off)
        if self._pad > 0:
            return pad_frames(out, out_off, self._pad)
        return out, out_off

    def _encode_units_unpadded(self, src, unit_off):
        import numpy as np
        src = np.ascontiguousarray(src, dtype=np.uint8)
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        cap = sum(((self.MaxEncodedSize(int(unit_off[i + 1] - unit_off[i])) + 15) & ~15) for i in range(n)) + 64
        dst = np.empty(cap, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        with self._held() as ctx:
            ctx.check(ctx.L.kc_zstd_encode_units(ctx.h, C.byref(self.o), src.ctypes.data, unit_off.ctypes.data, n,
                                                 dst.ctypes.data, cap, out_off.ctypes.data))
        return dst[:int(out_off[n])], out_off

    def EncodeUnitsSubmit(self, src, unit_off, dst=None):
        """Asynchronous EncodeUnits (kc_zstd_encode_units_submit): returns at once; Wait() returns what EncodeUnits returns.
        dst: optional pre-allocated (pre-faulted) uint8 array of at least the summed MaxEncodedSize."""
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        cap = sum(((self.MaxEncodedSize(int(unit_off[i + 1] - unit_off[i])) + 15) & ~15) for i in range(n)) + 64
        if dst is None:
            dst = np.empty(cap, dtype=np.uint8)
        assert dst.dtype == np.uint8 and dst.size >= cap
        out_off = np.zeros(n + 1, dtype=np.uint64)
        ctx.check(ctx.L.kc_zstd_encode_units_submit(ctx.h, C.byref(self.o), src.ctypes.data, unit_off.ctypes.data, n,
                                                    dst.ctypes.data, dst.size, out_off.ctypes.data))
        self._job = (src, unit_off, dst, out_off, n)  # kept alive until Wait

    def Wait(self):
        src, unit_off, dst, out_off, n = self._job
        self._job = None
        ctx = self.ctx()
        ctx.check(ctx.L.kc_wait(ctx.h))
        return dst[:int(out_off[n])], out_off

    def EncodeUnitsDevice(self, d_src_ptr, unit_off, d_dst_ptr, dst_cap):
        """Device-resident form (pointers are ints).  Returns uint64[n+1] offsets (host numpy)."""
        import numpy as np
        ctx = self.ctx()
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        ctx.check(ctx.L.kc_zstd_encode_units_dev(ctx.h, C.byref(self.o), d_src_ptr, unit_off.ctypes.data, n, d_dst_ptr,
                                                 int(dst_cap), out_off.ctypes.data))
        return out_off

    # -- streaming surface (encoder.go:140-253, 531-649) --
    def Reset(self, w):
        self._w = w
        self._buf = bytearray()
        self._cuts = []
        self._closed = False

    def Write(self, p):
        if self._closed:
            raise IOError("zstd: encoder closed")  # ErrEncoderClosed
        self._buf += bytes(p)
        return len(p)

    def ReadFrom(self, r):
        self._cuts.append(len(self._buf))  # ReadFrom first ends the block being filled (encoder.go:482-486)
        n = 0
        while True:
            b = r.read(1 << 20)
            if not b:
                return n
            n += self.Write(b)

    def Flush(self):
        """Encoder.Flush (encoder.go:547): ends the block being filled.  The bytes reach w on Close (the device path encodes the
        whole stream in one call); they are the bytes the reference's writer receives, block boundaries included."""
        if self._closed:
            return
        self._cuts.append(len(self._buf))

    def _finish_stream(self):
        """The frame the reference writes for Write(everything) + Close() goes to w."""
        if self._closed or self._w is None:
            self._closed = True
            return
        import numpy as np
        data = bytes(self._buf)
        cuts, self._cuts = self._cuts, []
        self._buf = bytearray()
        self._closed = True
        if self._conc_blocks and self._concurrency > 1 and not self.o.dict_len:  # zstd/encoder.go:81: else the option is off
            frame = bytes(self.EncodeJobs(data, cuts))
        else:
            out, _ = self.EncodeStreams(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.uint64),
                                        flush_at=[cuts] if cuts else None)
            frame = out.tobytes()
        if self._pad > 0:  # Close: padding from the bytes written in this stream (zstd/encoder.go:637-645, 700-708)
            frame += skippable_frame(calc_skippable_frame(len(frame), self._pad))
        self._w.write(frame)

    def JobSize(self):
        return int(_lib.load().kc_zstd_job_size(C.byref(self.o)))

    def OverlapSize(self):
        return int(_lib.load().kc_zstd_overlap_size(C.byref(self.o)))

    def EncodeJobs(self, src, flush_at=()):
        """ONE stream with WithConcurrentBlocks(true): NewWriter(w, opts, WithConcurrentBlocks(true)); Write(src) with Flush at
        flush_at; Close() (kc_zstd_encode_jobs: the jobs of zstd/enc_jobs.go are the device's units).  Returns bytes."""
        import numpy as np
        ctx = self.ctx()
        src = np.frombuffer(bytes(src), dtype=np.uint8) if not isinstance(src, np.ndarray) else np.ascontiguousarray(src, dtype=np.uint8)
        n = len(src)
        cuts = np.ascontiguousarray(sorted(int(x) for x in flush_at), dtype=np.uint64)
        js, ov = self.JobSize(), self.OverlapSize()
        njobs = n // js + len(cuts) + 2
        cap = njobs * (((self.MaxEncodedSize(js + ov) - js - ov) + 31) & ~15) + n + njobs * ov + 4096
        dst = np.empty(cap, dtype=np.uint8)
        out_len = C.c_uint64(0)
        sp = src.ctypes.data if n else None
        ctx.check(ctx.L.kc_zstd_encode_jobs(ctx.h, C.byref(self.o), sp, n, cuts.ctypes.data if len(cuts) else None, len(cuts),
                                            dst.ctypes.data, cap, C.byref(out_len)))
        return dst[:out_len.value].tobytes()

    def EncodeStreams(self, src, unit_off, flush_at=None):
        """Like EncodeUnits, but every unit is a stream: NewWriter(w).Write(unit) ... Close().  flush_at: per stream, the byte
        counts at which Flush was called (kc_zstd_encode_streams_cuts)."""
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        ncut = [len(flush_at[i]) if flush_at is not None else 0 for i in range(n)]
        cap = sum(((self.MaxEncodedSize(int(unit_off[i + 1] - unit_off[i])) + (3 * ncut[i] + 3 if flush_at is not None else 0) + 15) & ~15)
                  for i in range(n)) + 64
        dst = np.empty(cap, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        if flush_at is None:
            ctx.check(ctx.L.kc_zstd_encode_streams(ctx.h, C.byref(self.o), src.ctypes.data, unit_off.ctypes.data, n,
                                                   dst.ctypes.data, cap, out_off.ctypes.data))
        else:
            cut_off = np.zeros(n + 1, dtype=np.uint64)
            cut_off[1:] = np.cumsum(ncut)
            cuts = np.array([int(x) for f in flush_at for x in sorted(f)] + [0], dtype=np.uint64)
            ctx.check(ctx.L.kc_zstd_encode_streams_cuts(ctx.h, C.byref(self.o), src.ctypes.data, unit_off.ctypes.data, n,
                                                        cut_off.ctypes.data, cuts.ctypes.data, dst.ctypes.data, cap, out_off.ctypes.data))
        return dst[:int(out_off[n])], out_off

    def EncodeStreamsDevice(self, d_src_ptr, unit_off, d_dst_ptr, dst_cap):
        import numpy as np
        ctx = self.ctx()
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        ctx.check(ctx.L.kc_zstd_encode_streams_dev(ctx.h, C.byref(self.o), d_src_ptr, unit_off.ctypes.data, n, d_dst_ptr,
                                                   int(dst_cap), out_off.ctypes.data))
        return out_off

    def DecodeUnitsDevice(self, d_enc_ptr, enc_off, d_dst_ptr, dst_off, dict_content=None):
        """Verifier: decode one frame per unit on the device; returns uint32[n] status (0 = content and checksum match).
        dict_content: the (raw) dictionary content the frames were written with, if any."""
        import numpy as np
        ctx = self.ctx()
        enc_off = np.ascontiguousarray(enc_off, dtype=np.uint64)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.uint64)
        n = len(enc_off) - 1
        status = np.zeros(max(n, 1), dtype=np.uint32)
        dc = bytes(dict_content) if dict_content else None
        ctx.check(ctx.L.kc_zstd_decode_units_dict_dev(ctx.h, d_enc_ptr, enc_off.ctypes.data, n, d_dst_ptr, dst_off.ctypes.data, status.ctypes.data,
                                                      dc, len(dc) if dc else 0))
        return status[:n]

    def EncodeUnitsDeviceBegin(self, d_src_ptr, unit_off, d_dst_ptr, dst_cap):
        """First half of EncodeUnitsDevice (one device batch): enqueue up to and including the match finder, no wait."""
        import numpy as np
        ctx = self.ctx()
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        self._pending_n = len(unit_off) - 1
        ctx.check(ctx.L.kc_zstd_encode_units_dev_begin(ctx.h, C.byref(self.o), d_src_ptr, unit_off.ctypes.data, self._pending_n,
                                                       d_dst_ptr, int(dst_cap)))

    def EncodeUnitsDeviceEnd(self, d_dst_ptr=None, dst_cap=0):
        """Second half: entropy stage, wait, offsets (uint64[n+1], host numpy).  d_dst_ptr: the frames go THERE instead of to the
        place given to Begin (kc_zstd_encode_units_dev_end_at: the parts of one batch run as several launches, each part's frames
        right behind the previous part's); the offsets are relative to it."""
        import numpy as np
        ctx = self.ctx()
        out_off = np.zeros(self._pending_n + 1, dtype=np.uint64)
        if d_dst_ptr is None:
            ctx.check(ctx.L.kc_zstd_encode_units_dev_end(ctx.h, out_off.ctypes.data))
        else:
            ctx.check(ctx.L.kc_zstd_encode_units_dev_end_at(ctx.h, d_dst_ptr, int(dst_cap), out_off.ctypes.data))
        return out_off

    def ChainAfter(self, other):
        """Pipelining two encoders: this one's match finder waits for `other`'s last one (see include/kcgpu.h)."""
        self.ctx().L.kc_ctx_chain_after(self.ctx().h, other.ctx().h if other is not None else None)

    def DebugParseDevice(self, d_src_ptr, unit_off):
        """Match-finder intermediates for parity tests: list over blocks of (seqs[n,3] u32, extra_lits)."""
        import numpy as np
        ctx = self.ctx()
        unit_off = np.ascontiguousarray(unit_off, dtype=np.uint64)
        n = len(unit_off) - 1
        total = int(unit_off[n] - unit_off[0])
        bs = self.o.block_size
        blk_cap = total // bs + n + 2
        seqs = np.empty((total // 4 + 16, 3), dtype=np.uint32)
        first = np.zeros(blk_cap + 1, dtype=np.uint64)
        extra = np.zeros(blk_cap, dtype=np.uint32)
        flags = np.zeros(blk_cap, dtype=np.uint32)
        nb = C.c_uint32()
        ctx.check(ctx.L.kc_zstd_debug_parse_dev(ctx.h, C.byref(self.o), d_src_ptr, unit_off.ctypes.data, n, seqs.ctypes.data,
                                                len(seqs), first.ctypes.data, extra.ctypes.data, flags.ctypes.data, blk_cap,
                                                C.byref(nb)))
        self.last_block_flags = flags[:nb.value].copy()
        return [(seqs[int(first[b]):int(first[b + 1])].copy(), int(extra[b])) for b in range(nb.value)]

    def Close(self):
        """Encoder.Close (encoder.go:589): finish the stream, if one was written to a writer; the device context is released
        and re-created on the next use (the encoder stays usable after Reset, like the reference's)."""
        self._finish_stream()
        with self._lock:
            spare, self._spare = self._spare, []
            c, self._ctx = self._ctx, None
        for x in spare:
            x.close()
        if c is not None:
            c.close()


def NewWriter(w, *opts, **kw):
    """zstd.NewWriter(w, opts...) (encoder.go:71).  w (may be None for block-API use) receives the stream on Close."""
    return Encoder(*opts, w=w, **kw)


# ---- zstd.Decoder: DecodeAll over batches on the device (zstd/decoder.go:319-410, decoder_options.go) and the stream reader
# (NewReader(r) / Read / WriteTo, decoder.go:88-312) ----
class DecodeError(ValueError):
    """DecodeAll refused its input.  `name` is the class of the reference's error: KC_ZD_MAGIC (ErrMagicMismatch), KC_ZD_EOF
    (unexpected EOF), KC_ZD_UNKNOWN_DICT, KC_ZD_WINDOW_EXCEEDED, KC_ZD_SIZE_EXCEEDED, KC_ZD_CRC, KC_ZD_CORRUPT (everything else)."""

    def __init__(self, status):
        self.status = int(status)
        self.name = _lib.ZD_NAMES.get(self.status, str(self.status))
        super().__init__("zstd: DecodeAll: %s" % self.name)


class ErrDecoderClosed(ValueError):
    """zstd.ErrDecoderClosed: Read / WriteTo / Reset after Close."""

    def __init__(self):
        super().__init__("zstd: decoder used after Close")


class ErrDecoderNilInput(NotImplementedError):
    """zstd.ErrDecoderNilInput: Read / WriteTo on a decoder that has no stream (NewReader(None), Reset(None)): only DecodeAll and
    its batched forms are served then."""

    def __init__(self):
        super().__init__("zstd: nil input provided as reader: use DecodeAll / DecodeUnits, or Reset(r) with a stream")


class StreamBuffer:
    """The buffering between an io reader and a stream decoder given as three functions: new() -> handle, feed(handle, src, n, eof,
    dst, dst_cap, consumed*, produced*, status*) -> kc_status (kc_zstd_dstream_feed's signature behind the handle) and free(handle).
    It pulls r.read(batch_bytes), keeps the tail the decoder has not consumed, and hands the decoded bytes out in slices."""

    def __init__(self, new, feed, free, r, batch_bytes=32 << 20, min_cap=128 << 10, what="zstd stream decoder"):
        self._feed, self._free = feed, free
        self._what = what   # names the decoder in error texts
        self._h = new()
        if not self._h:
            raise MemoryError("%s: new() failed" % what)
        self._r = r
        self._batch = max(int(batch_bytes), 1)
        self._in, self._pos, self._eof = b"", 0, False
        self._cap = max(self._batch, int(min_cap))  # (zstd: no block's bound is above 128 KiB; another format names its own)
        self._out = C.create_string_buffer(self._cap)
        self._lo = self._hi = 0
        self.status = 0     # the class of the stream's error, once everything in front of it has been decoded
        self.done = False   # the stream has ended cleanly

    def close(self):
        h, self._h = self._h, None
        if h:
            self._free(h)

    @property
    def handle(self):
        """The decoder's handle (what new() returned), for calls beside feed."""
        return self._h

    def buffered(self):
        """Decoded bytes held and not yet handed out."""
        return self._hi - self._lo

    def drop(self, n):
        """Discards up to n of the buffered bytes; returns how many."""
        k = min(int(n), self._hi - self._lo)
        self._lo += k
        return k

    def restart(self, r):
        """The same handle and buffer for a new input r: the caller has reset the decoder behind the handle."""
        self._r = r
        self._in, self._pos, self._eof = b"", 0, False
        self._lo = self._hi = 0
        self.status, self.done = 0, False

    def fill(self):
        """Decodes until there are bytes to hand out (at once when some are buffered); False at the stream's end or at its error."""
        return self._more()

    def step(self):
        """One turn of the loop behind read_into, for a caller that drives the decoder without taking bytes (a skip)."""
        self._step()

    def _step(self):
        """One call of the decoder on what is held; when it neither takes nor gives anything, more input from r (or the end)."""
        consumed, produced, status = C.c_uint64(), C.c_uint64(), C.c_uint32()
        n = len(self._in) - self._pos
        src = C.cast(C.c_char_p(self._in), C.c_void_p).value + self._pos if n else None
        rc = self._feed(self._h, src, n, int(self._eof), C.addressof(self._out), self._cap, C.byref(consumed), C.byref(produced), C.byref(status))
        if rc != 0:
            raise _lib.KcError(rc, "%s: feed" % self._what)
        self._pos += consumed.value
        self._lo, self._hi = 0, produced.value
        self.status = status.value
        if consumed.value or produced.value or status.value:
            return
        if self._eof:  # nothing left and nothing asked for: the clean end
            self.done = True
            return
        chunk = self._r.read(self._batch)
        if chunk:
            self._in = self._in[self._pos:] + bytes(chunk)
            self._pos = 0
        else:
            self._eof = True

    def _more(self):
        """Decodes until there are bytes to hand out; False at the stream's end or at its error."""
        while self._lo == self._hi:
            if self.status or self.done:
                return False
            self._step()
        return True

    def read_into(self, p):
        """Fills the writable buffer p; the number of bytes (less than len(p) only at the stream's end or in front of its error)."""
        mv = memoryview(p).cast("B")
        n = 0
        while n < len(mv) and self._more():
            k = min(len(mv) - n, self._hi - self._lo)
            mv[n:n + k] = memoryview(self._out)[self._lo:self._lo + k].cast("B")
            self._lo += k
            n += k
        return n

    def write_to(self, w):
        n = 0
        while self._more():
            k = w.write(memoryview(self._out)[self._lo:self._hi])
            k = self._hi - self._lo if k is None else k
            if k != self._hi - self._lo:
                raise IOError("short write")
            n += k
            self._lo = self._hi
        return n


def _dopt(name, *args):
    def apply(d):
        if getattr(_lib.load(), "kc_zstd_dopts_" + name)(d._o, *args) != 0:
            raise ValueError("zstd decoder option %s rejected" % name)
    return apply


def WithDecoderMaxMemory(n):
    """zstd.WithDecoderMaxMemory (decoder_options.go:90-101): the most one DecodeAll may return (default 64 GiB)."""
    return _dopt("max_memory", int(n))


def WithDecoderMaxWindow(size):
    """zstd.WithDecoderMaxWindow (decoder_options.go:150-161; default 512 MiB)."""
    return _dopt("max_window", int(size))


def IgnoreChecksum(b):
    """zstd.IgnoreChecksum: the content checksum of a frame is skipped, not checked."""
    return _dopt("ignore_checksum", int(bool(b)))


def WithDecoderDicts(*dicts):
    """zstd.WithDecoderDicts (decoder_options.go:112-126): dictionaries in the `zstd --train` format; a frame's dictionary id picks one."""
    blobs = [bytes(b) for b in dicts]

    def apply(d):
        L = _lib.load()
        for b in blobs:
            if L.kc_zstd_dopts_dict(d._o, b, len(b)) != 0:
                raise ValueError("dictionary rejected (loadDict error)")
    return apply


def WithDecoderDictRaw(id, content):
    """zstd.WithDecoderDictRaw (decoder_options.go:131-142): arbitrary content as the dictionary with this id."""
    content = bytes(content)
    return _dopt("dict_raw", int(id), content, len(content))


def WithDecoderConcurrency(n):
    """zstd.WithDecoderConcurrency (decoder_options.go:68-83).  The device path is batch-parallel: no effect on bytes."""
    if n < 0:
        raise ValueError("concurrency must be at least 0")
    return lambda d: None


def WithDecoderLowmem(b):
    """zstd.WithDecoderLowmem: no effect on bytes."""
    return lambda d: None


class Decoder:
    """zstd.Decoder for the stateless form: DecodeAll, and its batched forms DecodeUnits (host buffers) and DecodeAllDevice
    (device-resident).  An input is what DecodeAll takes: any concatenation of frames and skippable frames; no decoded size is
    needed.  With a reader (NewReader(r), Reset(r)) it is the streaming decoder: Read / WriteTo decode r in bounded memory
    (kc_zstd_dstream_feed: the frame's blocks on many waves, one launch after the other)."""

    def __init__(self, *opts, device=0, stream=None, batch_bytes=32 << 20):
        L = _lib.load()
        self._o = C.c_void_p(L.kc_zstd_dopts_default())
        if not self._o:
            raise MemoryError("kc_zstd_dopts_default")
        for op in opts:
            op(self)
        self._device, self._stream = device, stream
        self._ctx = None
        self._batch_bytes = batch_bytes
        self._sb = None       # the stream in progress (StreamBuffer)
        self._closed = False

    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device, self._stream)
        return self._ctx

    def DecodeAll(self, input, dst=b""):
        """Decode all of `input` and append to dst (zstd/decoder.go:319).  Raises DecodeError with the class of the reference's error."""
        import numpy as np
        input = bytes(input)
        out, out_off, status = self.DecodeUnits(np.frombuffer(input, dtype=np.uint8), np.array([0, len(input)], dtype=np.uint64))
        if status[0]:
            raise DecodeError(status[0])
        return bytes(dst) + out.tobytes()

    def DecodeBounds(self, src, in_off):
        """The plan alone (kc_zstd_decode_all_bound): per input the decoded size — exact when every frame carries its content size,
        else an upper bound from the block headers — and the first header-level error.  Returns (uint64[n], uint32[n])."""
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        bound = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        ctx.check(ctx.L.kc_zstd_decode_all_bound(ctx.h, self._o, src.ctypes.data, in_off.ctypes.data, n, bound.ctypes.data, status.ctypes.data))
        return bound[:n], status[:n]

    def DecodeUnits(self, src, in_off):
        """N x DecodeAll(input_i, nil) in one batch.  src: numpy uint8 (host), in_off: uint64[n+1].  Returns (numpy uint8 output,
        uint64[n+1] offsets, uint32[n] status); an input that fails has a non-zero status (_lib.ZD_NAMES) and an empty range."""
        import numpy as np
        ctx = self.ctx()
        src = np.ascontiguousarray(src, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        bound, st0 = self.DecodeBounds(src, in_off)
        cap = int(sum(int(b) for b, s in zip(bound, st0) if s == 0))
        dst = np.empty(cap + 64, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        ctx.check(ctx.L.kc_zstd_decode_all(ctx.h, self._o, src.ctypes.data, in_off.ctypes.data, n, dst.ctypes.data, cap, out_off.ctypes.data,
                                           status.ctypes.data))
        return dst[:int(out_off[n])], out_off, status[:n]

    def DecodeBoundsDevice(self, d_src_ptr, in_off):
        """DecodeBounds over device-resident inputs (kc_zstd_decode_all_bound_dev): what d_dst must hold."""
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        bound = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        ctx.check(ctx.L.kc_zstd_decode_all_bound_dev(ctx.h, self._o, d_src_ptr, in_off.ctypes.data, n, bound.ctypes.data, status.ctypes.data))
        return bound[:n], status[:n]

    def DecodeAllDevice(self, d_src_ptr, in_off, d_dst_ptr, dst_cap):
        """Device-resident form (pointers are ints): returns (uint64[n+1] offsets, uint32[n] status), host numpy.  Raises KcError
        KC_ERR_DST_TOO_SMALL when the decoded inputs do not fit dst_cap (nothing is written past it)."""
        import numpy as np
        ctx = self.ctx()
        in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = len(in_off) - 1
        out_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        ctx.check(ctx.L.kc_zstd_decode_all_dev(ctx.h, self._o, d_src_ptr, in_off.ctypes.data, n, d_dst_ptr, int(dst_cap), out_off.ctypes.data,
                                               status.ctypes.data))
        return out_off, status[:n]

    def Reset(self, r):
        """Decoder.Reset (decoder.go:166-234): the next stream to read; None releases the current one (Read then raises
        ErrDecoderNilInput, DecodeAll goes on working)."""
        if self._closed:
            raise ErrDecoderClosed()
        self._drop_stream()
        if r is None:
            return
        self._sb = self._open(r)

    def _open(self, r):
        """The stream's buffering on the library's three functions (the CPU tests put the wave emulator's in their place)."""
        ctx = self.ctx()
        L = ctx.L
        return StreamBuffer(lambda: L.kc_zstd_dstream_new(ctx.h, self._o), L.kc_zstd_dstream_feed, L.kc_zstd_dstream_free, r, self._batch_bytes)

    def _drop_stream(self):
        sb, self._sb = self._sb, None
        if sb is not None:
            sb.close()

    def _stream_buffer(self):
        if self._closed:
            raise ErrDecoderClosed()
        if self._sb is None:
            raise ErrDecoderNilInput()
        return self._sb

    def Read(self, p):
        """Decoder.Read (decoder.go:120-159): fills p from the decoded stream and returns the count; 0 at the stream's clean end.
        Raises DecodeError with the class of the stream's error once every byte in front of it has been returned."""
        sb = self._stream_buffer()
        n = sb.read_into(p)
        if n == 0 and len(p) and sb.status:
            raise DecodeError(sb.status)
        return n

    def WriteTo(self, w):
        """Decoder.WriteTo (decoder.go:284-312): writes the rest of the decoded stream to w and returns the byte count.  An error
        of the stream is raised after the bytes in front of it were written (DecodeError.written = their count)."""
        sb = self._stream_buffer()
        n = sb.write_to(w)
        if sb.status:
            e = DecodeError(sb.status)
            e.written = n
            raise e
        return n

    def IOReadCloser(self):
        """Decoder.IOReadCloser (decoder.go:605-632): read / readinto / write_to / close on the same decoder."""
        return _ReadCloser(self)

    def Close(self):
        """Decoder.Close (decoder.go:579-603): the stream and the device context are released; Read / WriteTo / Reset then raise
        ErrDecoderClosed.  (DecodeAll and its batched forms keep working: their context comes back with the next use.)"""
        self._closed = True
        self._drop_stream()
        c, self._ctx = self._ctx, None
        if c is not None:
            c.close()

    def __del__(self):
        try:
            self._drop_stream()
            self.Close()
            if getattr(self, "_o", None):
                _lib.load().kc_zstd_dopts_free(self._o)
                self._o = None
        except Exception:
            pass


class _ReadCloser:
    def __init__(self, d):
        self.d = d

    def read(self, n=-1):
        if n is None or n < 0:
            import io
            w = io.BytesIO()
            self.d.WriteTo(w)
            return w.getvalue()
        p = bytearray(n)
        return bytes(p[:self.d.Read(p)])

    def readinto(self, p):
        return self.d.Read(p)

    def write_to(self, w):
        return self.d.WriteTo(w)

    def close(self):
        self.d.Close()


def NewReader(r, *opts, **kw):
    """zstd.NewReader(r, opts...) (decoder.go:88-118).  With r None the decoder serves DecodeAll and its batched forms (Read raises
    ErrDecoderNilInput); with a reader it streams: Read / WriteTo.  batch_bytes: how much is pulled from r, and decoded, at a time."""
    d = Decoder(*opts, **kw)
    if r is not None:
        d.Reset(r)
    return d
