"""compress/zlib's reader on the device: zlib streams (RFC 1950) inflated in batches of independent inputs (include/kcgpu.h
kc_zlib_inflate*).  The header, the preset dictionary's id, the DEFLATE stream and the Adler-32 of the decoded bytes are checked on
the device; the dictionary's own Adler-32 is computed once on the host, from all of its bytes.  There is no CPU fallback.

Every input is read as by a fresh zlib.NewReaderDict.  The reference hands the dictionary to a reused decompressor even where the
stream has no FDICT (Reset, zlib/reader.go:177-179); that is not modelled: Reader.Reset here behaves as a new NewReaderDict."""
from . import flate
from .flate import InflateError, CorruptInputError, ErrUnexpectedEOF  # noqa: F401


class ErrHeader(InflateError):
    """zlib.ErrHeader: "zlib: invalid header"."""

    def __init__(self, status=flate.FL_HEADER):
        super().__init__(status)


class ErrChecksum(InflateError):
    """zlib.ErrChecksum: "zlib: invalid checksum" — the Adler-32 of the decoded bytes."""

    def __init__(self, status=flate.FL_CHECKSUM):
        super().__init__(status)


class ErrDictionary(InflateError):
    """zlib.ErrDictionary: "zlib: invalid dictionary" — the stream's DICTID is not the Adler-32 of the dictionary given."""

    def __init__(self, status=flate.FL_DICTIONARY):
        super().__init__(status)


_ERRORS = dict(flate._ERRORS)
_ERRORS.update({flate.FL_HEADER: ErrHeader, flate.FL_CHECKSUM: ErrChecksum, flate.FL_DICTIONARY: ErrDictionary})


def InflateAll(src, in_off, dict=None, device=0):
    """N x io.ReadAll(zlib.NewReaderDict(input_i, dict)) in one batch (host buffers): a list of bytes or the InflateError per input."""
    b = flate.Batch("kc_zlib_inflate", _ERRORS, dict=dict, device=device)
    try:
        return b.all_host(src, in_off)
    finally:
        b.close()


def InflateBounds(src, in_off, dict=None, device=0):
    """The sizing pass alone (kc_zlib_inflate_bound): (sizes, status short of the Adler-32, consumed)."""
    import numpy as np
    b = flate.Batch("kc_zlib_inflate", _ERRORS, dict=dict, device=device)
    try:
        src = np.ascontiguousarray(src, dtype=np.uint8)
        if len(src) == 0:
            src = np.zeros(1, dtype=np.uint8)
        return b.bounds(src.ctypes.data, in_off, False)
    finally:
        b.close()


def InflateAllDevice(d_src_ptr, in_off, d_dst_ptr, dst_cap, dict=None, device=0, stream=None):
    """Device-resident form: (uint64[n + 1] offsets, uint32[n] status, uint64[n] consumed).  A failed input's range is empty, or
    zero-filled where the Adler-32 failed."""
    b = flate.Batch("kc_zlib_inflate", _ERRORS, dict=dict, device=device, stream=stream)
    try:
        return b.inflate(d_src_ptr, in_off, d_dst_ptr, dst_cap, True)
    finally:
        b.close()


class Reader(flate.Reader):
    """The ReadCloser of zlib.NewReader / NewReaderDict (zlib/reader.go:68-132): Read, WriteTo, Reset(r, dict), Close, consumed.
    Like flate.Reader the whole input is read and decoded on the device on first use."""

    _prefix, _errors = "kc_zlib_inflate", _ERRORS


def NewReader(r, device=0):
    """zlib.NewReader(r)."""
    return Reader(r, None, device=device)


def NewReaderDict(r, dict, device=0):
    """zlib.NewReaderDict(r, dict): the dictionary counts only where the stream asks for one, and must then be the one it names."""
    return Reader(r, dict, device=device)
