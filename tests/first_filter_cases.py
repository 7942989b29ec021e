"""Inputs and the NumPy restatement for the first-occurrence filter of the SpeedFastest HBM-table kernel (kc_zstd_first.hip):
shared by tests/test_emu_first_filter.py (wave emulator) and tests/test_gpu_first_filter.py (device)."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# odd lengths make every later unit of a batch start off the 16-byte and 64-byte grids the bits are laid out on
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 4099, 65536, 65537, 131072]
KINDS = ["zeros", "period3", "text", "random"]
PRIME6 = np.uint64(227718039650203)
TABLE_BITS = 15


@functools.lru_cache(maxsize=None)
def content(kind):
    n = sum(LENS)
    if kind == "zeros":
        return bytes(n)
    if kind == "period3":
        return (b"abc" * (n // 3 + 1))[:n]
    if kind == "text":
        t = open(os.path.join(HERE, "golden", "ref_inputs", "Mark.Twain-Tom.Sawyer.txt"), "rb").read()
        assert len(t) >= n
        return t[:n]
    return np.random.default_rng(0xF1257).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def units(kind, lens=tuple(LENS)):
    c, out, at = content(kind), [], 0
    for ln in lens:
        out.append(c[at:at + ln])
        at += ln
    return out


def all_units():
    """(kind, unit) for every kind and length, kinds interleaved: neighbours in a batch differ in content."""
    return [(k, u) for i in range(len(LENS)) for k in KINDS for u in [units(k)[i]]]


def first_ref(u):
    """The definition: position p (p + 8 <= len) is marked iff no smaller position of the unit has the same hash6(load64(p), 15)
    (the hash takes the low 6 of the 8 bytes).  Returns a bool array of len(u)."""
    n = len(u)
    out = np.zeros(n, dtype=bool)
    m = n - 7
    if m <= 0:
        return out
    a = np.frombuffer(u, dtype=np.uint8).astype(np.uint64)
    v = np.zeros(m, dtype=np.uint64)
    for i in range(6):
        v |= a[i:i + m] << np.uint64(8 * i)
    with np.errstate(over="ignore"):
        h = ((v << np.uint64(16)) * PRIME6) >> np.uint64(64 - TABLE_BITS)
    _, idx = np.unique(h, return_index=True)  # (the first index of every value)
    out[idx] = True
    return out


def unpack_bits(words, src_addr, off, i, n):
    """Unit i's n bits out of the kernel's words (KcFirstParams: bit d & 63 of word (d >> 6) + i for the byte at distance d from the
    source address rounded down to 16 bytes)."""
    if n == 0:
        return np.zeros(0, dtype=bool)
    d0 = (src_addr & 15) + int(off[i])
    w0, w1 = d0 >> 6, (d0 + n - 1) >> 6
    w = words[w0 + i:w1 + i + 1]
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    return bits[d0 - (w0 << 6):d0 - (w0 << 6) + n].astype(bool)
