"""The first-occurrence filter of the SpeedFastest HBM-table kernel on the CPU wave emulator (no GPU): the pre-pass's bits
(kc_zstd_first.hip) against a NumPy restatement of their definition, and the match finder with the bits (kc_zstd_match.hip) against
the same kernel without them and against the oracle's parse.  tests/test_gpu_first_filter.py runs the frames on the device."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import first_filter_cases as ffc
import oracle_lib

BLOCK = 65536  # (the 65 537- and 131 072-byte units are two blocks: the second one is parsed with history, on the unit's table)


def _pack(units):
    """Units back to back in a 16-byte aligned buffer (as a device allocation is) -> (keep-alive array, address, offsets, first blocks)."""
    n = len(units)
    off = np.zeros(n + 1, dtype=np.uint64)
    blk0 = np.zeros(n + 1, dtype=np.uint32)
    for i, u in enumerate(units):
        off[i + 1] = off[i] + len(u)
        blk0[i + 1] = blk0[i] + (len(u) + BLOCK - 1) // BLOCK
    raw = b"".join(units) + b"\0" * 64
    al = np.zeros(len(raw) + 32, dtype=np.uint8)
    o = (-al.ctypes.data) % 16
    al[o:o + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return al, al.ctypes.data + o, off, blk0


def _first_words(addr, off, n):
    L = emu_lib.lib()
    L.kcemu_zfast_first_words.restype = C.c_uint64
    L.kcemu_zfast_first_words.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    L.kcemu_zfast_first.restype = C.c_int
    L.kcemu_zfast_first.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    nw = int(L.kcemu_zfast_first_words(addr, int(off[n]), n))
    words = np.full(nw + 8, 0xA7A7A7A7A7A7A7A7, dtype=np.uint64)  # (what the kernel does not write is not zero; 8 guard words)
    assert L.kcemu_zfast_first(addr, off.ctypes.data, n, words.ctypes.data) == 0
    assert np.all(words[nw:] == np.uint64(0xA7A7A7A7A7A7A7A7)), "the pre-pass wrote behind the words kc_zfast_first_words gives it"
    return words


@pytest.fixture(scope="module")
def bits_by_kind():
    """Per kind: [(unit, kernel bits, restated bits)] — every length of the kind in ONE launch, so that units start at odd addresses."""
    out = {}
    for shift in (0, 5):  # the source itself on and off the 16-byte grid
        for kind in ffc.KINDS:
            us = ffc.units(kind)
            al, addr, off, _ = _pack([b"x" * shift] + us)
            addr += shift  # (the unit in front is dropped: src points 5 bytes into a granule)
            off = (off[1:] - off[1]).copy()
            words = _first_words(addr, off, len(us))
            out[kind, shift] = [(u, ffc.unpack_bits(words, addr, off, i, len(u)), ffc.first_ref(u)) for i, u in enumerate(us)]
    return out


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("kind", ffc.KINDS)
def test_bits_are_sound(bits_by_kind, kind, shift):
    """No bit set that the definition leaves clear (a wrong bit would hide a real candidate from the parse)."""
    for u, got, ref in bits_by_kind[kind, shift]:
        bad = np.nonzero(got & ~ref)[0]
        assert len(bad) == 0, "%s unit of %d bytes: position %d marked, but an earlier position has its hash" % (kind, len(u), bad[0])
    if kind == "zeros":  # one hash: exactly position 0 of every unit with 8 bytes
        for u, got, ref in bits_by_kind[kind, shift]:
            assert int(got.sum()) == (1 if len(u) >= 8 else 0) and (len(u) < 8 or got[0])


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("kind", ["text", "random"])
def test_bits_are_complete(bits_by_kind, kind, shift):
    """At least 90 % of the definition's bits are set.  The kernel's model says all of them: it keeps no lossy step scratch — the
    positions of a 64-position step whose hashes were not seen before either all find their bit clear when they set it (then no
    two share a hash and each is a first occurrence), or they compare their hashes lane by lane and the lowest lane of each hash
    is marked.  So nothing aliases, and the bits equal the definition's (positions without 8 bytes behind them are in neither)."""
    tot_ref = tot_got = 0
    for u, got, ref in bits_by_kind[kind, shift]:
        r, g = int(ref.sum()), int((got & ref).sum())
        tot_ref += r
        tot_got += g
        assert g >= 0.9 * r, "%s unit of %d bytes: %d of %d first occurrences marked" % (kind, len(u), g, r)
        assert g == r, "%s unit of %d bytes: %d of %d first occurrences marked, the kernel's model says all" % (kind, len(u), g, r)
    print("%s shift %d: %d of %d first occurrences marked (%.2f %%)" % (kind, shift, tot_got, tot_ref, 100.0 * tot_got / tot_ref))
    assert tot_got >= 0.9 * tot_ref


# ---- the match finder with the bits ----

def _parse(units, first, xseg_k, epoch=0, tables=None):
    """kc_zfast_match_grp_kernel<8> over `units` -> (sequence words, block records) as the kernel leaves them.  xseg_k 2^20: the plain
    compiled form, below: the form with cross-segment rounds and the empty-group filter."""
    n = len(units)
    al, addr, off, blk0 = _pack(units)
    L = emu_lib.lib()
    nb = int(blk0[n])
    stride = L.kcemu_zenc_seq_stride(BLOCK)
    seqs = np.zeros(max(nb, 1) * stride, dtype=np.uint64)
    meta = np.zeros(max(nb, 1) * 8, dtype=np.uint32)
    pb = L.kcemu_zenc_pos_bits(C.c_uint64(0), C.c_uint64(max(len(u) for u in units)))
    if tables is None:
        tables = np.zeros(((n + 7) // 8 * 8) << 15, dtype=np.uint32)
    words = _first_words(addr, off, n) if first else None
    L.kcemu_zfast_parse_grp_first.restype = C.c_int
    L.kcemu_zfast_parse_grp_first.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    r = L.kcemu_zfast_parse_grp_first(addr, off.ctypes.data, n, BLOCK, 4 << 20, 0, seqs.ctypes.data, meta.ctypes.data, stride, blk0.ctypes.data, 1, 1, pb,
                                      tables.ctypes.data, epoch, xseg_k, None if words is None else words.ctypes.data)
    assert r == 0
    return seqs, meta.reshape(-1, 8), stride, blk0


@pytest.fixture(scope="module")
def oracle_parse():
    return [oracle_lib.zstd_parse_unit(u, level=1, block_size=BLOCK) if len(u) else [] for _, u in ffc.all_units()]


def _cmp_oracle(units, got, ref, what):
    seqs, meta, stride, blk0 = got
    for ui, u in enumerate(units):
        for rb, (rseqs, rlits) in enumerate(ref[ui]):
            b = int(blk0[ui]) + rb
            ns = int(meta[b, 0])
            v = seqs[b * stride:b * stride + ns]
            tri = np.stack([(v >> np.uint64(44)).astype(np.uint32), ((v >> np.uint64(24)) & np.uint64(0xFFFFF)).astype(np.uint32),
                            (v & np.uint64(0xFFFFFF)).astype(np.uint32)], axis=1) if ns else np.zeros((0, 3), dtype=np.uint32)
            k = min(ns, len(rseqs))
            neq = np.nonzero((tri[:k] != rseqs[:k]).any(axis=1))[0] if k else []
            assert len(neq) == 0, "%s: unit %d (len %d) block %d first differing seq %d: emulated %r oracle %r" % (what, ui, len(u), rb, neq[0], tri[neq[0]], rseqs[neq[0]])
            assert ns == len(rseqs), "%s: unit %d (len %d) block %d: nseq %d vs oracle %d" % (what, ui, len(u), rb, ns, len(rseqs))
            assert int(meta[b, 1]) == len(rlits), "%s: unit %d block %d: nlit %d vs oracle %d" % (what, ui, rb, int(meta[b, 1]), len(rlits))


@pytest.mark.parametrize("xseg_k", [1 << 20, 0], ids=["plain-form", "tuned-form"])
def test_parse_is_identical_with_and_without_the_bits(oracle_parse, xseg_k):
    """Sequences and block records (counts, literal sums, flags with the round count, offsets in and out) are the same words with
    the bits and without, in both compiled forms, and the oracle's."""
    units = [u for _, u in ffc.all_units()]
    off_ = _parse(units, False, xseg_k)
    on = _parse(units, True, xseg_k)
    assert np.array_equal(on[1], off_[1]), "block records differ in blocks %r" % np.nonzero((on[1] != off_[1]).any(axis=1))[0][:8].tolist()
    assert np.array_equal(on[0], off_[0])
    _cmp_oracle(units, on, oracle_parse, "with the bits")


def test_parse_with_the_bits_over_a_stale_arena(oracle_parse):
    """Two launches on ONE uncleared arena (epoch stamps 1 and 2), the units in another order the second time: a bucket that the
    bits call empty holds the first launch's entries — they carry the other stamp and read as empty with the load as without it."""
    named = ffc.all_units()
    units = [u for _, u in named]
    tables = np.zeros(((len(units) + 7) // 8 * 8) << 15, dtype=np.uint32)
    _cmp_oracle(units, _parse(units, True, 1 << 20, epoch=1, tables=tables), oracle_parse, "stamp 1")
    assert tables.any()
    rev = list(reversed(units))
    ref = list(reversed(oracle_parse))
    on = _parse(rev, True, 1 << 20, epoch=2, tables=tables)
    _cmp_oracle(rev, on, ref, "stamp 2")
    off_ = _parse(rev, False, 1 << 20, epoch=1, tables=np.zeros_like(tables))
    assert np.array_equal(on[0], off_[0]) and np.array_equal(on[1], off_[1])


# ---- where the bits are used ----

def _rule(level, hist0=0, jobs=0, fed=0, n=4, opt=1):
    L = emu_lib.lib()
    L.kcemu_zenc_first_filter.restype = C.c_int
    L.kcemu_zenc_first_filter.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
    return L.kcemu_zenc_first_filter(level, hist0, jobs, fed, n, opt)


def test_rule_gives_bits_only_where_tables_start_empty():
    """kc_zenc_host.h's rule, the one kc_batch.cpp and the emulator's batch both ask: SpeedFastest without dictionary content in
    front of the units, without job prefixes or primed tables, not chunk-fed, and the option on."""
    assert _rule(1) == 1
    assert _rule(1, hist0=1) == 0 and _rule(1, hist0=32768) == 0   # a dictionary
    assert _rule(1, jobs=1) == 0                                   # the jobs of a WithConcurrentBlocks stream (prefixes, primed tables)
    assert _rule(1, fed=1) == 0                                    # chunk-fed
    assert _rule(1, opt=0) == 0
    assert _rule(1, n=0) == 0
    for level in (2, 3, 4):
        assert _rule(level) == 0


@pytest.mark.parametrize("tuned", [0, 1])
def test_frames_through_the_batch_path(tuned):
    """Whole frames through the emulator's encode batch (the library's host rules): with the option on the group kernel gets the bits,
    with it off or on the LDS-table path it gets none, and the frames are the oracle's every time."""
    L = emu_lib.lib()
    L.kcemu_set_first_filter.restype = None
    L.kcemu_set_first_filter.argtypes = [C.c_int]
    L.kcemu_last_first_filter.restype = C.c_int
    lens = (0, 1, 7, 8, 9, 63, 64, 65, 4099, 65537)
    units = ffc.units("text", lens) + ffc.units("random", lens[:-1]) + ffc.units("period3", lens)  # (below the size at which emu_lib forks children)
    assert sum(map(len, units)) < 200000
    ref = oracle_lib.ZstdOracle(level=1)
    want = [ref.encode_all(u) for u in units]
    try:
        for opt, grp, used in ((1, True, 1), (0, True, 0), (1, False, 0)):
            L.kcemu_set_first_filter(opt)
            frames, err, redo = emu_lib.zstd_frames(units, use_grp=grp, tuned=tuned, max_encoded_size=ref.max_encoded_size)
            assert err == 0
            assert L.kcemu_last_first_filter() == used
            bad = [(i, len(u)) for i, (u, f, w) in enumerate(zip(units, frames, want)) if f != w]
            assert not bad, "option %d, group kernel %r: frames differing from the oracle's (unit, length): %r" % (opt, grp, bad[:8])
    finally:
        L.kcemu_set_first_filter(1)  # the default
