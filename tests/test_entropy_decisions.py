"""The directed inputs of tests/entropy_cases.py reach the decisions they are named after (CPU).

For every case and every level it names: the oracle's decision counters (oracle/kco_counters.h) show the decision, the oracle's own
decoder restores the input, and - where oracle/_ref is built - the translated reference (tests/oracle_goref.py) writes the same
frame.  A difference there is a bug of the oracle on a branch that nothing exercised before.

The last test takes the union over all cases: every decision counter is reached at level 1 and at level 3 or 4, or stands in
OUT_OF_REACH with the argument (in full in profiles/entropy_decisions.md).  tests/test_emu_entropy_decisions.py and
tests/test_gpu_entropy_decisions.py compare the device code with the oracle on the same cases."""
import functools

import pytest

import entropy_cases as ec
import oracle_goref
import oracle_lib

# Decisions that need a unit far above the sizes of this suite's units (256 KiB at the most): a lower bound of the unit size, from
# the code.  They are reachable in principle and NOT proven out of reach; no case covers them.
BEYOND_UNIT_SIZE = {
    "of zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin": (
        2 << 20, "the only histograms that get there have 22, 43 or 44 symbols once each (tools/find_entropy_cases.py "
                 "--enumerate-round-robin): at least 22 distinct offset codes in one block, so one of them is 21 or above, an offset of "
                 "2^21 - 3 bytes and more"),
    "of zstd/fse_encoder.go:488 writeCount: zero run >= 24": (
        32 << 20, "a run of 24 unused codes after the first unused one ends at a used code >= 25: an offset of 2^25 - 3 bytes and "
                  "more, and a window option above the 4 / 8 MiB of the levels"),
}

# Decisions no input can reach, with the levels the statement is about ("all", or 1 where only SpeedFastest's 64 KiB block is the
# reason) and the argument from the code.  profiles/entropy_decisions.md spells each one out.
_ALL_SMALL = ("`distributed` is incremented at most once per symbol with a non-zero count, so it is at most symbolLen; the exit "
              "compares it with symbolLen + 1")
OUT_OF_REACH = {
    "fse/compress.go:557 normalizeCount2: all small exit": ("all", _ALL_SMALL),
    "ll zstd/fse_encoder.go:334 normalizeCount2: all small exit": ("all", _ALL_SMALL),
    "of zstd/fse_encoder.go:334 normalizeCount2: all small exit": ("all", _ALL_SMALL),
    "ml zstd/fse_encoder.go:334 normalizeCount2: all small exit": ("all", _ALL_SMALL),
    "fse/compress.go:557 normalizeCount2: second lowOne pass": (
        "all", "Huffman weights: at most 12 symbols, at most 255 of them counted, table log always 5.  The pass needs "
               "total / toDistribute > lowOne, i.e. at least 11 symbols set aside as small and one left with >= 21 * (lowOne + 1) "
               "counts, which with lowOne = 3n >> 6 needs n >= 704"),
    "fse/compress.go:557 normalizeCount2: total == 0 round robin": (
        "all", "every symbol small means at most 2 of 32 slots each for at most 12 symbols in the first normalisation: no overshoot, "
               "normalizeCount2 is not entered; via the second pass: see that entry"),
    "huff0/compress.go:269 compress4X: stream above 65535 bytes": (
        "all", "a block holds at most 128 KiB of literals, a stream a quarter of them at no more than 11 bits each: 45056 bytes"),
    "zstd/blockenc.go:831 genCodes: highest OF code 30 (top)": (
        "all", "offset + 3 < 2^30 for every window the encoder accepts (MaxWindowSize = 2^29): the highest code is 29"),
    "zstd/blockenc.go:150 literalsHeader.setSize: RLE, 1 byte": (
        "all", "one header byte needs fewer than 16 literals (bits.Len32 < 5), and huff0, the only source of ErrUseRLE, is called "
               "for more than 16 literals only"),
    "zstd/blockenc.go:481 encode: compressed no smaller than raw with both headers": (
        "all", "huff0 returns ErrIncompressible unless out < n - (n >> 4); the check needs out >= n - (szComp - szRaw).  The "
               "headers differ by 1 byte for 17 <= n < 32 (3 : 2), where n >> 4 = 1, and by at most 2 beyond (3 : 2, 4 : 2, 4 : 3, "
               "5 : 3), where n >> 4 >= 2: never both"),
    "zstd/blockenc.go:831 genCodes: highest LL code 35 (top)": (
        1, "code 35 is a literal run of 65536 bytes and more in front of a match; SpeedFastest's blocks are 65536 bytes"),
    "zstd/blockenc.go:831 genCodes: highest ML code 52 (top)": (
        1, "code 52 is a match of 65539 bytes and more; SpeedFastest's blocks are 65536 bytes and a match ends with its block"),
}


@functools.lru_cache(maxsize=None)
def results():
    """{(case name, level): (counters, frame)}, computed once for the whole module: one whole-unit EncodeAll per case and level,
    as the counts of the issue's table were taken."""
    out = {}
    for c in ec.CASES:
        u = ec.unit(c)
        for lv in ec.LEVELS:
            kw = ec.oracle_kw(c, lv)
            e = oracle_lib.ZstdOracle(**kw)
            oracle_lib.counters(reset=True)
            fr = e.encode_all(u)
            out[c[0], lv] = (oracle_lib.counters(reset=True), fr)
    return out


def test_counter_names_cite_the_reference():
    import ctypes as C
    names = list(oracle_lib.counters())  # (a dict: a repeated name would have merged two counters)
    buf = C.create_string_buffer(1 << 16)
    assert oracle_lib.lib().kco_debug_counters(buf, len(buf), 0) > 0
    assert len(buf.value.decode().splitlines()) == len(names) > 100
    assert all(".go:" in n for n in names)
    assert oracle_lib.lib().kco_debug_counters(buf, 10, 0) == -1  # too small a buffer is reported, not overrun


def test_counters_count_and_reset():
    oracle_lib.counters(reset=True)
    assert not any(oracle_lib.counters().values())
    oracle_lib.ZstdOracle(level=3).encode_all(ec.unit(ec.CASES[0]))
    assert any(oracle_lib.counters().values())
    assert any(oracle_lib.counters(reset=True).values())
    assert not any(oracle_lib.counters().values())


@pytest.mark.parametrize("case", ec.CASES, ids=[c[0] for c in ec.CASES])
def test_case_reaches_its_decisions(case):
    name, _, _, reaches = case
    u = ec.unit(case)
    for lv, decisions in sorted(reaches.items()):
        ctr, fr = results()[name, lv]
        missing = [d for d in decisions if not ctr.get(d)]
        assert not missing, "level %d: the oracle no longer takes %r on this input" % (lv, missing)
    for lv in ec.LEVELS:
        kw = ec.oracle_kw(case, lv)
        fr = results()[name, lv][1]
        assert oracle_lib.zstd_decode(fr, len(u) + 16, dict_content=kw.get("dict_content")) == u, "level %d: the oracle's frame does not decode to the input" % lv
        if not ec.uses_dict(case):  # (and the system's libzstd, where there is one; it takes no raw-content dictionary with an id)
            assert oracle_lib.zstd_decompress(fr, len(u) + 16) == u


@pytest.mark.skipif(not oracle_goref.available(), reason="oracle/_ref is not built here")
@pytest.mark.parametrize("case", ec.CASES, ids=[c[0] for c in ec.CASES])
def test_case_frames_equal_the_translated_reference(case):
    u = ec.unit(case)
    for lv in ec.LEVELS:
        kw = ec.oracle_kw(case, lv)
        assert results()[case[0], lv][1] == oracle_goref.zstd_encode_all(u, **kw), \
            "level %d: the oracle's frame differs from the reference's own EncodeAll (translated)" % lv


def test_every_decision_is_reached_or_proven_out_of_reach():
    names = list(oracle_lib.counters())
    assert set(OUT_OF_REACH) <= set(names) and set(BEYOND_UNIT_SIZE) <= set(names) and not set(OUT_OF_REACH) & set(BEYOND_UNIT_SIZE)
    assert all(size >= 8 * (256 << 10) for size, _ in BEYOND_UNIT_SIZE.values())
    hit = {lv: set() for lv in ec.LEVELS}
    for (name, lv), (ctr, _) in results().items():
        hit[lv] |= {d for d, v in ctr.items() if v}
    missing = []
    for d in names:
        if d in BEYOND_UNIT_SIZE:
            continue
        scope = OUT_OF_REACH.get(d, (None,))[0]
        if scope == "all":
            # a decision listed as unreachable that IS reached means the argument is wrong
            assert not any(d in hit[lv] for lv in ec.LEVELS), "%r is listed in OUT_OF_REACH but a case reaches it" % d
            continue
        if scope == 1:
            assert d not in hit[1], "%r is listed as out of reach at level 1 but a case reaches it" % d
        elif d not in hit[1]:
            missing.append((d, "level 1"))
        if d not in hit[3] and d not in hit[4]:
            missing.append((d, "level 3 or 4"))
    assert not missing, "decisions no case reaches: %r" % missing
