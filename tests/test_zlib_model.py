"""tests/zlib_model.py held to what can be executed: the reference's own expectations of its zlib reader (zlibTests of
zlib/reader_test.go, committed as data in tests/golden/zlib_vectors.json), CPython's zlib for the container on every family of
tests/zlib_cases.py, and — where oracle/_ref is present — the reference's own translated inflate for the body.  The reference's
zlib reader itself is not among the translated sources (oracle/ is frozen), so no test here runs it."""
import collections
import zlib

import pytest

import flate_model as M
import oracle_goref as G
import zlib_cases as ZC
import zlib_model as Z

needs_flate = pytest.mark.skipif(not G.flate_available(), reason="oracle/_ref/libzstdref.so with the reference's inflate neither present nor buildable")

# Cases on which CPython's zlib and the reference are KNOWN to differ, by name, with the reference's line: a stream with FDICT read
# without a dictionary is compared with adler32(nil) = 1 (zlib/reader.go:164-165) and, given DICTID 1, accepted; zlib asks for a
# dictionary.  None of the generated family is excluded.
NOT_ZLIBS = {"fdict/none-given-id-1": "zlib/reader.go:164-165"}


@pytest.fixture(scope="module")
def families():
    fams = ZC.families()
    for stale in (False, True):
        ZC.warm([c for _, cs in fams for c in cs], stale)
    return dict(fams)


def test_model_meets_the_references_vectors():
    rows = ZC.vectors()
    assert len(rows) == 14
    for c, want, cls in rows:
        for stale in (False, True):
            out, got, used = Z.inflate(c.data, c.dict, stale_tables=stale)
            assert got == cls, (c.name, Z.NAMES[got])
            if cls == Z.OK:   # (the reference's test compares the bytes only where no error is wanted)
                assert out == want, c.name
    by = {c.name: Z.inflate(c.data, c.dict) for c, _, _ in rows}
    assert by["vec/excess data is silently ignored"][2] == 8 and by["vec/dictionary"][2] == 19


def cpython(c):
    """-> (eof, bytes, unused_data), or None where zlib refuses the stream."""
    d = zlib.decompressobj(zdict=c.dict) if c.dict else zlib.decompressobj()
    try:
        out = d.decompress(c.data)
    except zlib.error:
        return None
    return d.eof, out, d.unused_data


@pytest.mark.parametrize("family", ["directed", "zmut", "generated"])
def test_model_agrees_with_cpython(families, family):
    """OK <=> decompressobj(...).eof, the same bytes, and unused_data is what lies behind `consumed`."""
    bad, excluded = [], []
    for c in families[family]:
        out, cls, used = ZC.verdict(c)
        if c.name in NOT_ZLIBS:
            excluded.append(c.name)
            continue
        z = cpython(c)
        if (cls == Z.OK) != (z is not None and z[0]) or (cls == Z.OK and (out, c.data[used:]) != (z[1], z[2])):
            bad.append((c.name, Z.NAMES[cls], used, None if z is None else (z[0], len(z[1]), len(z[2]))))
    assert not bad, (len(bad), bad[:10])
    if family == "generated":
        assert not excluded
    assert len(excluded) * 100 <= len(families[family])


def test_the_case_cpython_differs_on(families):
    c = next(c for c in families["directed"] if c.name == "fdict/none-given-id-1")
    assert ZC.verdict(c)[1] == Z.OK and cpython(c) in (None, (False, b"", b""))


def test_directed_cases_say_what_their_names_say(families):
    cs = families["directed"]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) and len(cs) >= 80
    got = {c.name: ZC.verdict(c) for c in cs}
    cls = {k: v[1] for k, v in got.items()}
    assert all(cls["hdr/cinfo-%d" % k] == (Z.OK if k <= 7 else Z.HEADER) for k in range(16))
    assert all(cls["hdr/cm-%d" % k] == Z.HEADER for k in (0, 7, 9, 15))
    fchecks = [k for k in cls if k.startswith("hdr/fcheck-")]
    assert len(fchecks) == 32 and all(cls[k] == (Z.OK if k.endswith("-right") else Z.HEADER) for k in fchecks)
    assert all(cls["hdr/flevel-%d" % k] == Z.OK for k in range(4))
    for kind in ("stored", "fixed", "dynamic", "fdict"):
        cut = [k for k in cls if k.startswith("cut/%s-" % kind) and not k.endswith("-whole")]
        assert len(cut) >= 15 and all(cls[k] == Z.EOF for k in cut), kind   # every proper prefix: io.ErrUnexpectedEOF
    assert all(cls["cut/%s-whole" % kind] == Z.OK for kind in ("stored", "fixed", "dynamic"))
    assert [cls["fdict/" + k] for k in ("right", "right-40000", "id-of-the-tail-40000", "wrong", "none-given-id-1", "none-given-id-1-match-into-it",
                                        "none-given-id-other", "given-stream-has-none", "given-stream-has-none-match-into-it")] == \
        [Z.OK, Z.OK, Z.DICTIONARY, Z.DICTIONARY, Z.OK, Z.CORRUPT, Z.DICTIONARY, Z.OK, Z.CORRUPT]
    assert [cls["trailer/" + k] for k in ("one-bit", "little-endian", "s1-s2-swapped")] == [Z.CHECKSUM] * 3
    for k in ("excess-1", "excess-4", "excess-a-second-stream"):
        c = cs[names.index("trailer/" + k)]
        assert cls[c.name] == Z.OK and got[c.name][2] == got["trailer/excess-1"][2] < len(c.data)
    assert got["trailer/empty-payload"] == (b"", Z.OK, 8) and got["trailer/empty-payload-stored"][:2] == (b"", Z.OK)
    c = cs[names.index("trailer/body-ends-by-raw-eof")]
    assert cls[c.name] == Z.EOF and "R3" in ZC.fired(c)


def test_generated_shares(families):
    """At least a quarter OK and a quarter not OK, and every one of CORRUPT, EOF and CHECKSUM; the mutations and the sweep say what
    they are."""
    cs = families["generated"]
    assert len(cs) == 2000
    n = collections.Counter(ZC.verdict(c)[1] for c in cs)
    print({Z.NAMES[k]: v for k, v in n.items()})
    assert n[Z.OK] * 4 >= len(cs) and (len(cs) - n[Z.OK]) * 4 >= len(cs), n
    assert n[Z.CORRUPT] and n[Z.EOF] and n[Z.CHECKSUM], n
    assert len(families["zmut"]) == 480
    sw = ZC.adler_sweep()
    assert len(sw) == len(ZC.SWEEP_LENGTHS) * 3 * 3 * 2
    wraps = [c for _, c in sw if c.name.startswith(ZC.ADLER_WRAPS + "-first") and not c.name.endswith("-bad")]
    assert len(wraps) == 3 and all(c.data[-4:] == b"\x00\x00\x00\x01" for c in wraps)
    assert zlib.adler32(b"\xff" * 65521) == 1 == zlib.adler32(b"")


def test_two_modes_differ_only_where_r6_fired(families):
    differ = 0
    for cs in families.values():
        for c in cs:
            if "R6" not in ZC.fired(c, True):
                assert ZC.verdict(c, True) == ZC.verdict(c, False), c.name
            else:
                differ += ZC.verdict(c, True) != ZC.verdict(c, False)
                assert ZC.verdict(c, False)[1] != Z.OK, c.name
    assert differ > 0


@needs_flate
@pytest.mark.parametrize("family", ["directed", "zmut", "generated"])
def test_model_over_the_references_inflate(families, family):
    """The container around the reference's OWN inflate (translated) answers what the container around the model as the reference
    (stale_tables=True) answers."""
    bad = []
    for c in families[family]:
        want = Z.inflate(c.data, c.dict, body=G.flate_inflate)
        if want != ZC.verdict(c, True):
            bad.append((c.name, want[1:], ZC.verdict(c, True)[1:]))
    assert not bad, (len(bad), bad[:10])
