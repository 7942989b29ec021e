"""The judge judged: tests/flate_model.py against the reference's own test vectors (tests/golden/flate_vectors.json: the 28 rows of
TestStreams, the gunzipTests rows; tests/golden/flate/: the non-final streams of flate/testdata) and against zlib on streams zlib
writes.  Where model and zlib part ways on a hostile input, the rule of the reference that decides is printed (flate_model R1..R5)."""
import gzip
import json
import os
import zlib

import pytest

import flate_cases as FC
import flate_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VEC = json.load(open(os.path.join(GOLD, "flate_vectors.json")))


def zlib_raw(data, zdict=None):
    """(bytes, ok, consumed) of zlib on a raw stream; ok False when zlib refuses it or it does not end."""
    d = zlib.decompressobj(-15, zdict) if zdict else zlib.decompressobj(-15)
    try:
        out = d.decompress(data)
    except zlib.error:
        return b"", False, 0
    return out, d.eof, len(data) - len(d.unused_data)


def test_streams_vectors():
    assert len(VEC["streams"]) == 28
    for row in VEC["streams"]:
        data = bytes.fromhex(row["stream"])
        out, cls, _ = M.inflate(data)
        zout, zok, _ = zlib_raw(data)
        if row["want"] == "fail":
            assert cls != M.OK, row["desc"]
            assert not zok, row["desc"]
        else:
            assert (out, cls) == (bytes.fromhex(row["want"]), M.OK), row["desc"]
            assert zok and zout == out, row["desc"]


def test_gunzip_vectors():
    assert len(VEC["gunzip"]) == 13
    for row in VEC["gunzip"]:
        out, cls, _, hdr = M.gunzip(bytes.fromhex(row["gzip"]), want_header=True)
        assert cls == row["class"], row["desc"]
        # (rows that end in an error too: the bytes in front of it are the row's, as TestDecompressor compares them)
        assert out == bytes.fromhex(row["want"]), row["desc"]
        assert hdr["Name"] == row["name"], row["desc"]


def test_golden_streams_are_data_then_eof():
    names = sorted(os.listdir(os.path.join(GOLD, "flate")))
    assert len(names) == 10
    for f in names:
        data = open(os.path.join(GOLD, "flate", f), "rb").read()
        out, cls, used = M.inflate(data)
        zout, zok, _ = zlib_raw(data)
        assert cls == M.EOF and not zok, f       # no final block
        # R4: in a block that is not the last the reference wants the end-of-block code's length + 10 bits in its buffer before every
        # symbol, so the symbols inside the input's last bits are never decoded: a prefix of what zlib hands out
        assert zout.startswith(out) and len(zout) - len(out) <= 25 and used == len(data), (f, len(out), len(zout))


TEXT = (b"Call me Ishmael. Some years ago - never mind how long precisely - having little or no money in my purse, " * 40) + bytes(range(256)) * 6


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE])
@pytest.mark.parametrize("zdict", [None, b"having little or no money, never mind how long"])
def test_model_equals_zlib_on_zlib_streams(level, strategy, zdict):
    s = FC._deflate(TEXT, level, strategy, zdict) + b"trailing"
    out, cls, used = M.inflate(s, zdict or b"")
    zout, zok, zused = zlib_raw(s, zdict)
    assert zok and zout == TEXT
    assert (out, cls, used) == (zout, M.OK, zused)


def test_gzip_multi_member():
    parts = [b"first member ", b"", b"third " * 1000]
    blob = b"".join(gzip.compress(p, lvl) for p, lvl in zip(parts, (1, 6, 9)))
    assert M.gunzip(blob) == (gzip.decompress(blob), M.OK, len(blob))
    first = len(gzip.compress(parts[0], 1))
    assert M.gunzip(blob, multistream=False) == (parts[0], M.OK, first)


def test_directed_cases_against_zlib():
    """Every directed raw-DEFLATE case: where zlib accepts, the model returns the same bytes and consumed; where they part, the rule
    that fired in the model is the one that explains it."""
    parted = {}
    for c in FC.cases():
        if c.fmt != "flate":
            continue
        out, cls, used = M.inflate(c.data, c.dict)
        rules = set(M.fired)
        zout, zok, zused = zlib_raw(c.data, c.dict or None)
        if zok:
            assert (out, cls, used) == (zout, M.OK, zused), c.name
        elif cls == M.OK:  # only the raw io.EOF makes the reference accept what zlib does not finish
            # (everything was read, and what stands is what zlib, waiting for more input, has handed out so far)
            assert "R3" in rules and used == len(c.data) and zout == out, c.name
            parted[c.name] = "R3: %d bytes stand" % len(out)
    for k, v in sorted(parted.items()):
        print(k, "->", v)
    assert parted


def test_mutations_against_zlib():
    """The 480 mutations: what both accept has the same bytes and consumed; what both refuse needs no rule; where they part, the rule
    that fired in the model explains it — R3 (the input ended inside extra bits: everything was read, and what stands is what
    zlib, waiting for more input, has handed out so far) where only the model accepts, R2 (an incomplete code) where only zlib does."""
    fl, _ = FC.mutations()
    both = neither = 0
    parted = []
    for c in fl:
        out, cls, used = M.inflate(c.data)
        rules = set(M.fired)
        assert (out, cls, used) == FC.verdict(c)
        zout, zok, zused = zlib_raw(c.data)
        if zok and cls == M.OK:
            assert (out, used) == (zout, zused), c.name
            both += 1
        elif not zok and cls != M.OK:
            neither += 1
        elif cls == M.OK:
            assert "R3" in rules and used == len(c.data), (c.name, rules)
            assert zout == out, c.name
            parted.append((c.name, "R3", len(out)))
        else:
            assert "R2" in rules, (c.name, M.NAMES[cls], rules)
            parted.append((c.name, "R2", len(out)))
    for p in parted:
        print(*p)
    assert both + neither + len(parted) == 480 and both >= 120 and neither >= 120
