"""The model of the HuffmanOnly writers (tests/deflate_model.py) against what pins it: the reference's own byte-exact expectations of
writeBlockHuff (flate/testdata/huffman-*.in -> huffman-*.golden), the reference's own inflate and gunzip on every stream the
model writes, CPython's zlib / gzip on the same, the committed digests, and the conditions the case set has to meet.

What is NOT pinned by bytes of the reference: the decisions across blocks (lastHeader, reuse against a new table, the owed EOB).  They
rest on the restatement, on the reference's inflate accepting every stream, and on review (profiles/flate_reference_parity.md)."""
import glob
import gzip
import importlib.util
import os
import zlib

import pytest

import deflate_cases as D
import deflate_model as M
import oracle_goref as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_flate = pytest.mark.skipif(not G.flate_available(), reason="oracle/_ref/libzstdref.so with the reference's inflate neither present nor buildable")
needs_gunzip = pytest.mark.skipif(not G.gunzip_available(), reason="oracle/_ref/libzstdref.so with the reference's gunzip neither present nor buildable")
ALL = D.directed() + D.seeded()
FL_EOF = 2  # io.ErrUnexpectedEOF in the classes of include/kcgpu.h, which oracle_goref reports


def golden_pairs():
    ins = sorted(glob.glob(os.path.join(GOLD, "flate_in", "huffman-*.in")))
    assert len(ins) == 9
    return [(os.path.basename(p)[:-3], open(p, "rb").read(), open(os.path.join(GOLD, "flate", os.path.basename(p)[:-3] + ".golden"), "rb").read()) for p in ins]


@pytest.mark.parametrize("name,data,want", golden_pairs(), ids=[p[0] for p in golden_pairs()])
def test_model_writes_the_references_goldens(name, data, want):
    """One writeBlockHuff(false, all, false) and flush, at logNewTablePenalty 8: the reference's TestWriteBlockHuff, byte for byte."""
    assert M.block_huff_alone(data, penalty=8) == want


@needs_flate
def test_reference_inflate_reads_every_stream():
    for c in ALL:
        out = D.model(c)[0]
        got, err, used = G.flate_inflate(out, max_out=len(c[1]) + 64)
        if c[4] == M.END_CLOSE:
            assert (got, err, used) == (c[1], 0, len(out)), c[0]
        else:  # a flushed stream stays open: everything is there, and the reader wants more
            assert got == c[1] and err == FL_EOF, c[0]


@needs_gunzip
def test_reference_gunzip_reads_every_stream():
    for c in ALL:
        if c[4] != M.END_CLOSE:
            continue
        out = D.model(c, True)[0]
        got, err, used = G.gunzip(out, max_out=len(c[1]) + 64)
        assert (got, err, used) == (c[1], 0, len(out)), c[0]


def test_cpython_reads_every_stream():
    for c in ALL:
        out, gz = D.model(c)[0], D.model(c, True)[0]
        do = zlib.decompressobj(-15)
        assert do.decompress(out) == c[1] and do.unused_data == b"", c[0]
        assert do.eof == (c[4] == M.END_CLOSE), c[0]  # a Flush-ended stream: no end of stream reported
        assert len(out) <= M.bound(len(c[1]), c[2]) and len(gz) <= M.bound(len(c[1]), c[2]) + 18, c[0]
        if c[4] == M.END_CLOSE:
            assert gzip.decompress(gz) == c[1], c[0]
        else:
            dg = zlib.decompressobj(31)
            assert dg.decompress(gz) == c[1] and not dg.eof, c[0]
            assert gz == M.GZIP_HEADER + out, c[0]


def test_digests():
    spec = importlib.util.spec_from_file_location("make_deflate_golden", os.path.join(GOLD, "make_deflate_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.OUT) as f:
        assert f.read().split("\n")[:-1] == mod.digests()


def test_case_set_conditions():
    """All eight bit phases at a block boundary and at the stream's end; in the seeded set every decision at least 20 times and both
    endings at least a quarter each."""
    counts = D.check_conditions()
    assert set(counts) == set(M.DECISIONS)
    names = [c[0] for c in ALL]
    assert len(set(names)) == len(names) and len(D.seeded()) == 400


def test_empty_input_is_the_fixed_block():
    assert M.deflate(b"") == bytes([0x03, 0x00])       # writeBits(3, 3), writeBits(0, 7), flush
    assert M.deflate(b"", end=M.END_FLUSH) == bytes([0x00, 0x00, 0x00, 0xFF, 0xFF])
    assert M.gzip_deflate(b"")[:10] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
