"""tests/deflate_model.py and tests/stateless_model.py judged by the reference's OWN encoder: flate/huffman_bit_writer.go, huffman_code.go
(with its two sorts), token.go, stateless.go, the HuffmanOnly part of deflate.go and gzip/gzip.go, translated statement by statement
(oracle/ref_go) and compiled into oracle/_ref/libzstdref.so.

First the translation is held to the reference's own expectations: the nine huffman-*.golden files of writeBlockHuff and the 34
*.dyn.expect / *.sync.expect files of writeBlockDynamic, byte for byte.  That is what makes it a judge.  Then the models equal it,
byte for byte and with no case excluded, on every case the emulator and GPU suites use -- at both endings, raw and as gzip, with the
cases' eof and dictionaries -- on the writer-object sequences those suites spell by hand, and on EstimatedBits alone.  Where
oracle/_ref is absent, the committed digests of the reference's outputs (tests/golden/reference_go_deflate_sha256.txt) gate the models."""
import glob
import os
import struct
import zlib

import pytest

import deflate_cases as D
import deflate_model as DM
import deflate_ref_families as F
import oracle_goref as G
import stateless_cases as S
import stateless_model as SM
from test_stateless_model import _read, _tokens, golden_names, tokens_of

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIGESTS = os.path.join(GOLD, "reference_go_deflate_sha256.txt")
needs_deflate = pytest.mark.skipif(not G.deflate_available(), reason="oracle/_ref/libzstdref.so with the reference's DEFLATE writers neither present nor buildable")
FL_EOF = 2


@needs_deflate
def test_translation_writes_the_references_huffman_goldens():
    """One writeBlockHuff over the whole input at logNewTablePenalty 8, then flush: the reference's TestBlockHuff."""
    names = sorted(glob.glob(os.path.join(GOLD, "flate", "huffman-*.golden")))
    assert len(names) == 9
    for p in names:
        data = _read("flate_in", os.path.basename(p)[:-len(".golden")] + ".in")
        assert G.flate_block_huff(data, len(data), 8, G.BLOCK_HUFF_BARE) == _read("flate", os.path.basename(p)), p
        assert DM.block_huff_alone(data, 8) == _read("flate", os.path.basename(p)), p


@needs_deflate
def test_translation_writes_the_references_dynamic_expectations():
    """writeBlockDynamic(indexTokens(tokens), false, input | nil, sync) and flush from a fresh bit writer: the reference's
    TestWriteBlockDynamic / ...Sync, all 34 files, the tokens recovered from the -noinput fixtures as tests/test_stateless_model.py does."""
    seen = set()
    for name in golden_names():
        for mode in ("dyn", "sync"):
            for source in ("dyn", "sync"):
                symbols, _ = tokens_of(_read("flate_dyn", "%s.%s.expect-noinput" % (name, source)))
                words = _tokens(symbols).tok
                f = "%s.%s.expect-noinput" % (name, mode)
                assert G.flate_block_dynamic(words, None, mode == "sync") == _read("flate_dyn", f), (f, source)
                seen.add(f)
                f = "%s.%s.expect" % (name, mode)
                if os.path.exists(os.path.join(GOLD, "flate_dyn", f)):
                    assert G.flate_block_dynamic(words, _read("flate_in", name + ".in"), mode == "sync") == _read("flate_dyn", f), (f, source)
                    seen.add(f)
    assert len(seen) == 34 and seen == set(os.listdir(os.path.join(GOLD, "flate_dyn")))


@needs_deflate
@pytest.mark.parametrize("family", F.FAMILIES)
def test_model_equals_reference(family):
    """Byte for byte (EstimatedBits: the number), every case of the family."""
    model, ref = F.ModelWriter(), F.RefWriter()
    bad, n = [], 0
    for (key, want), (key2, got) in zip(F.records(family, ref), F.records(family, model)):
        assert key == key2
        n += 1
        if want != got:
            bad.append(key)
    assert n >= {"huffman-only": 300, "huffman-only-gzip": 300, "stateless": 150, "stateless-gzip": 150, "estimated-bits": 150}[family.split(".")[0]]
    assert not bad, (len(bad), bad[:10])


@needs_deflate
def test_writer_object_sequences():
    """The Write / Flush / Close sequences that tests/test_gpu_stateless.py::test_writer_objects and tests/test_gpu_deflate.py::
    test_writer_objects expect of the device's writer objects, run on the reference's."""
    data = D.text(70001, 99)
    n = len(data)
    want = SM.stateless_deflate(data[:1000], False) + SM.stateless_deflate(data[1000:], False) + SM.stateless_deflate(b"", True)
    assert G.flate_stateless_writer(data, [1000, n]) == want
    assert G.flate_stateless_writer(b"", []) == bytes([3, 0])
    assert G.flate_stateless(data, True, data[:5000]) == SM.stateless_deflate(data, True, data[:5000])
    body = SM.stateless_deflate(data[:30000], False) + SM.stateless_deflate(data[30000:], False) + bytes([3, 0])
    got = G.gzip_write(G.GZIP_STATELESS, data, [30000, G.WRITE_FLUSH, n, G.WRITE_CLOSE])
    assert got[:10] == SM.GZIP_HEADER and got[10:-8] == body and got[-8:] == struct.pack("<II", zlib.crc32(data), n)
    assert G.gzip_write(G.GZIP_STATELESS, data, [n, G.WRITE_CLOSE]) == SM.gzip_stateless(data)
    assert G.gzip_write(G.GZIP_STATELESS, b"", [G.WRITE_CLOSE]) == SM.gzip_stateless(b"")
    assert G.flate_huffman_only(data, [1000, n, G.WRITE_CLOSE]) == DM.deflate(data)
    assert G.flate_huffman_only(data, [1000, n, G.WRITE_FLUSH]) == DM.deflate(data, end=DM.END_FLUSH)
    assert G.flate_huffman_only(b"", [G.WRITE_CLOSE]) == DM.deflate(b"")
    assert G.gzip_write(G.GZIP_HUFFMAN_ONLY, data, [n, G.WRITE_CLOSE]) == DM.gzip_deflate(data)
    assert G.gzip_write(G.GZIP_HUFFMAN_ONLY, b"", [G.WRITE_CLOSE]) == DM.gzip_deflate(b"")


@needs_deflate
def test_estimated_bits_clamps_at_fifteen():
    """atLeastOne clamps a symbol's cost to [1, 15] bits.  The upper clamp needs a symbol rarer than one in 2^15, which a stateless block
    (at most 30 720 tokens where EstimatedBits is asked) cannot hold: met here with a token list that only indexTokens can build."""
    words = [65] * 65000 + [66]
    assert G.flate_estimated_bits(words) == F.tokens_from_words(words).estimated_bits() == 65000 + 15 + 15


@needs_deflate
def test_no_final_block_streams_as_the_reference_reads_them():
    """writeBlockHuff(eof = true) under a reused table writes no header, so no final bit: the reference's own inflate reads all the bytes
    back and then reports io.ErrUnexpectedEOF."""
    cases = [c for c in S.all_cases() if c[0] in S.NO_FINAL_BLOCK]
    assert len(cases) >= 2
    for c in cases:
        out = G.flate_stateless(c[1], c[2], c[3])
        assert out == S.model(c).data
        got, err, used = G.flate_inflate(out, max_out=len(c[1]) + 64)
        # (all the input is read; what the window still held when the input ran out is not handed out with the error)
        assert c[1].startswith(got) and len(got) >= len(c[1]) - 32768 and (err, used) == (FL_EOF, len(out)), c[0]
        do = zlib.decompressobj(-15)
        assert do.decompress(out) == c[1] and not do.eof and do.unused_data == b"", c[0]


def test_case_set_conditions():
    """Counted with the models' counters (which the comparisons above hold equal to the reference byte for byte): every decision of both
    writers is reached by at least 10 cases of the full set and 3 of the emulator's subset, and the no-final-block shape by two."""
    for cases, floor in ((S.all_cases(), 10), (S.emu_subset(), 3)):
        for name in SM.DECISIONS:
            assert sum(1 for c in cases if S.model(c).counts[name] > 0) >= floor, (name, floor)
    full = D.directed() + D.seeded()
    for cases, floor in ((full, 10), (D.emu_subset(), 3)):
        for name in DM.DECISIONS:
            assert sum(1 for c in cases if D.model(c)[1].counts[name] > 0) >= floor, (name, floor)
    # each tie is present on both sides: the margin the comparison sees, in a case of the full set and of the emulator's
    for cases in (full, D.emu_subset()):
        seen = {m for c in cases if c[0].startswith("tie-") for m in D.model(c)[1].margins}
        assert {("ssize-est", 0), ("ssize-est", 1), ("est-reuse", 0), ("est-reuse", -1)} <= seen, seen
        assert {("abs-max", -2 * 65536), ("abs-max", 0), ("abs-max", 2 * 65536)} <= seen, seen   # (the margin is 65536 * (abs - max))
    for cases in (S.all_cases(), S.emu_subset()):
        seen = {m for c in cases if c[0].startswith("tie-") for m in S.model(c).margins}
        assert {("tokens-15/16", 0), ("tokens-15/16", 1)} <= seen, seen
        # reuse against the doubled estimate of a new table: newSize moves by two for one bit of EstimatedBits, so 1 / 0 (reuse) and
        # -1 / -2 (the new table) are each one bit of EstimatedBits from the other decision
        assert {("dyn-new-reuse", m) for m in (1, 0, -1, -2)} <= seen, seen
    for name in S.NO_FINAL_BLOCK:
        c = next(c for c in S.all_cases() if c[0] == name)
        r = S.model(c)
        assert c[2] and len(r.blocks) >= 2 and r.counts["huffman-only"] == len(r.blocks) and r.counts["first-table"] == 1, name
        assert r.counts["reuse"] == len(r.blocks) - 1 and r.counts["new-table-eob-owed"] == 0 and r.counts["est-stored"] == r.counts["quick-stored"] == 0, name
    assert len(S.NO_FINAL_BLOCK) >= 2 and all(c in S.emu_subset() for c in S.all_cases() if c[0] in S.NO_FINAL_BLOCK)


def test_models_meet_the_committed_reference_digests():
    """The reference's outputs, committed as one digest per family by tests/golden/make_reference_go_golden.py: the gate where
    oracle/_ref did not travel."""
    want = dict(l.split() for l in open(DIGESTS) if l.strip())
    assert sorted(want) == sorted("deflate." + f for f in F.FAMILIES)
    model = F.ModelWriter()
    for f in F.FAMILIES:
        assert F.digest(F.records(f, model)) == want["deflate." + f], f
