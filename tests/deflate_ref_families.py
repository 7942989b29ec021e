"""The outputs of the two DEFLATE writers by family, as a writer gives them: the shared shape behind tests/test_ref_deflate.py (model
against reference, and model against the committed digests) and tests/golden/make_reference_go_golden.py (which writes the digests from
the reference's outputs).

A `writer` is an object with the methods below; ModelWriter answers from tests/deflate_model.py and tests/stateless_model.py, RefWriter
from the translated reference (oracle_goref)."""
import hashlib
import struct
import zlib

import deflate_cases as D
import deflate_model as DM
import stateless_cases as S
import stateless_model as SM

ENDS = (DM.END_CLOSE, DM.END_FLUSH)
OWN = (D.BLOCK, D.PENALTY)   # compressor.init's configuration: what flate.NewWriter(w, HuffmanOnly) and gzip's writer run


def strip_eob(tok):
    return tok[:-1] if tok and tok[-1] == 256 else tok


def tokens_from_words(words):
    """A fresh stateless_model.Tokens indexed from token words, as the reference's indexTokens does it."""
    t = SM.Tokens()
    for w in words:
        if w < SM.MATCH:
            t.add_literals([w])
        else:
            t.add_match((w >> 22) & 0xFF, w & 0xFFFF)
    return t


class ModelWriter:
    def huffman_only(self, data, block, penalty, end):
        return DM.deflate(data, block, penalty, end)

    def huffman_only_gzip(self, data, block, penalty, end):
        return DM.gzip_deflate(data, block, penalty, end)

    def stateless(self, case):
        return S.model(case).data

    def stateless_gzip(self, case):
        return S.model_gzip(case)

    def estimated_bits(self, words):
        return tokens_from_words(words).estimated_bits()


class RefWriter:
    """The translated reference.  A HuffmanOnly case at compressor.init's own (block, penalty) goes through flate.NewWriter / gzip's writer
    AND through the bare bit writer, which must agree; any other (block, penalty) only the bare bit writer can run, and its gzip form is
    gzip's ten header bytes and trailer around it: in the huffman-only-gzip families only the cases at (32768, 10) have their trailer written
    by the reference's gzip.Writer; at the other pairs the family judges the header and the body, and the trailer is CRC-32 / ISIZE by zlib."""

    def __init__(self):
        import oracle_goref as G
        self.G = G

    def huffman_only(self, data, block, penalty, end):
        G = self.G
        out = G.flate_block_huff(data, block, penalty, G.BLOCK_HUFF_CLOSE if end == DM.END_CLOSE else G.BLOCK_HUFF_FLUSH)
        if (block, penalty) == OWN:
            own = G.flate_huffman_only(data, [len(data), G.WRITE_CLOSE if end == DM.END_CLOSE else G.WRITE_FLUSH])
            assert own == out, "flate.NewWriter(HuffmanOnly) and the bare bit writer at (32768, 10) differ"
        return out

    def huffman_only_gzip(self, data, block, penalty, end):
        G = self.G
        if (block, penalty) == OWN:
            return G.gzip_write(G.GZIP_HUFFMAN_ONLY, data, [len(data), G.WRITE_CLOSE if end == DM.END_CLOSE else G.WRITE_FLUSH])
        body = G.gzip_write(G.GZIP_HUFFMAN_ONLY, b"", [0, G.WRITE_FLUSH])[:10] + self.huffman_only(data, block, penalty, end)
        return body if end == DM.END_FLUSH else body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)

    def stateless(self, case):
        return self.G.flate_stateless(case[1], case[2], case[3])

    def stateless_gzip(self, case):
        return self.G.gzip_write(self.G.GZIP_STATELESS, case[1], [len(case[1]), self.G.WRITE_CLOSE])

    def estimated_bits(self, words):
        return self.G.flate_estimated_bits(words)


def records(family, writer):
    """(key, value) per output of a family; a value is bytes or an int."""
    kind, which = family.split(".")
    if kind in ("huffman-only", "huffman-only-gzip"):
        fn = writer.huffman_only if kind == "huffman-only" else writer.huffman_only_gzip
        for c in (D.directed() if which == "directed" else D.seeded()):
            for end in ENDS:   # both endings, whatever the case's own is
                yield "%s/%d" % (c[0], end), fn(c[1], c[2], c[3], end)
    elif kind in ("stateless", "stateless-gzip"):
        fn = writer.stateless if kind == "stateless" else writer.stateless_gzip
        for c in (S.directed() if which == "directed" else S.seeded()):
            yield c[0], fn(c)
    elif kind == "estimated-bits":
        for c in (S.directed() if which == "directed" else S.seeded()):
            for k, t in enumerate(S.model(c).blocks):
                yield "%s/%d" % (c[0], k), writer.estimated_bits(strip_eob(t.tok))
    else:
        raise ValueError(family)


FAMILIES = tuple("%s.%s" % (k, w) for k in ("huffman-only", "huffman-only-gzip", "stateless", "stateless-gzip", "estimated-bits") for w in ("directed", "seeded"))


def digest(recs):
    h = hashlib.sha256()
    for key, val in recs:
        body = val if isinstance(val, bytes) else b"%d" % val
        h.update(b"%s %d %s\n" % (key.encode(), len(body), hashlib.sha256(body).hexdigest().encode()))
    return h.hexdigest()
