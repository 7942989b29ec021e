"""Hand-built frames (tests/zstd_frame_cases.py) for the shapes of the zstd format that no fixture archive and no encoder here emits.

  * the builder against the decoders: the reference's own DecodeAll (translated: oracle_goref.zstd_decode_all) and the oracle's decoder
    return the plaintext of the builder's executor on every `valid` case (the two decoders are the independent ones: the plaintext is
    the executor's by construction); the reference refuses every `refused` case; its verdicts on the `judge` cases are printed and held
    in profiles/zstd_decode_shapes.md, and where it returns bytes there the oracle returns the same;
  * a coverage statement in the style of test_outcome_coverage.py: which shapes the valid cases reach, by a header-level walker and the
    oracle's inspection hook;
  * the DecodeAll kernels on the CPU wave emulator (kcemu_zstd_decode_all) on all cases as one batch, in both orders."""
import collections
import ctypes as C
import os
import re

import pytest

import zstd_frame_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERDICTS = os.path.join(ROOT, "profiles", "zstd_decode_shapes.md")


@pytest.fixture(scope="module")
def G():
    import oracle_goref
    if not oracle_goref.available():
        pytest.skip("oracle/_ref/libzstdref.so (the translated reference decoder) is not built")
    return oracle_goref


def test_builder_against_three_decoders(G, oracle):
    cs = zc.cases()
    wrong, verdicts = [], []
    for c in cs:
        ref, err = zc.reference(G, c)
        if c.expect == "valid":
            if ref != c.plain:
                wrong.append("%s: the reference gives %s" % (c.name, err if ref is None else "%d other bytes" % len(ref)))
            try:
                o = oracle.zstd_decode(c.data, len(c.plain) + 64, dict_content=zc.DICTS[c.dicts[0]] if c.dicts else None)
            except Exception as e:  # the oracle's decoder reports a refusal by raising
                o = repr(e)
            if o != c.plain:
                wrong.append("%s: the oracle's decoder gives %s" % (c.name, o if isinstance(o, str) else "%d other bytes" % len(o)))
        elif c.expect == "refused":
            if ref is not None:
                wrong.append("%s: the reference accepts it (%d bytes)" % (c.name, len(ref)))
            elif c.cls is not None and zc.message_class(err) != c.cls:
                wrong.append("%s: the reference's message is not of class %s: %s" % (c.name, c.cls, err))
        else:
            verdicts.append((c.name, "returns %d bytes" % len(ref) if ref is not None else "refuses: " + err))
            if ref is not None:  # the oracle restates the reference: the same bytes where the reference decides for the frame
                try:
                    o = oracle.zstd_decode(c.data, len(ref) + 64, dict_content=zc.DICTS[c.dicts[0]] if c.dicts else None)
                except Exception as e:
                    o = repr(e)
                if o != ref:
                    wrong.append("%s: the reference returns %d bytes, the oracle's decoder gives %s" % (c.name, len(ref), o if isinstance(o, str) else "%d other bytes" % len(o)))
    assert not wrong, "\n".join(wrong)
    print("\nthe reference's verdicts on the judge cases:")
    for name, v in verdicts:
        print("  %-70s %s" % (name, v))
    # the list in profiles/zstd_decode_shapes.md is this one
    lines = ["| %s | %s |" % (name, v.replace("|", "/")) for name, v in verdicts]
    text = open(VERDICTS).read()
    a, b = text.index("<!-- verdicts -->"), text.index("<!-- /verdicts -->")
    new = text[:a] + "<!-- verdicts -->\n| case | the reference's DecodeAll |\n|---|---|\n" + "\n".join(lines) + "\n" + text[b:]
    if new != text and os.environ.get("KC_WRITE_PROFILES", "") == "1":
        open(VERDICTS, "w").write(new)
    assert new == text, "profiles/zstd_decode_shapes.md does not hold the verdict list above (KC_WRITE_PROFILES=1 rewrites it)"
    n = collections.Counter(c.expect for c in cs)
    assert n["valid"] >= 100 and n["refused"] >= 30 and n["judge"] >= 10, dict(n)


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def walk(data, cov):
    """Header-level walker over well-formed frames: frame header fields, block types, literal section types and size formats, how the
    Huffman weights are coded, sequence-count classes and the mode of each sequence table.  Nothing is decoded."""
    p = 0
    while p < len(data):
        magic = int.from_bytes(data[p:p + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            cov["frame:skippable"] += 1
            p += 8 + int.from_bytes(data[p + 4:p + 8], "little")
            continue
        assert magic == 0xFD2FB528
        fhd = data[p + 4]
        p += 5
        single, fcs_flag, did_flag = (fhd >> 5) & 1, fhd >> 6, fhd & 3
        window = None
        if not single:
            window = (1 << (10 + (data[p] >> 3))) // 8 * (8 + (data[p] & 7))
            cov["window:descriptor"] += 1
            if data[p] & 7:
                cov["window:mantissa"] += 1
            p += 1
        did = [0, 1, 2, 4][did_flag]
        cov["dictionary id:%d bytes" % did] += 1
        p += did
        fcs = [1 if single else 0, 2, 4, 8][fcs_flag]
        cov["fcs:%d bytes" % fcs] += 1
        if single:
            size = int.from_bytes(data[p:p + fcs], "little") + (256 if fcs == 2 else 0)
            window = max(size, 1024) if size < 1024 else size
        p += fcs
        if window < 128 << 10:
            cov["window:below 128 KiB"] += 1
        if fhd & 4:
            cov["frame:checksum"] += 1
        while True:
            bh = int.from_bytes(data[p:p + 3], "little")
            p += 3
            btype, size = (bh >> 1) & 3, bh >> 3
            cov["block:" + ("raw", "rle", "compressed")[btype]] += 1
            if btype == 2:
                _walk_block(data[p:p + size], cov)
            p += 1 if btype == 1 else size
            if bh & 1:
                break
        if fhd & 4:
            p += 4


def _walk_block(b, cov):
    ltype, sf = b[0] & 3, (b[0] >> 2) & 3
    kind = ("raw", "rle", "compressed", "treeless")[ltype]
    if ltype < 2:
        hdr = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = int.from_bytes(b[:hdr], "little") >> (3 if hdr == 1 else 4)
        cov["literals:%s, %d-byte header" % (kind, hdr)] += 1
        q = hdr + (regen if ltype == 0 else 1)
    else:
        hdr = 3 if sf < 2 else 4 if sf == 2 else 5
        v = int.from_bytes(b[:hdr], "little")
        bits = 10 if sf < 2 else 14 if sf == 2 else 18
        comp = (v >> (4 + bits)) & ((1 << bits) - 1)
        cov["literals:%s, size format %d" % (kind, sf)] += 1
        cov["literals:%d stream%s" % ((1, "") if sf == 0 else (4, "s"))] += 1
        if ltype == 2:
            if b[hdr] >= 128:
                cov["weights:direct"] += 1
            else:
                cov["weights:fse, table log %d" % ((b[hdr + 1] & 15) + 5)] += 1
        q = hdr + comp
    n = b[q]
    q += 1
    if n >= 128:
        n, q = (((n - 128) << 8) + b[q], q + 1) if n < 255 else (b[q] + (b[q + 1] << 8) + 0x7F00, q + 2)
    cov["nseq:" + ("0" if n == 0 else "<128" if n < 128 else "<32512" if n < 0x7F00 else ">=32512")] += 1
    if n:
        for k, shift in (("ll", 6), ("of", 4), ("ml", 2)):
            cov["%s:%s" % (k, ("predefined", "rle", "compressed", "repeat")[(b[q] >> shift) & 3])] += 1


def test_valid_cases_reach_these_shapes(oracle):
    L = oracle.lib()
    L.kco_zstd_inspect.restype = C.c_int64
    L.kco_zstd_inspect.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    buf = C.create_string_buffer(1 << 20)
    cov = collections.Counter()
    for c in zc.cases():
        if c.expect != "valid":
            continue
        walk(c.data, cov)
        if c.dicts or c.name.startswith("two frames"):
            continue  # the inspection hook takes one frame and no dictionary
        assert L.kco_zstd_inspect(c.data, len(c.data), buf, len(buf)) >= 0, c.name
        m = re.search(r"REP1=(\d+) REP2=(\d+) REP3=(\d+) offset codes LOW=(\d+) HIGH=(\d+)", buf.value.decode())
        for k, name in enumerate(("repcode:1", "repcode:2", "repcode:3", "offset code:<=24", "offset code:>24")):
            cov[name] += int(m.group(k + 1))
    want = {"block:raw", "block:rle", "block:compressed", "frame:skippable", "frame:checksum", "window:below 128 KiB", "window:mantissa",
            "weights:direct", "weights:fse, table log 5", "weights:fse, table log 6", "weights:fse, table log 7", "literals:1 stream", "literals:4 streams",
            "nseq:0", "nseq:<128", "nseq:<32512", "nseq:>=32512", "repcode:1", "repcode:2", "repcode:3", "offset code:<=24", "offset code:>24"}
    want |= {"literals:%s, %d-byte header" % (k, h) for k in ("raw", "rle") for h in (1, 2, 3)}
    want |= {"literals:%s, size format %d" % (k, sf) for k in ("compressed", "treeless") for sf in (0, 1, 2, 3)}
    want |= {"%s:%s" % (k, m) for k in ("ll", "of", "ml") for m in ("predefined", "rle", "compressed", "repeat")}
    want |= {"fcs:%d bytes" % n for n in (0, 1, 2, 4, 8)} | {"dictionary id:%d bytes" % n for n in (0, 1, 2, 4)}
    missing = sorted(w for w in want if cov[w] == 0)
    assert not missing, (missing, dict(cov))
    # Left out, and why:
    #   weights:fse, table log 8 and above - judge cases, not valid ones: the format's limit for the weights is 6, the reference takes up to 15


# ---- the emulator --------------------------------------------------------------------------------------------------------------
def test_emulator_judged_by_the_reference(G):
    """Every case through kcemu_zstd_decode_all as one batch, in the listed order and reversed: the reference's bytes with status 0, or
    a status and an empty range; guard bytes intact (checked by the runner)."""
    cs = [c for c in zc.cases() if zc.full() or not c.big]
    refs = [zc.reference(G, c) for c in cs]
    dicts = [zc.raw_dict_blob(i, d) for i, d in zc.DICTS.items()]
    cap = sum(len(r) for r, _ in refs if r is not None)
    for order in (1, -1):
        outs, status = zc.emu_decode_all([c.data for c in cs][::order], cap, dicts=dicts)
        wrong = zc.judge(cs[::order], refs[::order], outs, status)
        assert not wrong, "%s order:\n%s" % ("listed" if order == 1 else "reversed", "\n".join(wrong))
        for c, (_, err), s in zip(cs[::order], refs[::order], status):
            if c.cls is not None:  # the directed refusals: the class of the status is the class of the reference's message
                assert zc.NAMES[int(s)] == c.cls == zc.message_class(err), (c.name, zc.NAMES[int(s)], err)
