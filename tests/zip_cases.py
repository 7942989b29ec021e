"""The inputs of the zip suites (tests/test_zip_model.py, test_emu_zip.py, test_gpu_zip.py): the reference's own fixtures
(tests/golden/zip), hand-built archives with one case per return of the member rules and the directory rules (tests/zip_builder.py),
the stored-member shapes, and 480 seeded mutations of a 12-member archive.  A case is a buffer and a member table: the table the
model's directory pass reads from the buffer, or one given by hand (offsets past the end, buffers cut short, two archives in one
buffer).  `rule` is the return of tests/zip_model.member that the case's member `focus` is built to land on."""
import collections
import json
import os
import random
import struct
import zlib

import flate_cases as FC
import zip_builder as B
import zip_model as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zip")
Case = collections.namedtuple("Case", "name data members rule focus dir_cls")

# every return of zip_model.member
ALL_RULES = {"1-readat", "1-format", "2-format", "2-ok", "3", "8", "5-format", "5-corrupt", "5-eof", "5-short", "6-absent", "6-short", "6-field",
             "6-hash", "6-ok", "7-hash", "7-ok", "7-unset"}


def text(n, seed=1):
    rng = random.Random(seed)
    words = [b"the", b"wave", b"reads", b"one", b"member", b"of", b"an", b"archive", b"and", b"checks", b"its", b"sum", b"zip", b"deflate", b"stored"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b"\n" if rng.random() < 0.1 else b" ")
    return bytes(out[:n])


def C(name, data, members=None, rule=None, focus=0, dir_cls=Z.OK):
    return Case(name, bytes(data), members, rule, focus, dir_cls)


def members_of(c):
    """The member table of a case: its own, or the directory's as the model reads it ([] where the directory is refused)."""
    if c.members is not None:
        return c.members
    cls, d = Z.directory(c.data)
    return [Z.member_of(e) for e in d.files] if cls == Z.OK else []


def arch(name, ms, rule, focus=0, dir_cls=Z.OK, **kw):
    return C(name, B.build(ms, **kw)[0], None, rule, focus, dir_cls)


def one(name, m, rule, cut=None, offset=None):
    """A buffer that is one local record (cut: its first `cut` bytes) and a table of one member at `offset` (default 0)."""
    buf = m.local()
    if cut is not None:
        buf = buf[:cut]
    mem = Z.Member(0 if offset is None else offset, m.csize, m.usize, m.crc, m.method, m.flags, m.name.endswith(b"/"))
    return C(name, buf, [mem], rule)


def _r3():
    """A fixed block whose input ends where the extra bit of a length should be: six 9-bit literals and the symbol 265, 64 bits."""
    bw = FC.BW()
    FC.fixed_block(bw, [200] * 6 + [("sym", 265)], eob=False)
    assert len(bw.bytes()) == 8
    return bw.bytes(), bytes([200] * 6)


def _cut_stored(total, have):
    """A stored block of `total` bytes of which the input holds `have`."""
    bw = FC.BW()
    FC.stored_block(bw, bytes(range(97, 97 + 26)) * 8, final=True)
    full = bw.bytes()
    return full[:1] + struct.pack("<HH", total, total ^ 0xFFFF) + full[5:5 + have]


def header_cases():
    t = text(300)
    cs = []
    m = B.M("a.txt", t)
    cs.append(one("hdr/past-the-end", m, "1-readat", offset=len(m.local()) - 10))
    cs.append(one("hdr/negative-offset", m, "1-readat", offset=-1))
    cs.append(one("hdr/cut-at-29", m, "1-readat", cut=29))
    cs.append(one("hdr/whole-30", B.M("", b"", method=0), "7-unset", cut=30))
    cs.append(one("hdr/wrong-signature", B.M("a.txt", t, local_sig=b"PK\x03\x05"), "1-format"))
    cs.append(arch("hdr/local-name-and-extra-differ", [B.M("a.txt", t, local_name=b"a-longer-name.txt", local_extra=b"\x99\x99\x02\x00xy")], "7-ok"))
    cs.append(arch("dir/size-0-csize-2", [B.M("d/", b"", body=b"\x03\x00")], "2-ok"))
    cs.append(arch("dir/size-1", [B.M("d/", b"x", method=0)], "2-format"))
    cs.append(one("dir/header-past-the-end", B.M("d/", b""), "1-readat", cut=20))   # rule 1 runs first
    for meth in (1, 9, 93):
        cs.append(arch("method/%d" % meth, [B.M("a.txt", t, method=meth, body=t)], "3"))
    cs.append(arch("prefix/junk", [B.M("a.txt", t), B.M("b.txt", t[:50], method=0)], "7-ok", focus=1, prefix=b"junk" * 25))
    two = [B.M("a.txt", t), B.M("b.txt", t[:50], method=0)]
    true_size = sum(len(m.central(0)) for m in two)
    cs.append(arch("prefix/valid-header-at-0", two, "7-ok", focus=1, dsize=true_size - 10))   # baseOffset would be 10
    cs.append(arch("end/fake-record-in-comment", [B.M("a.txt", t)], None, comment=B.end_record(0, 0, 0)))
    cs.append(arch("end/comment", [B.M("a.txt", t)], "7-ok", comment=b"an archive comment"))
    cs.append(arch("end/comment-cut", [B.M("a.txt", t)], None, dir_cls=Z.FORMAT, comment=b"short", comment_len=9))
    cs.append(arch("end/trailing-junk", [B.M("a.txt", t)], None, dir_cls=Z.FORMAT, junk=b"\0" * 70000))
    cs.append(arch("count/plus-65536", [B.M("a.txt", t), B.M("b.txt", t)], "7-ok", zip64=True, records=2 + 65536))
    # the header read that ends the directory meets the end record: 22 bytes are a short read, with a comment of 24 a wrong signature
    cs.append(arch("count/plus-1", [B.M("a.txt", t), B.M("b.txt", t)], None, dir_cls=Z.DIR_EOF, records=3))
    cs.append(arch("count/plus-1-long-comment", [B.M("a.txt", t), B.M("b.txt", t)], None, dir_cls=Z.FORMAT, records=3, comment=b"c" * 24))
    cs.append(arch("count/minus-1", [B.M("a.txt", t), B.M("b.txt", t)], None, dir_cls=Z.DIR_EOF, records=1))
    cs.append(C("end/none", b"PK\x03\x04" + bytes(100), None, None, 0, Z.FORMAT))
    cs.append(C("end/empty-buffer", b"", None, None, 0, Z.FORMAT))
    cs.append(arch("end/zip64", [B.M("a.txt", t)], "7-ok", zip64=True))
    a64 = B.build([B.M("a.txt", t)], zip64=True)[0]
    p = a64.rindex(b"PK\x06\x07")
    cs.append(C("end/zip64-record-past-the-end", a64[:p + 8] + struct.pack("<Q", len(a64) - 40) + a64[p + 16:], None, None, 0, Z.DIR_EOF))
    cs.append(C("end/zip64-record-wrong-signature", a64.replace(b"PK\x06\x06", b"PK\x06\x05"), None, None, 0, Z.FORMAT))
    cs.append(C("end/directory-to-the-last-byte", _dir_to_end(t), None, None, 0, Z.DIR_EOF))
    body = B.deflate(t)
    cs.append(arch("zip64/extra-complete", [B.M("a.txt", t, raw32=(B.U32, B.U32, B.U32), extra=B.zip64_extra(len(t), len(body), 0))], "7-ok"))
    cs.append(arch("zip64/extra-7-short", [B.M("a.txt", t, raw32=(B.U32, B.U32, 0), extra=struct.pack("<HH", 1, 9) + struct.pack("<Q", len(t)) + b"\0")], None,
                   dir_cls=Z.FORMAT))
    cs.append(arch("zip64/extra-not-consulted", [B.M("a.txt", t, extra=B.zip64_extra(12345, 678, 9))], "7-ok"))
    cs.append(arch("zip64/usize-maxed-no-extra", [B.M("a.txt", t, raw32=(len(body), B.U32, 0))], "8"))
    cs.append(arch("zip64/csize-maxed-no-extra", [B.M("a.txt", t, raw32=(B.U32, len(t), 0))], None, dir_cls=Z.FORMAT))
    cs.append(arch("name/utf8-flag", [B.M("h\xe9.txt".encode("utf-8"), t, flags=0x800), B.M("h\xe9.txt".encode("utf-8"), t), B.M(b"h\xe9.txt", t, flags=0x800),
                                      B.M("plain.txt", t, comment=b"back\\slash")], "7-ok"))
    a, _ = B.build([B.M("a1.txt", t), B.M("a2.txt", t[:100], method=0)])
    b, _ = B.build([B.M("b1.txt", t[::-1]), B.M("b/", b"")], comment=b"second")
    ma = [Z.member_of(e) for e in Z.directory(a)[1].files]
    mb = [Z.member_of(e)._replace(header_offset=e.header_offset + len(a)) for e in Z.directory(b)[1].files]
    cs.append(C("merged/two-archives", a + b, ma + mb, "7-ok", 2))
    return cs


def _dir_to_end(t):
    """A directory whose second header's name, extra and comment lengths reach exactly the archive's last byte: the next read is io.EOF."""
    a, _ = B.build([B.M("a.txt", t), B.M("b.txt", t[:10], method=0)])
    p = a.rindex(b"PK\x01\x02")
    rest = len(a) - (p + 46)
    return a[:p + 28] + struct.pack("<HHH", 5, 0, rest - 5) + a[p + 34:]


def size_cases():
    t = text(1000, 2)
    r3, r3_out = _r3()
    cs = []
    for meth, tag in ((0, "stored"), (8, "deflated")):
        cs.append(arch("size/%s-one-too-small" % tag, [B.M("a", t, method=meth, usize=len(t) - 1)], "5-format"))
        cs.append(arch("size/%s-one-too-large" % tag, [B.M("a", t, method=meth, usize=len(t) + 1)], "5-short"))
    cs.append(arch("cap/literal", [B.M("a", b"abc", usize=2)], "5-format"))
    cs.append(arch("cap/match", [B.M("a", b"a" * 10, usize=9)], "5-format"))
    cs.append(arch("cap/match-far-over", [B.M("a", b"ab" * 200, usize=5)], "5-format"))
    cs.append(arch("cap/stored-block", [B.M("a", t, level=0, usize=len(t) - 1)], "5-format"))
    cs.append(arch("cap/then-corrupt", [B.M("a", b"abc", body=B.deflate(b"abc")[:-1] + b"\xff\xff", usize=1)], "5-format"))
    for usize, rule in ((40, "5-format"), (49, "5-format"), (50, "5-eof"), (60, "5-eof"), (100, "5-eof")):
        cs.append(one("cap/cut-stored-block-50-of-100-stated-%d" % usize, B.M("a", b"", body=_cut_stored(100, 50), usize=usize, crc=0), rule))
    cs.append(arch("csize/one-short", [B.M("a", t, body=B.deflate(t)[:-1])], "5-eof"))
    cs.append(arch("csize/trailing-garbage", [B.M("a", t, body=B.deflate(t) + b"garbage")], "7-ok"))
    m = B.M("a", t)
    cs.append(one("csize/clipped-by-the-end-deflated", m, "5-eof", cut=len(m.local()) - 8))
    cs.append(one("csize/clipped-by-the-end-inside-extra-bits", m, "5-short", cut=len(m.local()) - 7))   # rule R3 of tests/flate_model.py
    m = B.M("a", t, method=0)
    cs.append(one("csize/clipped-by-the-end-stored", m, "5-short", cut=len(m.local()) - 7))
    cs.append(one("csize/body-past-the-end", B.M("a", t, method=0, local_name=b"n" * 40), "5-short", cut=50))
    cs.append(arch("r3/size-matches", [B.M("a", r3_out, body=r3)], "7-ok"))
    cs.append(arch("r3/size-differs", [B.M("a", r3_out, body=r3, usize=7)], "5-short"))
    cs.append(arch("bomb/corrupt", [B.M("a", b"", body=b"\x07", usize=1000000)], "5-corrupt"))
    cs.append(arch("bomb/truncated", [B.M("a", b"", body=B.deflate(t)[:5], usize=1000000)], "5-eof"))
    cs.append(arch("bomb/at-the-bound", [B.M("a", b"", body=b"\x07", usize=2064)], "5-corrupt"))
    cs.append(arch("limit/usize", [B.M("a", t, raw32=(10, (1 << 30) + 1, 0))], "8"))
    cs.append(arch("limit/csize", [B.M("a", t, method=0, raw32=((1 << 30) + 1, 10, 0))], "8"))
    cs.append(arch("crc/wrong", [B.M("a", t, crc=zlib.crc32(t) ^ 1)], "7-hash"))
    cs.append(arch("crc/wrong-stored", [B.M("a", t, method=0, crc=zlib.crc32(t) ^ 0x80000000)], "7-hash"))
    cs.append(arch("crc/zero-and-unchecked", [B.M("a", t, crc=0)], "7-unset"))
    body, crc = B.deflate(t), zlib.crc32(t)
    d = B.descriptor(crc, len(body), len(t))
    cs.append(arch("dd/with-signature", [B.M("a", t, flags=8, trailer=d)], "6-ok"))
    cs.append(arch("dd/without-signature", [B.M("a", t, flags=8, trailer=d[4:])], "6-ok"))
    cs.append(arch("dd/stored", [B.M("a", t, method=0, flags=8, trailer=B.descriptor(crc, len(t), len(t)))], "6-ok"))
    cs.append(arch("dd/wrong-crc-field", [B.M("a", t, flags=8, trailer=B.descriptor(crc ^ 4, len(body), len(t)))], "6-field"))
    cs.append(arch("dd/the-directory-in-its-place", [B.M("a", t, flags=8)], "6-field"))
    cs.append(arch("dd/wrong-content", [B.M("a", t, flags=8, crc=crc ^ 2, trailer=B.descriptor(crc ^ 2, len(body), len(t)))], "6-hash"))
    cs.append(arch("dd/crc-zero-is-checked", [B.M("a", t, flags=8, crc=0, trailer=B.descriptor(0, len(body), len(t)))], "6-hash"))
    m = B.M("a", t, flags=8, trailer=d)
    n = len(m.local())
    cs.append(one("dd/missing", m, "6-absent", cut=n - 16))
    cs.append(one("dd/cut-at-3", m, "6-absent", cut=n - 13))
    cs.append(one("dd/cut-at-11", m, "6-short", cut=n - 5))
    cs.append(one("dd/cut-at-15", m, "6-short", cut=n - 1))
    cs.append(one("dd/without-signature-cut-at-11", B.M("a", t, flags=8, trailer=d[4:]), "6-short", cut=n - 4 - 1))
    cs.append(one("dd/short-size-wins", B.M("a", t, flags=8, usize=len(t) + 1), "5-short"))
    return cs


STORED_SIZES = (0, 1, 63, 64, 65, 65535, 65536, 65537, 131072, 3 * 65536 + 5)


def stored_cases(full):
    """Stored members of every size x name lengths 1 to 8 (the body start sweeps every alignment modulo 8); without `full` the
    sizes above 65 take one name length each.  One archive; the last two members are twins of the largest with a wrong CRC."""
    ms = []
    for k, size in enumerate(STORED_SIZES):
        data = text(size, 100 + k)
        for nl in (range(1, 9) if full or size <= 65 else (k % 8 + 1,)):
            ms.append(B.M("n" * nl, data, method=0))
    big = text(STORED_SIZES[-1], 7)
    ms.append(B.M("twin-1", big, method=0, crc=zlib.crc32(big) ^ 1))
    ms.append(B.M("twin-2", big[:70000], method=0, crc=zlib.crc32(big[:70001])))
    data, _ = B.build(ms)
    return C("stored/shapes" + ("-full" if full else ""), data, None, "7-hash", len(ms) - 1)


def base_archive():
    """The 12 members the mutations start from."""
    rng = random.Random(12)
    ms = []
    for i in range(12):
        t = text(rng.choice([0, 40, 300, 900, 2500]) if i else 700, 50 + i)
        meth = 0 if i % 3 == 2 else 8
        kw = {}
        if i % 4 == 1:
            body = B.deflate(t) if meth == 8 else t
            kw = {"flags": 8, "trailer": B.descriptor(zlib.crc32(t), len(body), len(t), sig=i % 8 == 1)}
        if i == 6:
            ms.append(B.M("dir/", b""))
            continue
        if i == 9:
            kw["comment"] = "caf\xe9".encode("utf-8")
        ms.append(B.M("m%02d%s.txt" % (i, "x" * (i % 5)), t, method=meth, level=rng.choice([1, 6, 9]), **kw))
    return B.build(ms, comment=b"twelve")


def mutations(n=480, seed=0x21B):
    data, offs = base_archive()
    cd = data.index(b"PK\x01\x02")
    rng = random.Random(seed)
    out = []
    for k in range(n):
        b = bytearray(data)
        where = rng.choice(["dir", "dir", "local", "body", "end"])
        for _ in range(rng.choice([1, 1, 2])):
            if where == "dir":
                p = rng.randrange(cd, len(b) - 22 - 6)
            elif where == "end":
                p = rng.randrange(len(b) - 22 - 6, len(b))
            elif where == "local":
                p = rng.choice(offs) + rng.randrange(30)
            else:
                p = rng.randrange(0, cd)
            if rng.random() < 0.5:
                b[p] ^= 1 << rng.randrange(8)
            else:
                b[p] = rng.choice([0, 1, 8, 0xFF, rng.getrandbits(8)])
        if rng.random() < 0.05:
            b = b[:rng.randrange(len(b) - 40, len(b))]
        out.append(C("mut/%03d-%s" % (k, where), b))
    return out


def fixtures():
    """The reference's own archives (zip/testdata) with what the table of zip/reader_test.go states about them."""
    exp = json.load(open(os.path.join(GOLDEN, "expect.json")))
    return [(name, open(os.path.join(GOLDEN, name), "rb").read(), e) for name, e in sorted(exp.items())]


def fixture_cases():
    return [C("fixture/" + name, data) for name, data, _ in fixtures()]


def directed():
    return header_cases() + size_cases()


def merged(cases):
    """The buffers of `cases` laid end to end and their member tables as ONE table, the offsets moved along: one batch.  What a
    member reads behind its own buffer's end is now the next case's bytes, so the model judges the merged buffer as it is."""
    buf, members, at = bytearray(), [], 0
    for c in cases:
        members += [m._replace(header_offset=m.header_offset + at) for m in members_of(c)]
        buf += c.data
        at = len(buf)
    return bytes(buf), members


def many_small(n=2048, size=4096):
    """One archive of n members of `size` bytes of seeded text, deflated by CPython at levels 1, 6 and 9 in turn -> (archive, contents)."""
    contents = [text(size, 1000 + i) for i in range(n)]
    ms = [B.M("t/%04d.txt" % i, t, level=(1, 6, 9)[i % 3]) for i, t in enumerate(contents)]
    return B.build(ms)[0], contents
