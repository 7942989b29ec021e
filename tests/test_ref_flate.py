"""tests/flate_model.py judged by the reference's OWN inflate and gunzip: flate/inflate.go, inflate_gen.go, dict_decoder.go and
gzip/gunzip.go translated statement by statement (oracle/ref_go) and compiled into oracle/_ref/libzstdref.so
(goref_flate_inflate, goref_gunzip).  On every case the emulator and GPU suites use — the directed ones, both sets of mutations,
the seeded structured streams raw and as gzip, the two sweeps, the reference's own vectors and golden streams — the model with
stale_tables=True answers the same (bytes, class, consumed), and for gzip the same header fields.  No case is excluded.

The device's judge is the model with stale_tables=False.  The two modes differ only where rule R6 fired (a symbol read through an
empty table), which a test here asserts on the same cases, together with the shares of verdicts the seeded streams have to reach
by the reference's own count.  Where oracle/_ref is absent, the committed digests of the reference's verdicts
(tests/golden/reference_go_flate_sha256.txt) gate the model instead."""
import collections
import json
import os

import pytest

import flate_cases as FC
import flate_model as M
import oracle_goref as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIGESTS = os.path.join(GOLD, "reference_go_flate_sha256.txt")
needs_flate = pytest.mark.skipif(not G.flate_available(), reason="oracle/_ref/libzstdref.so with the reference's inflate neither present nor buildable")
needs_gunzip = pytest.mark.skipif(not G.gunzip_available(), reason="oracle/_ref/libzstdref.so with the reference's gunzip neither present nor buildable")


def ref(c):
    return G.gunzip(c.data, c.multistream) if c.fmt == "gzip" else G.flate_inflate(c.data, c.dict)


def all_families():
    return FC.families() + [("crc-sweep", FC.crc_sweep()), ("copy-sweep", FC.copy_sweep())]


@pytest.fixture(scope="module")
def families():
    fams = all_families()
    for stale in (True, False):
        FC.warm([c for _, cs in fams for c in cs], stale)
    return dict(fams)


def compare(cs):
    bad = []
    for c in cs:
        want, got = ref(c), FC.verdict(c, True)
        if want != got:
            bad.append((c.name, "reference", len(want[0]), want[1:], "model", len(got[0]), got[1:], sorted(FC.reference_verdict(c)[1])))
        if c.fmt == "gzip":
            hdr = G.gunzip(c.data, c.multistream, want_header=True)[3]
            if hdr != M.gunzip_header(c.data):
                bad.append((c.name, "header", hdr, M.gunzip_header(c.data)))
    assert not bad, (len(bad), bad[:8])


@needs_flate
@pytest.mark.parametrize("family", ["directed", "mut", "generated", "copy-sweep"])
def test_model_equals_reference_inflate(families, family):
    cs = families[family]
    assert len(cs) >= {"directed": 612, "mut": 480, "generated": 2000, "copy-sweep": 192}[family]
    if not G.gunzip_available():
        cs = [c for c in cs if c.fmt == "flate"]
    compare(cs)


@needs_gunzip
@pytest.mark.parametrize("family", ["mutgz", "generated-gz", "crc-sweep"])
def test_model_equals_reference_gunzip(families, family):
    cs = families[family]
    assert len(cs) >= {"mutgz": 480, "generated-gz": 2000, "crc-sweep": 170}[family]
    compare(cs)


@needs_flate
def test_reference_on_its_own_vectors():
    """The rows of tests/golden/flate_vectors.json and the streams of tests/golden/flate/ are the reference's expectations of itself:
    the translated reference meets them, and the model equals it on them."""
    vec = json.load(open(os.path.join(GOLD, "flate_vectors.json")))
    for row in vec["streams"]:
        data = bytes.fromhex(row["stream"])
        out, cls, used = G.flate_inflate(data)
        assert (out, cls, used) == M.inflate(data, stale_tables=True), row["desc"]
        if row["want"] == "fail":
            assert cls in (M.CORRUPT, M.EOF), row["desc"]
        else:
            assert (out, cls) == (bytes.fromhex(row["want"]), M.OK), row["desc"]
    for f in sorted(os.listdir(os.path.join(GOLD, "flate"))):
        data = open(os.path.join(GOLD, "flate", f), "rb").read()
        assert G.flate_inflate(data) == M.inflate(data, stale_tables=True), f
        assert G.flate_inflate(data)[1:] == (M.EOF, len(data)), f
    if not G.gunzip_available():
        return
    for row in vec["gunzip"]:
        data = bytes.fromhex(row["gzip"])
        out, cls, used, hdr = G.gunzip(data, want_header=True)
        assert (out, cls, used, hdr) == M.gunzip(data, want_header=True, stale_tables=True), row["desc"]
        assert cls == row["class"] and out == bytes.fromhex(row["want"]), row["desc"]
        assert (hdr["Name"] if hdr else "") == row["name"], row["desc"]


@needs_flate
def test_generated_streams_are_not_one_sided(families):
    """The shares the seeded streams have to reach, counted on the REFERENCE's verdicts: at least a quarter OK and a quarter not OK,
    every error class, and at least 30 accepted streams that decode through a literal/length code longer than the device's primary
    table (10 bits) and 30 through such a distance code (9 bits; the code-length code's 7 bits are the format's limit)."""
    fams = [("generated", families["generated"])] + ([("generated-gz", families["generated-gz"])] if G.gunzip_available() else [])
    for name, cs in fams:
        got = [ref(c) for c in cs]
        assert all(len(c.data) <= 2048 + (0 if name == "generated" else 3 * 2048 + 2000) and len(r[0]) <= (65536 if name == "generated" else 3 * 65536) for c, r in zip(cs, got))
        n = collections.Counter(r[1] for r in got)
        print(name, dict(n))
        assert n[M.OK] * 4 >= len(cs) and (len(cs) - n[M.OK]) * 4 >= len(cs), (name, n)
        assert n[M.CORRUPT] and n[M.EOF], (name, n)
        if name == "generated-gz":
            assert n[M.HEADER] and n[M.CHECKSUM], n
        else:
            for tag in ("longL", "longD"):
                k = sum(1 for c, r in zip(cs, got) if r[1] == M.OK and tag in c.name.split("/", 2)[2].split("+"))
                assert k >= 30, (tag, k)
    first = families["generated"][:480]   # the emulator's share holds the stale shapes and the long codes too
    for tag in ("stale-dist", "stale-lit", "stale-clen"):
        assert sum(1 for c in first if tag in c.name) == 60
    for tag in ("longL", "longD"):
        assert sum(1 for c in first if tag in c.name.split("/", 2)[2].split("+") and ref(c)[1] == M.OK) >= 30, tag


def test_two_modes_differ_only_where_r6_fired(families):
    """stale_tables=False (the device's judge) and stale_tables=True (the reference) answer the same wherever no symbol was read
    through an empty table; R6 fires for each of the three tables, and on some inputs of each the answers do differ."""
    differ = collections.Counter()
    fired = collections.Counter()
    for name, cs in families.items():
        for c in cs:
            v, rules = FC.reference_verdict(c)
            if "R6" not in rules:
                assert FC.verdict(c) == v, c.name
                continue
            for t in ("dist", "lit", "clen"):
                if "stale-" + t in c.name:
                    fired[t] += 1
                    differ[t] += FC.verdict(c) != v
            assert FC.verdict(c)[1] != M.OK, c.name   # the device's reading: a symbol through an empty table is an error
    print("R6 fired", dict(fired), "answers differ", dict(differ))
    assert all(fired[t] >= 60 for t in ("dist", "lit", "clen")), fired
    assert all(differ[t] > 0 for t in ("dist", "lit", "clen")), differ


def test_model_meets_the_committed_reference_digests(families):
    """The reference's verdicts, committed as one digest per family by tests/golden/make_reference_go_golden.py: the gate where
    oracle/_ref did not travel."""
    want = dict(l.split() for l in open(DIGESTS) if l.strip())
    assert sorted(want) == sorted("flate." + n for n, _ in FC.families())
    for name, cs in FC.families():
        assert FC.family_digest(cs, lambda c: FC.verdict(c, True)) == want["flate." + name], name
