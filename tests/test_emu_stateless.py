"""The stateless writers' kernels and host sequence (compress_amd/csrc/kc_flate_stateless.hip, kc_stateless_host.h) on the wave emulator
against the model (tests/stateless_model.py): bytes, out_off, the bound and the decision counters, one call per option set with all
its inputs mixed in one batch, behind 0xA5 guards on both sides of a dst that is not word-aligned."""
import pytest

import emu_lib
import stateless_cases as S
import stateless_model as M

CASES = S.emu_subset()


def groups(cases):
    g = {}
    for c in cases:
        g.setdefault((c[2], c[3]), []).append(c)
    return g


GROUPS = groups(CASES)
KEYS = sorted(GROUPS, key=lambda k: (not k[0], len(k[1]), k[1]))


def check_group(cs, eof, dic, cap=None):
    rc, outs, out_off, counts = S.emu_stateless([c[1] for c in cs], False, eof, dic, cap=cap)
    assert rc == 0
    at = 0
    for i, c in enumerate(cs):
        want = S.model(c).data
        assert outs[i] == want, (c[0], len(outs[i]), len(want))
        assert int(out_off[i]) == at
        at += len(want)
        assert len(want) <= M.bound(len(c[1]), len(dic))
    assert int(out_off[len(cs)]) == at
    want_counts = {k: sum(S.model(c).counts[k] for c in cs) for k in S.COUNT_NAMES}
    assert counts == want_counts
    return at


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "%s-dict%d" % ("eof" if k[0] else "open", len(k[1])))
def test_emulator_equals_model(key):
    check_group(GROUPS[key], key[0], key[1])


def test_every_decision_is_met_on_the_emulator():
    tot = dict.fromkeys(S.COUNT_NAMES, 0)
    for key in KEYS:
        for c in GROUPS[key]:
            for k in tot:
                tot[k] += S.model(c).counts[k]
    assert all(tot[k] > 0 for k in M.DECISIONS), tot


def test_gzip_form():
    cs = [c for c in CASES if len(c[1]) <= 3000][::2] + [c for c in CASES if c[0] in ("cut-32768-text", "shifted-alphabet-0")]
    rc, outs, out_off, _ = S.emu_stateless([c[1] for c in cs], True)
    assert rc == 0
    for c, out in zip(cs, outs):
        assert out == S.model_gzip(c), c[0]
        assert len(out) <= M.bound(len(c[1])) + 20


def test_exact_capacity_and_one_byte_less():
    cs = [c for c in GROUPS[(True, b"")] if len(c[1]) <= 1000]
    total = sum(len(S.model(c).data) for c in cs)
    assert check_group(cs, True, b"", cap=total) == total          # the exact total is enough
    rc, outs, out_off, _ = S.emu_stateless([c[1] for c in cs], False, True, b"", cap=total - 1)
    assert rc == -2 and outs is None                               # KC_ERR_DST_TOO_SMALL, nothing written (emu_stateless checks every byte)
    assert int(out_off[len(cs)]) == total                          # ... and the layout says what it takes


def test_empty_batch_and_empty_inputs():
    rc, outs, out_off, _ = S.emu_stateless([])
    assert rc == 0 and outs == [] and int(out_off[0]) == 0
    rc, outs, _, _ = S.emu_stateless([b"", b"", b"x", b""])
    assert rc == 0 and outs == [M.stateless_deflate(d) for d in (b"", b"", b"x", b"")]
    rc, outs, _, _ = S.emu_stateless([b"", b"x" * 20, b""], eof=False)
    assert rc == 0 and outs == [M.stateless_deflate(d, False) for d in (b"", b"x" * 20, b"")]
    rc, outs, _, _ = S.emu_stateless([b"", b"x"], gzip=True)
    assert rc == 0 and outs == [M.gzip_stateless(d) for d in (b"", b"x")]


def test_dictionary_longer_than_8192_is_its_tail():
    d = S.text(9000, 5)
    data = [S.text(500, 8000), d[-40:] + S.text(30, 1)]
    rc, outs, _, _ = S.emu_stateless(data, False, True, d)
    assert rc == 0 and outs == [M.stateless_deflate(x, True, d[-8192:]) for x in data]


def test_scratch_budget_cuts_the_batch():
    """A budget of a few blocks' records and tokens: the call is cut into groups of inputs, runs match, plan and chain twice per group
    and writes the same bytes; the counters are read after the first pass, so every block counts once."""
    cs = [c for c in GROUPS[(True, b"")] if 5000 <= len(c[1]) <= 70000][:6]
    assert len(cs) >= 4
    with emu_lib.scratch_budget(700 * 1024):
        rc, outs, out_off, counts = S.emu_stateless([c[1] for c in cs])
        batches = emu_lib.last_batches()
    assert rc == 0 and batches > 1
    assert outs == [S.model(c).data for c in cs]
    need = emu_lib.last_max_need()
    with emu_lib.scratch_budget(need):  # the least budget that refuses nothing ...
        rc, outs, _, _ = S.emu_stateless([c[1] for c in cs])
        assert rc == 0 and outs == [S.model(c).data for c in cs]
    with emu_lib.scratch_budget(need - 1):  # ... and one byte less refuses the largest input
        rc, outs, _, _ = S.emu_stateless([c[1] for c in cs])
    assert rc == -4 and outs is None
