"""The HuffmanOnly writers' kernels and host sequence (compress_amd/csrc/kc_flate_deflate.hip, kc_deflate_host.h) on the wave emulator
against the model (tests/deflate_model.py): bytes, out_off and the bound, in batches of mixed inputs, behind 0xA5 guards on both
sides of a dst that is not word-aligned."""
import glob
import os

import pytest

import deflate_cases as D
import deflate_model as M
import emu_lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = D.emu_subset()
GROUPS = D.groups(CASES)


def check_group(cs, gz, key, cap=None):
    block, penalty, end = key
    rc, outs, out_off = D.emu_deflate([c[1] for c in cs], gz, end, block, penalty, cap=cap)
    assert rc == 0
    at = 0
    for i, c in enumerate(cs):
        want = D.model(c, gz)[0]
        assert outs[i] == want, (c[0], len(outs[i]), len(want))
        assert int(out_off[i]) == at
        at += len(want)
        assert len(want) <= M.bound(len(c[1]), block) + (18 if gz else 0)
    assert int(out_off[len(cs)]) == at
    return at


@pytest.mark.parametrize("gz", [False, True], ids=["flate", "gzip"])
@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "b%d-p%d-%s" % (k[0], k[1], "flush" if k[2] else "close"))
def test_emulator_equals_model(key, gz):
    """Every directed case and the first 160 seeded ones: one call per (block, penalty, end), all its inputs mixed in one batch."""
    check_group(GROUPS[key], gz, key)


def test_exact_capacity_and_one_byte_less():
    key = (D.BLOCK, D.PENALTY, M.END_CLOSE)
    cs = [c for c in GROUPS[key] if c[0].startswith(("sweep-", "one-", "multi-reuse"))]
    for gz in (False, True):
        total = sum(len(D.model(c, gz)[0]) for c in cs)
        assert check_group(cs, gz, key, cap=total) == total   # the exact total is enough
        rc, outs, out_off = D.emu_deflate([c[1] for c in cs], gz, key[2], key[0], key[1], cap=total - 1)
        assert rc == -2 and outs is None                      # KC_ERR_DST_TOO_SMALL, nothing written (emu_deflate checks every byte)
        assert int(out_off[len(cs)]) == total                 # ... and the layout says what it takes


def test_empty_batch_and_empty_inputs():
    rc, outs, out_off = D.emu_deflate([], False)
    assert rc == 0 and outs == [] and int(out_off[0]) == 0
    rc, outs, _ = D.emu_deflate([b"", b"", b"x", b""], True)
    assert rc == 0 and outs == [M.gzip_deflate(d) for d in (b"", b"", b"x", b"")]


def test_goldens_ended_with_flush():
    """The reference's nine expectations of writeBlockHuff through the device code, at (65535, 8): a single block that ends with Flush
    is the golden's bytes — writeBlockHuff(false, all, true) differs from the golden's (false, all, false) + flush only in who pays
    the EOB — and then the empty stored block: 00 00 ff ff when the EOB ended a byte, else 00 00 00 ff ff... (3 bits in the last byte or
    in one more)."""
    names = sorted(glob.glob(os.path.join(GOLD, "flate_in", "huffman-*.in")))
    assert len(names) == 9
    datas = [open(p, "rb").read() for p in names]
    rc, outs, _ = D.emu_deflate(datas, False, M.END_FLUSH, 65535, 8)
    assert rc == 0
    for p, out in zip(names, outs):
        want = open(os.path.join(GOLD, "flate", os.path.basename(p)[:-3] + ".golden"), "rb").read()
        # the golden's last byte holds the EOB's last bits and zero padding; the 3 header bits 000 of the empty stored block fall
        # into that padding or into one more zero byte
        assert out[:len(want)] == want, p
        assert out[len(want):] in (b"\x00\x00\xff\xff", b"\x00\x00\x00\xff\xff"), (p, out[len(want):])


def test_scratch_budget_cuts_the_batch():
    """A budget of a few block records: the call is cut into groups of inputs, plans each group twice and writes the same bytes."""
    key = (D.BLOCK, D.PENALTY, M.END_CLOSE)
    cs = [c for c in GROUPS[key] if c[0].startswith(("multi-", "text-3", "text-6", "sweep-1"))]
    with emu_lib.scratch_budget(12 * 1024):
        check_group(cs, True, key)
        batches = emu_lib.last_batches()
    assert batches > 3
    need = emu_lib.last_max_need()
    with emu_lib.scratch_budget(need):  # the least budget that refuses nothing ...
        check_group(cs, False, key)
    with emu_lib.scratch_budget(need - 1):  # ... and one byte less refuses the largest input
        rc, outs, _ = D.emu_deflate([c[1] for c in cs], False, key[2], key[0], key[1])
    assert rc == -4 and outs is None
