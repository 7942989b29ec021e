"""The directed entropy-stage inputs (tests/entropy_cases.py) through the device code on the wave emulator (no GPU): the frames
kc_huf_dev.h / kc_fse_dev.h / kc_zstd_entropy.hip write equal the oracle's, at levels 1 - 4, with the LDS and the group match
finder at level 1.  tests/test_entropy_decisions.py shows which decisions of the reference each case takes.

The emulator entry takes no dictionary: the sequence programmes (families seq, rle, ofs) run on the device only
(tests/test_gpu_entropy_decisions.py)."""
import pytest

import emu_lib
import entropy_cases as ec
import oracle_lib

CASES = [c for c in ec.CASES if not ec.uses_dict(c)]


def _check(level, finder="lds"):
    bad = []
    for ale in (False, True):  # (one emulated launch per option set: all_lit_entropy is a launch parameter)
        cases = [c for c in CASES if bool(ec.oracle_kw(c, level).get("all_lit_entropy")) == ale]
        if not cases:
            continue
        units = [ec.unit(c) for c in cases]
        kw = {"all_lit_entropy": True} if ale else {}
        ref = oracle_lib.ZstdOracle(level=level, **kw)
        frames, err, redo = emu_lib.zstd_frames(units, use_grp=finder != "lds", level=level, max_encoded_size=ref.max_encoded_size,
                                                all_lit_entropy=ale or level > 2)
        assert err == 0 and redo == 0
        bad += [(c[0], len(u), len(f)) for c, u, f in zip(cases, units, frames) if f != ref.encode_all(u)]
    assert not bad, "cases whose emulated frame differs from the oracle's (name, length, frame length): %r" % bad
    return True


def test_there_are_cases_without_a_dictionary():
    assert len(CASES) >= 15 and {c[1] for c in CASES} >= {"lit", "lit2", "litw", "per"}


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_directed_cases_on_the_emulator(level):
    assert _check(level)


def test_directed_cases_on_the_emulator_group_finder():
    assert _check(1, finder="grp")
