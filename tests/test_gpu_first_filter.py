"""The first-occurrence filter of the SpeedFastest HBM-table kernel on the device (KC_OPT_ZFAST_FIRST_FILTER, kc_zstd_first.hip):
frames with the option on and off are the same bytes, and the oracle's.  tests/test_emu_first_filter.py checks the bits themselves."""
import numpy as np
import pytest

import corpora
import first_filter_cases as ffc

pytestmark = pytest.mark.gpu

OPT_FIRST_FILTER, OPT_VARIANT, OPT_LAST_FIRST_BITS = 38, 27, 103


def _batch(n):
    """n units: every kind and length of the emulator tests, the long ones first, repeated where n asks for more."""
    pool = [u for _, u in reversed(ffc.all_units())]
    return [pool[i % len(pool)] for i in range(n)]


@pytest.fixture(scope="module")
def reference(oracle):
    buf, off = corpora.pack_units(_batch(65))
    ref, ref_off = oracle.zstd_encode_units(buf, off, threads=8, level=1)
    ref = np.asarray(ref)
    return [ref[int(ref_off[i]):int(ref_off[i + 1])].tobytes() for i in range(65)]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])  # one group, a wave minus one unit, a whole wave, a wave and a group, nine waves
def test_frames_same_with_and_without_the_filter(reference, kclib, n):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from compress_amd import zstd
    units = _batch(n)
    buf, off = corpora.pack_units(units)
    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(1), zstd.WithMatchPath("hbm"))
    assert enc.ctx().get_option(OPT_FIRST_FILTER) == 1  # the default
    got = {}
    # one context throughout: its table arena is never cleared in between (epoch stamps), so later batches look up stale buckets
    for first, variant in ((1, 0), (0, 0), (1, 1), (0, 1), (1, 0)):
        enc.ctx().set_option(OPT_FIRST_FILTER, first)
        enc.ctx().set_option(OPT_VARIANT, variant)  # the match finder's compiled form
        out, out_off = enc.EncodeUnits(buf, off)
        assert enc.ctx().last_path() == "hbm"
        assert enc.ctx().get_option(OPT_LAST_FIRST_BITS) == first  # the match finder really ran with / without the bits
        frames = [out[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)]
        bad = [(i, len(units[i])) for i in range(n) if frames[i] != reference[i]]
        assert not bad, "filter %d, form %d: frames differing from the oracle's (unit, length): %r" % (first, variant, bad[:8])
        got[first, variant] = frames
    assert got[1, 0] == got[0, 0] and got[1, 1] == got[0, 1]
    enc.Close()


def _hbm_writer(*opts):
    from compress_amd import zstd
    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(1), zstd.WithMatchPath("hbm"), *opts)
    enc.ctx().set_option(OPT_FIRST_FILTER, 1)
    enc.ctx().set_option(OPT_VARIANT, 0)  # (a fixed form: the bits are not dropped for input that did not compress)
    return enc


def test_no_bits_with_a_dictionary(oracle, kclib):
    """A dictionary primes every unit's table: a bucket that the unit has not written may hold a dictionary candidate, so the bits
    must not be used — the option is on, the match finder gets none, and the frames are the oracle's.  The same context then
    encodes the same units without the dictionary: with the bits."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from compress_amd import zstd
    dct = ffc.content("text")[100000:100000 + 65536]
    units = _batch(17)
    buf, off = corpora.pack_units(units)
    enc = _hbm_writer(zstd.WithEncoderDictRaw(7, dct))
    out, out_off = enc.EncodeUnits(buf, off)
    assert enc.ctx().last_path() == "hbm"
    assert enc.ctx().get_option(OPT_LAST_FIRST_BITS) == 0
    ref, ref_off = oracle.zstd_encode_units(buf, off, threads=8, level=1, dict_id=7, dict_content=dct)
    assert np.array_equal(out_off, ref_off) and np.array_equal(out, np.asarray(ref))
    enc.Close()
    enc = _hbm_writer()
    out, out_off = enc.EncodeUnits(buf, off)
    assert enc.ctx().get_option(OPT_LAST_FIRST_BITS) == 1
    enc.Close()


def test_no_bits_for_the_jobs_of_a_stream(oracle, kclib):
    """The jobs of a WithConcurrentBlocks stream start with tables primed from their overlap prefixes: no bits, the oracle's stream."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from compress_amd import zstd
    win = 1 << 17
    data = corpora.corpus("T", 12, 131072, first_unit=40).tobytes()  # 1.5 MiB: three jobs of 512 KiB, two of them with a prefix
    enc = _hbm_writer(zstd.WithConcurrentBlocks(True), zstd.WithEncoderConcurrency(4), zstd.WithWindowSize(win))
    ref = oracle.ZstdOracle(level=1, window_size=win)
    for cuts in ((), (1000, 300000)):
        got = enc.EncodeJobs(data, cuts)
        assert enc.ctx().last_path() == "hbm"
        assert enc.ctx().get_option(OPT_LAST_FIRST_BITS) == 0
        assert got == ref.encode_jobs(data, cuts), cuts
    enc.Close()


def test_no_bits_for_input_that_did_not_compress(oracle, kclib):
    """With the form chosen per batch (the default), a batch behind one that did not compress runs without the pre-pass."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from compress_amd import zstd
    r = corpora.corpus("H", 16, 131072, first_unit=3).tobytes()
    buf, off = corpora.pack_units([r[i * 131072:(i + 1) * 131072] for i in range(16)])
    ref, ref_off = oracle.zstd_encode_units(buf, off, threads=8, level=1)
    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(1), zstd.WithMatchPath("hbm"))
    for k in range(2):
        out, out_off = enc.EncodeUnits(buf, off)
        assert np.array_equal(out_off, ref_off) and np.array_equal(out, np.asarray(ref))
        assert enc.ctx().get_option(OPT_LAST_FIRST_BITS) == (1 if k == 0 else 0), k
    enc.Close()
