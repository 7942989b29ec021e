"""Streams with Flush points and the speculation re-run through the device's zstd encode batch on the wave emulator (no GPU).

The emulator runs the host rules that ship (compress_amd/csrc/kc_zenc_host.h: the block grid of a stream with Flush points, the
staging slots, the parameter fill, the rule that picks the re-run's units and blocks), so what tests/test_gpu_zstd.py
test_streams_with_flush_points_bit_exact and tests/test_redo_path.py check on the device is checked here on its host side too."""
import pytest

import corpora
import emu_lib
import oracle_lib
from test_redo_path import _make

WINDOW = 16 << 10  # blocks of 16 KiB: the directed shapes stay small


def _flush_cases():
    bs = WINDOW
    t = corpora.corpus("T", 6, 131072, first_unit=90).tobytes()
    m = corpora.corpus("M", 3, 131072, first_unit=5).tobytes()
    return [(t[:1000], [10, 500]),                            # cuts inside the first block
            (t[:1000], [1000]),                               # a cut at the end: empty last block
            (t[:1000], [0]),                                  # a cut at 0
            (t[:1000], []),                                   # a single short block without cuts: the EncodeAll frame form
            (t[:bs + 100], [50, bs + 100]),
            (t[:bs], [bs]), (t[:2 * bs], [bs]),               # cuts on a block boundary
            (t[:2 * bs + 9], [bs - 1, bs, bs + 1]),           # ... and one byte either side of it
            (t[:3 * bs], [7, 7, 7, 2 * bs + 7]),              # the same position three times
            (m[:bs + 5000], [100 * k for k in range(1, 25)]), # 24 cuts 100 bytes apart
            (b"", [0]), (b"", []),                            # the empty stream with and without a cut
            (t[:5], [1, 2, 3, 4, 5]),                         # a 5-byte stream cut after every byte
            (corpora.corpus("H", 1, bs).tobytes(), [bs // 2]),
            (t[:4 * bs + 1], [3 * bs + 6000, 4 * bs + 1, 4 * bs + 9])]


@pytest.mark.parametrize("level", [1, 2, 3])
def test_flush_points_on_the_emulator_equal_the_oracle(level):
    cases = _flush_cases()
    frames, err, redo = emu_lib.zstd_frames([u for u, _ in cases], stream_mode=1, level=level, window=WINDOW, flush_at=[c for _, c in cases])
    ref = oracle_lib.ZstdOracle(level=level, window_size=WINDOW)
    bad = [(i, len(u), cuts) for i, ((u, cuts), f) in enumerate(zip(cases, frames)) if f != ref.encode_stream(u, cuts)]
    assert not bad, "streams whose emulated frame differs from the oracle's (case, length, cuts): %r" % bad
    assert err == 0 and redo == 0


def test_speculation_re_run_on_the_emulator():
    """A late raw fallback with popped offsets (tests/test_redo_path.py, the 1 MiB form of its generator) at SpeedDefault: the
    emulator takes the re-run — match finder and entropy stage again over the flagged unit with the lowest flagged block's verdict
    forced — and ends at the oracle's frame; an ordinary stream through the same call takes none."""
    d, cuts = _make(7, 1 << 16, 1 << 20, 30, 250, 30, 5)
    ref = oracle_lib.ZstdOracle(level=2)
    frames, err, redo = emu_lib.zstd_frames([d.tobytes()], stream_mode=1, level=2, flush_at=[cuts])
    print("re-run units:", redo)
    assert err == 0 and frames[0] == ref.encode_stream(d.tobytes(), cuts)
    assert redo >= 1, "the batch did not take the re-run path"
    t = corpora.corpus("T", 3, 131072).tobytes()
    frames, err, redo = emu_lib.zstd_frames([t], stream_mode=1, level=2, flush_at=[[1000, 200000]])
    assert err == 0 and redo == 0 and frames[0] == ref.encode_stream(t, [1000, 200000])
