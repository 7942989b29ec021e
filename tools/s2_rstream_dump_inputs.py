"""The inputs of tools/s2_rstream_check_main.cpp as files: the item-1 streams of tests/s2_decode_cases.py (itemNN.s2) and its 480 seeded
mutations (mutNNN.s2), made with the reference's own writer (translated: oracle/_ref, built by build()).

    python tools/s2_rstream_dump_inputs.py DIR
    ASAN_OPTIONS=detect_leaks=0 tools/_build/s2_rstream_check DIR/item*.s2          # each with the program's own mutation recipe
    ASAN_OPTIONS=detect_leaks=0 tools/_build/s2_rstream_check -n 0 DIR/mut*.s2      # the 480 mutations the tests judge
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_goref as G  # noqa: E402
import s2_decode_cases as K  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    items = K.item1_streams(G)
    for i, (_, s, _) in enumerate(items):
        with open(os.path.join(out, "item%02d.s2" % i), "wb") as f:
            f.write(s)
    muts = K.mutations([s for _, s, _ in items[:8]])
    for k, m in enumerate(muts):
        with open(os.path.join(out, "mut%03d.s2" % k), "wb") as f:
            f.write(m)
    print("%d streams, %d mutations -> %s" % (len(items), len(muts), out))


if __name__ == "__main__":
    main()
