#!/usr/bin/env python3
"""Find inputs at which the two DEFLATE writers decide by a hair: walks seeded inputs, reads the MODEL's margins (the `margins` of
tests/deflate_model.py and tests/stateless_model.py: left side minus right side of every comparison between two encodings) and prints
the (seed, length) pairs at which a margin takes a wanted value.  The pairs go into tests/deflate_cases.py / tests/stateless_cases.py as
generator calls; the translated reference then judges the model on them (tests/test_ref_deflate.py).

    python tools/find_deflate_ties.py huff         # writeBlockHuff: ssize - estBits in {0, 1}, estBits - reuseSize in {0, -1}   (two minutes)
    python tools/find_deflate_ties.py stateless    # StatelessDeflate: dst.n - (len - len>>4) in {0, 1}; newSize - reuseSize in {1, 0, -1, -2}   (one minute)
    python tools/find_deflate_ties.py shapes       # seeds of the new-table and stored-by-size shapes of stateless_cases

The quick check's tie (abs against max) is not searched: deflate_cases.tie_quick builds the histogram with the wanted sum of squares.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import deflate_cases as D  # noqa: E402
import deflate_model as DM  # noqa: E402
import stateless_cases as S  # noqa: E402
import stateless_model as SM  # noqa: E402


def huff(limit=4):
    """ssize against estBits on one block of deflate_cases.tie_mix, walking its length; estBits against reuseSize on a block of
    deflate_cases.tie_shift behind deflate_cases.tie_first(), walking its length.  Blocks of 2048 bytes, penalty 10."""
    found = {}
    for seed in range(6):
        for every in (3, 4, 5, 6, 8):
            for n in range(200, 1025):
                w = DM.BitWriter(10)
                w.write_block_huff(False, D.tie_mix(seed, n, every), True)
                for name, m in w.margins:
                    if name == "ssize-est" and m in (0, 1):
                        found.setdefault((name, m), []).append(("mix", seed, n, every))
        if all(len(found.get(("ssize-est", m), ())) >= limit for m in (0, 1)):
            break
    first = D.tie_first()
    for seed in range(4):
        for p in (2, 4, 6, 8):
            base = D.tie_shift(seed, 2048, p)
            for n in range(100, 2049):
                w = DM.BitWriter(10)
                w.write_block_huff(False, first, False)
                k = len(w.margins)
                w.write_block_huff(False, base[:n], True)
                for name, m in w.margins[k:]:
                    if name == "est-reuse" and m in (0, -1):
                        found.setdefault((name, m), []).append(("shift", seed, n, p))
        if all(len(found.get(("est-reuse", m), ())) >= limit for m in (0, -1)):
            break
    for key in sorted(found):
        print(key, found[key][:limit])


def stateless(limit=4):
    """The token count on the 15/16 threshold, over the seeds of stateless_cases.tie_planted; and writeBlockDynamic's newSize against
    reuseSize in the second, open block of stateless_cases.shifted_alphabet(seed)[:FIRST + m]: the margin falls as m grows, so m is
    bisected to the crossing and the lengths around it are walked for margins of 1, 0 (reuse), -1 and -2 (the new table)."""
    want = {0: [], 1: []}
    for seed in range(3000):
        data = S.tie_planted(seed)
        r = SM.stateless_deflate_ex(data, seed % 2 == 0)
        for name, m in r.margins:
            if name == "tokens-15/16" and m in want and len(want[m]) < limit:
                want[m].append((seed, len(data)))
        if all(len(v) >= limit for v in want.values()):
            break
    print("tokens - (len - len>>4) == 0:", want[0])
    print("tokens - (len - len>>4) == 1:", want[1])

    def margin(seed, m):
        r = SM.stateless_deflate_ex(S.shifted_alphabet(seed)[:S.FIRST + m], False)
        ms = [v for k, v in r.margins if k == "dyn-new-reuse"]
        return ms[-1] if ms else None
    found = {}
    for seed in range(40):
        lo, hi = 300, 3900
        a, b = margin(seed, lo), margin(seed, hi)
        if a is None or b is None or not a > 0 > b:
            continue
        while hi - lo > 16:
            mid = (lo + hi) // 2
            v = margin(seed, mid)
            if v is None:
                break
            lo, hi = (mid, hi) if v > 0 else (lo, mid)
        for m in range(lo - 24, hi + 25):
            v = margin(seed, m)
            if v is not None and -2 <= v <= 1:
                found.setdefault(v, []).append((seed, m))
        if all(len(found.get(k, ())) >= 2 for k in (0, 1)) and sum(len(found.get(k, ())) for k in (-1, -2)) >= 3:
            break
    for k in sorted(found, reverse=True):
        print("newSize - reuseSize == %d (seed, m):" % k, found[k][:limit])


def shapes():
    """Seeds of the two-block and small shapes that the case set needs ten of: shifted_alphabet seeds whose second, open block takes the new
    table behind an owed EOB, and stored_by_size_planted seeds whose dynamic block would be larger than the bytes."""
    new_table = [seed for seed in range(5, 40) if SM.stateless_deflate_ex(S.shifted_alphabet(seed)[:S.FIRST + 3900], False).counts["dyn-new-table-eob-owed"]]
    print("shifted_alphabet, new table in the second block:", new_table[:8])
    by_size = [seed for seed in range(40) if SM.stateless_deflate_ex(S.stored_by_size_planted(seed), seed % 2 == 0).counts["dyn-stored-by-size"]]
    print("stored_by_size_planted, stored by size:", by_size[:8])


if __name__ == "__main__":
    {"huff": huff, "stateless": stateless, "shapes": shapes}[sys.argv[1] if len(sys.argv) > 1 else "huff"]()
