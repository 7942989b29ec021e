#!/usr/bin/env python3
"""Reference against model on seeded inputs beyond the suite: the translated reference (oracle/_ref/libzstdref.so) and the models of
tests/deflate_model.py / tests/stateless_model.py must write the same bytes.  Stateless inputs are `pieces` of stateless_cases in one to
four blocks, a third of them with a dictionary, both endings; HuffmanOnly inputs are chains of `block_of` blocks at small block sizes
and at 32768, penalties 10 / 8 / 7 / 0, both endings.  Not part of pytest; the result is recorded in profiles/flate_reference_parity.md.

    python tools/deflate_ref_sweep.py [seed] [seconds]      (default 0x5EEB, 600)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import deflate_cases as D  # noqa: E402
import deflate_model as DM  # noqa: E402
import oracle_goref as G  # noqa: E402
import stateless_cases as S  # noqa: E402
import stateless_model as SM  # noqa: E402


def main():
    seed = int(sys.argv[1], 0) if len(sys.argv) > 1 else 0x5EEB
    budget = float(sys.argv[2]) if len(sys.argv) > 2 else 600.0
    rng = random.Random(seed)
    t0 = time.time()
    n = {"stateless": 0, "huffman-only": 0}
    bad = []
    k = 0
    while time.time() - t0 < budget:
        k += 1
        if k % 2:
            nblk = rng.choice((1, 1, 2, 2, 3, 4))
            spec = [(rng.choice(S.SEED_KINDS), rng.randrange(13, S.FIRST + 1) if j == 0 and nblk == 1 else S.FIRST if j == 0 else S.LATER) for j in range(nblk)]
            if nblk > 1:
                spec[-1] = (spec[-1][0], rng.randrange(1, S.LATER + 1))
            data = S.pieces(spec, rng)
            dic = b""
            if rng.random() < 0.33:
                d = rng.choice((1, 100, 3000, 8192, 9000))
                dic = data[:d] if rng.random() < 0.5 and len(data) >= d else S.text(d, rng.randrange(1 << 18))
            eof = rng.random() < 0.5
            if G.flate_stateless(data, eof, dic) != SM.stateless_deflate(data, eof, dic):
                bad.append(("stateless", k, spec, eof, len(dic)))
            n["stateless"] += 1
        else:
            block = rng.choice((1024, 2048, 2048, 4096, 32768))
            nblk = rng.randint(1, 5)
            parts = [D.block_of(rng.choice(D.KINDS), block if b + 1 < nblk else rng.randint(1, block), rng) for b in range(nblk)]
            data = b"".join(parts)
            penalty = rng.choice((10, 10, 8, 7, 0))
            end = rng.choice((DM.END_CLOSE, DM.END_FLUSH))
            if G.flate_block_huff(data, block, penalty, G.BLOCK_HUFF_CLOSE if end == DM.END_CLOSE else G.BLOCK_HUFF_FLUSH) != DM.deflate(data, block, penalty, end):
                bad.append(("huffman-only", k, block, nblk, penalty, end))
            n["huffman-only"] += 1
    print("seed %#x: %d stateless and %d HuffmanOnly inputs in %.0f s, %d disagreements" % (seed, n["stateless"], n["huffman-only"], time.time() - t0, len(bad)))
    for b in bad[:20]:
        print(b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
