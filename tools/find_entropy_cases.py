#!/usr/bin/env python3
"""Search for directed inputs of the zstd entropy stage (no GPU): the oracle's decision counters (oracle/kco_counters.h) are the
objective, the generators of tests/entropy_cases.py the search space.

  tools/find_entropy_cases.py --decision "<substring of a counter name>" [--level N]
        prints the parameters of the first candidate that reaches the decision (at the level, or at any)
  tools/find_entropy_cases.py --emit
        runs every candidate at the four levels, covers every reachable (decision, level) greedily with as few candidates as it
        can and prints the CASES list that tests/entropy_cases.py commits
  tools/find_entropy_cases.py --weights-search
        samples complete prefix codes and prints the weight histograms that send the byte FSE of the Huffman weights
        (huff0/huff0.go:211-229) into normalizeCount2, with the exit they take: the parameters of family litw
  tools/find_entropy_cases.py --enumerate-round-robin [--max-n 63]
        exhaustive: every histogram of the sequence coders with up to 63 sequences (every multiset of counts, every symbolLen up
        to 53) through a model of fseEncoder.normalizeCount / normalizeCount2; prints the ones that take the `total == 0` exit.
        (From 64 sequences on the table log is at least highBit(symbolLen - 1) + 2: profiles/entropy_decisions.md argues that case.)
  tools/find_entropy_cases.py --table
        hit table of the committed CASES per decision and level (profiles/entropy_decisions.md)
  tools/find_entropy_cases.py --table-old
        the same for the inputs the parity tests had before (tests/test_outcome_coverage._inputs + corpora.rle_literal_units)

Candidates are enumerated in a fixed order from fixed seeds, so the list is reproducible and can be extended: add a family or widen a
range in candidates() and run --emit again."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import entropy_cases as ec  # noqa: E402
import oracle_lib  # noqa: E402


def candidates():
    """(family, parameters) in a fixed order; the cheap families first."""
    rng = np.random.default_rng(0xCA5E)
    # --- literal programmes ---
    for a in (2, 3):
        for b in (20, 100, 700):
            yield "lit", ("equal0", a, b, a)
            yield "lit", ("fib0", a, b, a)
    for a in range(4, 13):
        for seed in range(6):
            yield "lit", ("fib0", a, 1 + seed % 3, seed)
    for a in (4, 8, 16, 32, 64, 128):
        for b in (3, 9, 40):
            yield "lit", ("equal0", a, b, a)
            yield "lit", ("equal", a, b, a)
    for a in range(8, 27):  # deeper than the table log by 1 .. 6 and more
        for b in (1, 2, 3):
            yield "lit", ("fib", a, b, a)
    for ln in (16, 17, 1023, 1024):  # (with the 1X / 4X boundary lengths)
        yield "lit", ("steps", 16, ln // 60, ln)
    for n in (1023, 1024):
        yield "lit", ("flat", n // 8, 8, n)
    for a in (129, 140, 160, 192, 200, 256):
        for b in (3, 30, 300):
            yield "lit", ("flat", a, b, a)
        for b in (1500, 20000, 120000):
            yield "lit", ("skew", a, b, a)
    for i in range(1500):  # many distinct symbols in 33 .. 400 bytes: table logs 5 .. 8 with a forced height limit
        yield "lit", ("skew", int(rng.integers(8, 60)), int(rng.integers(33, 400)), i)
    for i in range(300):
        yield "lit", ("skew0", int(rng.integers(3, 14)), int(rng.integers(33, 3000)), i)
    for i in range(200):
        yield "lit", ("skew", int(rng.integers(20, 256)), int(rng.choice([2000, 9000, 66000, 131072, 250000])), i)
    for i in range(300):
        yield "lit", ("skew", int(rng.integers(4, 14)), int(rng.integers(33, 52)), i)  # 32 .. 47 bytes: "no smaller than raw" by the headers
    for a in (3, 6, 12, 48, 192):
        yield "lit", ("eqlast0", a, 5, a)
    for i in range(200):
        yield "lit", ("loguni", int(rng.integers(12, 256)), int(rng.integers(8, 56)), i)
    for zeros in (0, 1, 3):  # weight histograms that send the byte FSE of the weights into normalizeCount2 (found by --weights-search)
        for seed in range(3):
            yield "litw", ((2, 1, 2, 2, 2, 2, 2), zeros, 3, 1 + seed, seed)
    for bs in (65536, 131072):
        for e in (100, 200):
            yield "lit2", (bs, e, e)
    # --- periodic units ---
    for head in (0, 1, 5):
        for period in (1, 2, 11, 16, 17, 100, 1023, 1024):
            for total in (40, 300, 5000, 70000, 131072, 140000):
                if total > head + period + 8:
                    yield "per", (head, period, total, period)
    yield "per", (65536, 300, 131072, 1)
    yield "per", (65537, 300, 131072, 2)
    # --- sequence programmes ---
    yield "seq", (43, "flat", 8, 15, "flat", 43, 47, 1)  # 43 sequences, 43 distinct ML codes: see profiles/entropy_decisions.md
    for seed in range(2, 6):  # 22 sequences with 22 distinct LL codes: the LL coder's round robin at table log 5 (see --enumerate-round-robin)
        yield "seq", (22, "flat", 22, 24, "flat", 3, 12, seed)
    for seed in range(4):  # and 44 with 44 distinct ML codes (table log 6)
        yield "seq", (44, "flat", 8, 15, "flat", 44, 48, seed)
    for n in (127, 128):
        for seed in range(3):
            yield "seq", (n, "geo", 12, 20, "geo", 12, 30, seed)
    for n in (1, 2, 5, 17, 31, 32, 43, 60, 100, 200, 300, 600, 1100, 2500):
        for shape in ("flat", "geo", "big", "pair"):
            for seed in range(4):
                ll_k, ml_k = int(rng.integers(1, 30)), int(rng.integers(1, 40))
                ll_top, ml_top = int(rng.choice([8, 15, 24, 27, 29])), int(rng.choice([10, 31, 42, 45, 47]))
                alpha = int(rng.choice([256, 256, 1, 3, 16, 64]))
                yield "seq", (n, shape, ll_k, ll_top, str(rng.choice(["flat", "geo", "big", "pair"])), ml_k, ml_top, seed, alpha,
                              int(rng.choice([0, 0, 7, 300])))
    for n, ll in ((20, 1), (2100, 2), (1400, 3)):  # RLE literal sections of 20 and of 4096+ bytes: short runs of one byte between matches
        for seed in range(2):
            yield "seq", (n, "top", 1, ll, "top", 1, 13, seed, 1)
    for t in range(17, 32):  # 17 .. 31 literals over a few dozen values: "no smaller than raw" by the two headers
        for alpha in (8, 10, 12, 14, 16, 20):
            for seed in range(4):
                yield "seq", (3, "top", 1, 0, "top", 1, 13, seed, alpha, t, 0)
    for n in (40, 200):  # LL / ML codes 0 (5) and a far one only: zero runs of 24 and more in the table description
        for top in (26, 27, 28, 29):
            yield "seq", (n, "ends", 2, top, "ends", 2, 34 + top % 3, top)
    for n in (255, 256, 300, 480, 490, 500, 505, 511, 512, 1000):  # many codes once, a few sharing the rest: normalizeCount2's second pass
        for k in (14, 16, 20, 24, 27, 32):
            for seed in range(3 if k != 27 else 6):
                yield "seq", (n, "few", k, k - 1, "few", k, k + 4, seed)
                yield "seq", (n, "few2", k, k - 1, "few2", k, k + 4, seed)
    for seed in range(6):  # an RLE literal section above 4095 bytes
        for step in (9, 12):
            yield "rle", (4200, step, seed)
    for n in (245, 250):  # the offset coder's normalizeCount2, second pass
        for seed in range(2):
            yield "ofs", (n, seed)
    for total in (16, 17, 1023, 1024):  # literal sections of exactly these lengths in a block with sequences
        for alpha in (16, 256):
            yield "seq", (4, "flat", 1, 0, "flat", 3, 30, total, alpha, total)
    for n, ll_top in ((40, 31), (20, 33), (6, 34)):  # long literal runs: LL codes up to 34
        for seed in range(3):
            yield "seq", (n, "flat", 6, ll_top, "geo", 8, 40, seed, [256, 16, 200][seed])
    for seed in range(3):  # several blocks with compressible literals: table reuse
        yield "seq", (4000, "geo", 10, 24, "geo", 10, 30, seed, 12)


def weights_search(tries=200000, seed=1):
    """Random complete prefix codes of up to 230 symbols and 11 bits -> the histogram of their weights without the last symbol
    (any weight) and with 0 .. 60 absent symbols -> a model of fse/compress.go:510 normalizeCount / :557 normalizeCount2 at the
    table log the weights always get (5).  Prints the first histogram per exit of normalizeCount2."""
    import random
    rtb = [0, 473195, 504333, 520860, 550000, 700000, 750000, 830000]

    def exit_of(counts):
        n, T = sum(counts), 5
        scale, step, low = 62 - T, (1 << 62) // sum(counts), sum(counts) >> T
        still, largest = 1 << T, 0
        for c in counts:
            if c == 0:
                continue
            if c <= low:
                still -= 1
                continue
            p = (c * step) >> scale
            if p < 8 and c * step - (p << scale) > (1 << (scale - 20)) * rtb[p]:
                p += 1
            largest = max(largest, p)
            still -= p
        if -still < (largest >> 1):
            return None
        tot, dist, low_one, left = n, 0, (n * 3) >> (T + 1), []
        for c in counts:
            if c and c <= max(low, low_one):
                dist += 1
                tot -= c
            elif c:
                left.append(c)
        second = (1 << T) - dist > 0 and tot // ((1 << T) - dist) > low_one
        if second:
            low_one = (tot * 3) // (((1 << T) - dist) * 2)
            tot -= sum(c for c in left if c <= low_one)
        return ("round robin" if tot == 0 else "proportional") + (" after the second pass" if second else "")

    rnd = random.Random(seed)
    found = {}
    for _ in range(tries):
        depth_limit, leaves, n_leaves, target = rnd.randint(3, 11), {0: 1}, 1, rnd.randint(4, 230)
        while n_leaves < target:
            ds = [d for d, c in leaves.items() if c > 0 and d < depth_limit]
            if not ds:
                break
            d = rnd.choice(ds) if rnd.random() < 0.5 else (max(ds) if rnd.random() < 0.5 else min(ds))
            k = min(rnd.randint(1, leaves[d]) if rnd.random() < 0.3 else 1, target - n_leaves)
            leaves[d] -= k
            leaves[d + 1] = leaves.get(d + 1, 0) + 2 * k
            n_leaves += k
        deepest = max(d for d, c in leaves.items() if c > 0)
        h = [0] * (deepest + 1)
        for d, c in leaves.items():
            if c:
                h[deepest + 1 - d] = c
        for last in [w for w in range(1, deepest + 1) if h[w]]:
            for zeros in (0, 1, 3, 7, 20, 60):
                hh = h[:]
                hh[last] -= 1
                hh[0] = zeros
                if not 3 <= sum(hh) <= 255 or max(hh) in (1, sum(hh)):
                    continue
                e = exit_of(hh)
                if e and e not in found:
                    found[e] = (hh, last)
                    print("%s: symbols per weight 1.. %r, %d absent, the last symbol of weight %d" % (e, tuple(hh[1:]), zeros, last))
    print("exits reached in %d codes: %s" % (tries, sorted(found) or "none"))


RTB = [0, 473195, 504333, 520860, 550000, 700000, 750000, 830000]


def nc2_exit(mult, n, T, first_is_low):
    """zstd/fse_encoder.go:259 normalizeCount and :334 normalizeCount2 on a histogram given as [(count, how many symbols)], total n,
    at table log T.  Returns None (normalizeCount2 not entered) or (exit, second pass taken).  Only `norm[largest]` depends on the
    order of the symbols, and only when no symbol is above lowThreshold: first_is_low says whether symbol 0 is then a -1 symbol."""
    scale, step, low = 62 - T, (1 << 62) // n, n >> T
    still, largest = 1 << T, 0
    for c, k in mult:
        if c <= low:
            still -= k
            continue
        p = (c * step) >> scale
        if p < 8 and c * step - (p << scale) > (1 << (scale - 20)) * RTB[p]:
            p += 1
        largest = max(largest, p)
        still -= p * k
    half = (largest >> 1) if largest else (-1 if first_is_low else 0)
    if -still < half:
        return None
    total, dist, low_one, left = n, 0, (n * 3) >> (T + 1), []
    for c, k in mult:
        if c <= low or c <= low_one:
            dist += k
            total -= c * k
        else:
            left.append((c, k))
    to_dist = (1 << T) - dist
    second = to_dist > 0 and total // to_dist > low_one  # (to_dist == 0 is a division by zero in the reference: reported below)
    if to_dist <= 0:
        return ("toDistribute <= 0", False)
    if second:
        low_one = (total * 3) // (to_dist * 2)
        for c, k in left:
            if c <= low_one:
                dist += k
                total -= c * k
    return ("round robin" if total == 0 else "other", second)


def enumerate_round_robin(max_n=63):
    """Every multiset of counts with sum n <= max_n and at most 53 parts, with every symbolLen from the number of parts to 53."""
    def hb(v):
        return v.bit_length() - 1

    def parts(n, biggest, room):  # partitions of n in parts <= biggest, at most `room` parts, as [(count, multiplicity)]
        if n == 0:
            yield []
            return
        if room == 0 or biggest == 0:
            return
        for c in range(min(n, biggest), 0, -1):
            for k in range(min(n // c, room), 0, -1):
                for rest in parts(n - c * k, c - 1, room - k):
                    yield [(c, k)] + rest

    found, tried = [], 0
    for n in range(1, max_n + 1):
        max_bits_src = (hb(n - 1) - 2) & 255 if n > 1 else 253
        for mult in parts(n, n, 53):
            m = sum(k for _, k in mult)
            logs = {}
            for S in range(max(m, 1), 54):
                min_bits = min(hb(n) + 1, (hb(S - 1) + 2) if S > 1 else 255 + 2)
                T = min(8, max_bits_src)
                T = min(8, max(T, min_bits, 5))
                logs.setdefault(T, S)
            for T, S in logs.items():
                if max(c for c, _ in mult) == n:
                    continue  # (one symbol: useRLE, no normalisation)
                for first_is_low in (False, True):
                    tried += 1
                    r = nc2_exit(mult, n, T, first_is_low)
                    if r and r[0] != "other" and (n, mult, T) not in [f[:3] for f in found]:
                        found.append((n, mult, T, S, r))
                        print("n = %d, table log %d, symbolLen >= %d, counts x symbols %r: %s%s" % (n, T, S, mult, r[0], ", after the second pass" if r[1] else ""), flush=True)
    print("%d histograms x table logs tried, n <= %d: %d take the total == 0 exit" % (tried, max_n, len(found)))


def run(enc_cache, fam, params, level):
    """Counters that one whole-unit EncodeAll of the candidate hits at the level, after checking the round trip."""
    case = ("", fam, params)
    kw = ec.oracle_kw(case, level)
    key = (level, bool(kw.get("all_lit_entropy")), ec.uses_dict(case))
    if key not in enc_cache:
        enc_cache[key] = oracle_lib.ZstdOracle(**kw)
    u = ec.unit(case)
    oracle_lib.counters(reset=True)
    fr = enc_cache[key].encode_all(u)
    hit = {k for k, v in oracle_lib.counters(reset=True).items() if v}
    back = oracle_lib.zstd_decode(fr, len(u) + 16, dict_content=kw.get("dict_content"))
    assert back == u, ("the oracle's frame does not decode to the input", fam, params, level)
    return hit


def table(rows, title):
    names = list(oracle_lib.counters())
    print("| decision | " + " | ".join("level %d" % lv for lv in ec.LEVELS) + " |")
    print("|---|" + "---|" * len(ec.LEVELS))
    for n in names:
        print("| %s | %s |" % (n, " | ".join(str(rows[lv].get(n, 0)) for lv in ec.LEVELS)))
    print("\n(%s)" % title)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decision")
    ap.add_argument("--level", type=int)
    ap.add_argument("--emit", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-old", action="store_true")
    ap.add_argument("--weights-search", action="store_true")
    ap.add_argument("--enumerate-round-robin", action="store_true")
    ap.add_argument("--max-n", type=int, default=63)
    a = ap.parse_args()
    cache = {}
    if a.weights_search:
        weights_search()
        return
    if a.enumerate_round_robin:
        enumerate_round_robin(a.max_n)
        return
    if a.table or a.table_old:
        rows = {}
        for lv in ec.LEVELS:
            oracle_lib.counters(reset=True)
            if a.table:
                for c in ec.CASES:
                    kw = ec.oracle_kw(c, lv)
                    oracle_lib.ZstdOracle(**kw).encode_all(ec.unit(c))
            else:
                import corpora
                import test_outcome_coverage
                e = oracle_lib.ZstdOracle(level=lv)
                for u in test_outcome_coverage._inputs():
                    e.encode_all(u)
                dct, units = corpora.rle_literal_units()
                e = oracle_lib.ZstdOracle(level=lv, dict_id=7, dict_content=dct)
                for u in units:
                    e.encode_all(u)
            rows[lv] = oracle_lib.counters(reset=True)
        table(rows, "the committed cases of tests/entropy_cases.py" if a.table else "the parity inputs before the directed cases")
        return
    if a.decision:
        for fam, params in candidates():
            for lv in ([a.level] if a.level else ec.LEVELS):
                if any(a.decision in h for h in run(cache, fam, params, lv)):
                    print("level %d: %r" % (lv, (fam, params)))
                    return
        print("no candidate reaches %r" % a.decision)
        sys.exit(1)
    if a.emit:
        cands = list(candidates())
        hits = [{lv: run(cache, fam, params, lv) for lv in ec.LEVELS} for fam, params in cands]
        want = {(d, lv) for h in hits for lv in ec.LEVELS for d in h[lv]}
        size = [len(ec.unit(("", f, p))) for f, p in cands]
        chosen = []
        while want:
            # most new (decision, level) pairs first; among equals the smaller unit, then the earlier candidate
            gain = [sum(1 for lv in ec.LEVELS for d in h[lv] if (d, lv) in want) for h in hits]
            best = max(range(len(cands)), key=lambda i: (gain[i], -size[i], -i))
            if gain[best] == 0:
                break
            new = {lv: sorted(d for d in hits[best][lv] if (d, lv) in want) for lv in ec.LEVELS}
            want -= {(d, lv) for lv in ec.LEVELS for d in new[lv]}
            chosen.append((best, {lv: v for lv, v in new.items() if v}))
        chosen.sort()
        print("CASES = [")
        for i, reaches in chosen:
            fam, params = cands[i]
            print("    (%r, %r, %r, {" % ("%s%04d" % (fam, i), fam, params))
            for lv in sorted(reaches):
                print("        %d: [%s]," % (lv, ",\n            ".join(repr(d) for d in reaches[lv])))
            print("    }),")
        print("]")
        names = set(oracle_lib.counters())
        for lv in ec.LEVELS:
            missing = sorted(names - {d for h in hits for d in h[lv]})
            print("# level %d: no candidate reaches: %s" % (lv, "; ".join(missing) or "-"), file=sys.stderr)


if __name__ == "__main__":
    main()
