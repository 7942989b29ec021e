#!/usr/bin/env python3
"""Writes the inputs of tools/stateless_check_main.cpp into a directory: the data of cases of tests/stateless_cases.py (those without a dictionary; the program adds dictionaries of its own), one file each.

    python tools/stateless_dump_inputs.py tools/_build/stateless_inputs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stateless_cases as S  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    small = [c for c in S.directed() if not c[3] and len(c[1]) <= 2000]
    directed = small[::3] + [c for c in S.directed() if c[0] in ("cut-32768-text", "planted-32767", "text-then-short-60", "shifted-alphabet-0")]
    seeded = [c for c in S.seeded()[:60] if not c[3] and len(c[1]) <= 8000][:12]
    for k, c in enumerate(directed + seeded):
        name = "%03d-%s" % (k, "".join(ch if ch.isalnum() else "_" for ch in c[0]))
        with open(os.path.join(out, name), "wb") as f:
            f.write(c[1])
    print("%d inputs in %s" % (len(directed) + len(seeded), out))


if __name__ == "__main__":
    main()
