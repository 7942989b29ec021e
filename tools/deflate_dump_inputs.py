#!/usr/bin/env python3
"""Writes the inputs of tools/deflate_check_main.cpp into a directory: the data of cases of tests/deflate_cases.py, one file each.

    python tools/deflate_dump_inputs.py tools/_build/deflate_inputs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as D  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    directed = [c for c in D.directed() if c[0].endswith("/close") or c[0].startswith("sweep-")]
    seeded = list(D.seeded()[:60])
    for k, c in enumerate(directed + seeded):
        name = "%03d-%s" % (k, "".join(ch if ch.isalnum() else "_" for ch in c[0]))
        with open(os.path.join(out, name), "wb") as f:
            f.write(c[1])
    print("%d inputs in %s" % (len(directed) + len(seeded), out))


if __name__ == "__main__":
    main()
