#!/usr/bin/env python3
"""Writes the inputs of tools/zip_check_main.cpp into a directory: the buffers of tests/zip_cases.py — the reference's fixtures, the
hand-built cases, the stored shapes and the 480 mutations — one file each.

    python tools/zip_dump_inputs.py tools/_build/zip_inputs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zip_cases as ZC  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    cs = ZC.fixture_cases() + ZC.directed() + [ZC.stored_cases(False)] + ZC.mutations()
    for k, c in enumerate(cs):
        name = "%04d-%s" % (k, "".join(ch if ch.isalnum() else "_" for ch in c.name))
        with open(os.path.join(out, name), "wb") as f:
            f.write(c.data)
    print("%d inputs in %s" % (len(cs), out))


if __name__ == "__main__":
    main()
