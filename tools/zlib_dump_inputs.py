#!/usr/bin/env python3
"""Writes the base inputs of tools/zlib_check_main.cpp into a directory: streams of tests/zlib_cases.py as files, a stream's preset
dictionary beside it as <name>.dict.

    python tools/zlib_dump_inputs.py tools/_build/zlib_inputs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zlib_cases as ZC  # noqa: E402
import zlib_model as Z  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    directed = [c for c in ZC.cases() if c.name.endswith("-whole") or c.name.startswith(("fdict/", "trailer/", "vec/"))]
    sweep = [c for _, c in ZC.adler_sweep((0, 1, 5, 257, 5553, 16383, 16384, 16385, 65521, 65536)) if c.name.endswith("-first1")]
    gen = [c for c in ZC.generated()[:480] if ZC.verdict(c)[1] == Z.OK][:24]
    for k, c in enumerate(directed + sweep + gen):
        name = "%03d-%s" % (k, "".join(ch if ch.isalnum() else "_" for ch in c.name))
        with open(os.path.join(out, name), "wb") as f:
            f.write(c.data)
        if c.dict:
            with open(os.path.join(out, name + ".dict"), "wb") as f:
                f.write(c.dict)
    print("%d inputs in %s" % (len(directed) + len(sweep) + len(gen), out))


if __name__ == "__main__":
    main()
