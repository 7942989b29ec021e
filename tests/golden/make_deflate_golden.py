"""Writes tests/golden/deflate_model_sha256.txt: one digest per case family of what tests/deflate_model.py writes, flate and gzip.

    python tests/golden/make_deflate_golden.py

The digests pin the model: a change of the model that changes any stream of a family changes its line.  (The model itself is pinned
to the reference by the nine huffman-*.golden files and by the reference's inflate, tests/test_deflate_model.py.)"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "deflate_model_sha256.txt")


def families():
    import deflate_cases as D
    d, s = D.directed(), D.seeded()
    fam = {
        "lengths": [c for c in d if c[0].startswith("text-")],
        "sweep": [c for c in d if c[0].startswith("sweep-")],
        "contents": [c for c in d if not c[0].startswith(("text-", "sweep-", "multi-"))],
        "multi-block": [c for c in d if c[0].startswith("multi-")],
        "seeded-000-159": list(s[:160]),
        "seeded-160-399": list(s[160:]),
    }
    assert sum(len(v) for k, v in fam.items() if not k.startswith("seeded")) == len(d)
    return fam


def digests():
    import deflate_cases as D
    rows = []
    for name, cs in families().items():
        for gz in (False, True):
            h = hashlib.sha256()
            for c in cs:
                out = D.model(c, gz)[0]
                h.update(c[0].encode() + b"\0" + len(out).to_bytes(8, "little") + out)
            rows.append("%s  %s/%s" % (h.hexdigest(), "gzip" if gz else "flate", name))
    return rows


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write("\n".join(digests()) + "\n")
    print("wrote", OUT)
