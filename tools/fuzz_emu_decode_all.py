"""Differential fuzz of the device DecodeAll against the reference's own (translated) DecodeAll on mutated frames, on the CPU: the
whole library built for the wave emulator (tools/build_emu_lib.sh; ASAN=1 for the memory-error hunt).  The seeded form of this is
tests/test_gpu_zstd_decode_all.py::test_differential_on_mutations; here any number of seeds, checksummed frames and dictionary
frames included.

    tools/build_emu_lib.sh && KC_LIB_TAG=emu python tools/fuzz_emu_decode_all.py [first_seed [n_seeds [mutations_per_frame]]]
"""
import os
import random
import sys
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("KC_LIB_TAG", "").startswith("emu"), "runs against the emulator build of the library (KC_LIB_TAG=emu)"

import numpy as np  # noqa: E402

import oracle_goref as G  # noqa: E402
from compress_amd import _lib, zstd  # noqa: E402

REFIN = os.path.join(ROOT, "tests", "golden", "ref_inputs")
CAP = 1 << 20


def mutate(rng, f):
    m = bytearray(f)
    kind = rng.randrange(4)
    if kind == 0:
        p = rng.randrange(len(m) * 8)
        m[p >> 3] ^= 1 << (p & 7)
    elif kind == 1:
        m = m[:rng.randrange(len(m))]
    elif kind == 2:
        m[rng.randrange(len(m))] = rng.randrange(256)
    else:  # two flips: one may repair what the other broke in a size field
        for _ in range(2):
            p = rng.randrange(min(len(m), 64) * 8)
            m[p >> 3] ^= 1 << (p & 7)
    return bytes(m)


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    nseeds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    tw = open(os.path.join(REFIN, "Mark.Twain-Tom.Sawyer.txt"), "rb").read()
    frames = []
    for n in (1, 300, 5000, 70000, 140000):
        for level in (1, 2, 3):
            for crc in (False, True):
                frames.append((G.zstd_encode_all(tw[1000:1000 + n], level=level, crc=crc), None))
                frames.append((G.zstd_encode_stream(tw[1000:1000 + n], level=level, crc=crc), None))
    zf = zipfile.ZipFile(os.path.join(REFIN, "dict-tests-small.zip"))
    dicts = {int.from_bytes(zf.read(m)[4:8], "little"): zf.read(m) for m in zf.namelist() if m.endswith(".dict")}
    for m in zf.namelist():
        if m.endswith(".zst") and zf.getinfo(m).file_size < 40000:
            z = zf.read(m)
            fhd = z[4]
            p = 5 + (0 if (fhd >> 5) & 1 else 1)
            frames.append((z, dicts[int.from_bytes(z[p:p + [0, 1, 2, 4][fhd & 3]], "little")]))
    bad = 0
    for seed in range(first, first + nseeds):
        rng = random.Random(seed)
        for blob in [None] + list(dicts.values()):
            cases = [mutate(rng, f) for f, d in frames if d is blob for _ in range(per)]
            opts = [zstd.WithDecoderMaxMemory(CAP)] + ([zstd.WithDecoderDicts(blob)] if blob else [])
            dec = zstd.NewReader(None, *opts)
            off = np.zeros(len(cases) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(c) for c in cases])
            out, oo, st = dec.DecodeUnits(np.frombuffer(b"".join(cases) + b"\0", dtype=np.uint8), off)
            dec.Close()
            acc = 0
            for i, c in enumerate(cases):
                try:
                    ref = G.zstd_decode_all(c, CAP, dict_blob=blob) if blob else G.zstd_decode_all(c, CAP)
                    err = None
                except ValueError as e:
                    ref, err = None, str(e)
                got = out[int(oo[i]):int(oo[i + 1])].tobytes()
                if ref is not None:
                    acc += 1
                    if st[i] != 0 or got != ref:
                        bad += 1
                        print("seed %d case %d: reference returns %d bytes, device %s / %d bytes: %s" % (seed, i, len(ref), _lib.ZD_NAMES[int(st[i])], len(got), c[:24].hex()))
                elif st[i] == 0:
                    bad += 1
                    print("seed %d case %d: reference refuses (%s), device returns %d bytes: %s" % (seed, i, err, len(got), c[:24].hex()))
            print("seed %d dict %s: %d cases, %d accepted by the reference, %d disagreements so far" % (seed, "yes" if blob else "no", len(cases), acc, bad), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
