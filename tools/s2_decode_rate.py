"""Device decode rate of the S2 product path (kc_s2_decode_streams_dev: no sizes supplied, plan + decode + CRC + verdict) beside the
verifier (kc_s2_decode_blocks_dev: given every block's decoded length, no CRC) and a plain device copy of the decoded bytes, on streams
the device encoder wrote.  GPU only.

  shape A: 8 192 J-corpus blocks of 64 KiB as one framed stream (EncodeStreamDevice); the verifier on the same blocks as bare blocks
  shape B: 256 MiB of T-corpus as chunks of 1 MiB, one framed stream

Per shape, same process, warm-up first, alternating, device events around each call: the product path with ignore_crc, the product path
with CRC, (shape A) the verifier, the copy.  Each shape runs in a child process of its own under its own time limit; the first shape
that fails, faults or runs out of time ends the run, and what was measured until then is written with `stopped_at`.

    python tools/s2_decode_rate.py [--reps 9] [--out profiles/s2_decode_all.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"A": ("J", 8192, 64 << 10), "B": ("T", 256, 1 << 20)}
LIMIT_S = {"A": 240, "B": 240}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}


def measure(shape, reps):
    import numpy as np
    import torch
    from compress_amd import s2
    import corpora
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    kind, n, bs = SHAPES[shape]
    host = corpora.corpus(kind, n, bs)
    total = n * bs
    off = np.arange(n + 1, dtype=np.uint64) * bs
    d_src = torch.from_numpy(host).cuda(0)
    enc = s2.BlockEncoder(level=s2.LevelDefault)
    cap = n * ((s2.MaxEncodedLen(bs) + 8 + 15) & ~15) + 64
    d_stream = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    soff = enc.EncodeStreamDevice(d_src.data_ptr(), off, d_stream.data_ptr(), cap)
    in_off = np.array([0, int(soff[-1])], dtype=np.uint64)
    rd_crc = s2.NewReader(None)
    rd_nocrc = s2.NewReader(None, s2.ReaderIgnoreCRC())
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    d_ver = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    d_cpy = torch.zeros(total, dtype=torch.uint8, device="cuda:0")

    def product(rd):
        def f():
            oo, st = rd.DecodeStreamsDevice(d_stream.data_ptr(), in_off, d_out.data_ptr(), total)
            assert not st.any() and int(oo[-1]) == total
        return f

    runs = {"product_ignore_crc": product(rd_nocrc), "product_crc": product(rd_crc), "copy": lambda: d_cpy.copy_(d_src)}
    if shape == "A":  # the verifier is the unchanged yardstick: the same blocks, bare, every size supplied
        d_blk = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        boff = enc.EncodeBlocksDevice(d_src.data_ptr(), off, d_blk.data_ptr(), cap)

        def verifier():
            st = enc.DecodeBlocksDevice(d_blk.data_ptr(), boff, d_ver.data_ptr(), off)
            assert not st.any()
        runs["verifier"] = verifier

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):  # warm-up: code objects, scratch growth
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_src), "decoded bytes differ from the source"
    assert shape != "A" or torch.equal(d_ver, d_src)
    t = {k: [] for k in runs}
    plan, decode = [], []
    for _ in range(max(reps, 7)):
        for k, fn in runs.items():
            t[k].append(timed(fn))
            if k == "product_ignore_crc":
                tm = rd_nocrc.ctx().timings()
                plan.append(tm["prep_ms"])
                decode.append(tm["match_ms"])
    med = statistics.median
    res = {
        "what": "%d blocks of %d KiB (corpus %s, default level) as one framed stream, device-resident, ms per call between device events" % (n, bs >> 10, kind),
        "blocks": n, "decoded_bytes": total, "encoded_bytes": int(soff[-1]), "reps": len(t["copy"]),
        "ms": {k: stats(v) for k, v in t.items()},
        "decoded_GBps": {k: total / med(v) / 1e6 for k, v in t.items()},
        "fraction_of_copy_rate": {k: med(t["copy"]) / med(v) for k, v in t.items() if k != "copy"},
        "plan_kernel_ms": stats(plan),   # both passes: one lane walks all chunk headers of the stream in sequence
        "decode_kernel_ms": stats(decode),
        "device": torch.cuda.get_device_name(0),
    }
    if shape == "A":
        spread = max(res["ms"]["verifier"]["spread"], res["ms"]["product_ignore_crc"]["spread"])
        res["product_ignore_crc_over_verifier"] = med(t["product_ignore_crc"]) / med(t["verifier"])
        res["within_bar"] = med(t["product_ignore_crc"]) <= med(t["verifier"]) + spread
    enc.Close()
    rd_crc.Close()
    rd_nocrc.Close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_decode_all.json"))
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(child) measure this shape and print its JSON")
    a = ap.parse_args()
    if a.shape:
        print("RESULT " + json.dumps(measure(a.shape, a.reps)))
        return 0
    res = {"parse": "uniform: the tag stream parsed once per wave (the window parse of the design was not built, so there is no second median)", "shapes": {}}
    rc = 0
    for shape in sorted(SHAPES):
        with tempfile.TemporaryFile("w+") as log:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape, "--reps", str(a.reps)], stdout=log, stderr=subprocess.STDOUT,
                                   timeout=LIMIT_S[shape])
                code = p.returncode
            except subprocess.TimeoutExpired:
                code = 124
            log.seek(0)
            text = log.read()
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if code != 0 or not line:  # a fault, an abort, a failed assertion or the time limit: nothing more is started on the device
            res["stopped_at"] = {"shape": shape, "exit": code, "tail": text[-2000:]}
            rc = 1
            break
        res["shapes"][shape] = json.loads(line[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({s: {k: v for k, v in r.items() if k in ("decoded_GBps", "fraction_of_copy_rate", "within_bar", "product_ignore_crc_over_verifier")}
                      for s, r in res["shapes"].items()}))
    if rc:
        print(json.dumps(res["stopped_at"]))
    return rc


if __name__ == "__main__":
    sys.exit(main())
