"""Device rate of the stateless writers (kc_flate_stateless_deflate_dev, kc_gzip_stateless_deflate_dev: match, plan, chain and emit
kernels) beside the HuffmanOnly writer on the same bodies, a plain device copy of the same bytes and CPython's zlib at level 1 on one
host thread of the same box.  GPU only.

  workload: the 8 192 bodies of 128 KiB of corpus T that tools/deflate_rate.py writes, device-resident

Same process, warm-up first, alternating, device events around each call; the four kernels are read from kc_last_timings (match =
match_ms, plan = prep_ms, chain = other_ms, emit = entropy_ms; the zero-fill of dst lies between them and is in the call's time only).
The measurement runs in a child process under a time limit; if it fails, faults or runs out of time, nothing more is started on the
device and what happened is written as `stopped_at`.  zlib's level 1 writes other bytes (a 32 KiB window carried through the whole
body): it is context, not a yardstick.  Nothing here is a threshold: the file is the record.

    python tools/stateless_rate.py [--reps 3] [--members 8192] [--out profiles/stateless_batch.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MEMBER = 128 << 10
LIMIT_S = 420


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def measure(members, reps):
    import zlib
    import numpy as np
    import corpora
    host = corpora.corpus("T", members, MEMBER)
    total = members * MEMBER
    off = (np.arange(members + 1, dtype=np.uint64) * MEMBER)
    import torch
    from compress_amd import flate
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    d_src = torch.from_numpy(host).cuda(0)
    cap = members * (max(flate.DeflateBound(MEMBER), flate.StatelessBound(MEMBER)) + 20)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_cpy = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    b = {"flate": flate.StatelessBatch("kc_flate_stateless_deflate"), "gzip": flate.StatelessBatch("kc_gzip_stateless_deflate"),
         "huffman_only": flate.WriteBatch("kc_flate_deflate")}
    sizes = {}

    def product(k):
        def f():
            sizes[k] = int(b[k].deflate(d_src.data_ptr(), off, d_out.data_ptr(), cap, True)[-1])
        return f

    runs = {"flate": product("flate"), "gzip": product("gzip"), "huffman_only": product("huffman_only"), "copy": lambda: d_cpy.copy_(d_src)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for k, fn in runs.items():  # warm-up: code objects, scratch growth; and the bytes are right (a sample through zlib on the host)
        fn()
        torch.cuda.synchronize()
    oo = b["gzip"].deflate(d_src.data_ptr(), off, d_out.data_ptr(), cap, True)
    out = d_out[:int(oo[-1])].cpu().numpy()
    for i in range(0, members, max(1, members // 64)):
        got = zlib.decompress(out[int(oo[i]):int(oo[i + 1])].tobytes(), 31)
        assert got == host[i * MEMBER:(i + 1) * MEMBER].tobytes(), "the device's stream does not decode to its input"
    t = {k: [] for k in runs}
    kern = {k: {"match": [], "plan": [], "chain": [], "emit": []} for k in ("flate", "gzip")}
    for _ in range(max(reps, 3)):
        for k, fn in runs.items():
            t[k].append(timed(fn))
            if k in kern:
                tm = b[k].ctx().timings()
                kern[k]["match"].append(tm["match_ms"])
                kern[k]["plan"].append(tm["prep_ms"])
                kern[k]["chain"].append(tm["other_ms"])
                kern[k]["emit"].append(tm["entropy_ms"])
    n_host = max(1, members // 16)  # one host thread of the same box: a sixteenth of the bodies, three rounds
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(n_host):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            host_out = len(c.compress(host[i * MEMBER:(i + 1) * MEMBER].tobytes())) + len(c.flush())
        host_s.append(time.perf_counter() - t0)
    med = statistics.median
    res = {
        "what": "%d bodies of %d KiB (corpus T), device-resident, StatelessDeflate (blocks of 32767 then 24575 bytes), one wave per block in "
                "match, plan and emit, one wave per body in chain; ms per call between device events; huffman_only: kc_flate_deflate_dev on the "
                "same bodies" % (members, MEMBER >> 10),
        "members": members, "input_bytes": total, "output_bytes": sizes, "reps": len(t["copy"]),
        "ms": {k: stats(v) for k, v in t.items()},
        "input_GBps": {k: total / med(v) / 1e6 for k, v in t.items()},
        "ms_per_GiB": {k: med(v) * (1 << 30) / total for k, v in t.items()},
        "kernel_ms": {k: {p: stats(v) for p, v in ks.items()} for k, ks in kern.items()},
        "fraction_of_copy_rate": {k: med(t["copy"]) / med(v) for k, v in t.items() if k != "copy"},
        "ratio": {k: v / total for k, v in sizes.items()},
        "spread_max_over_min": {k: max(v) / min(v) for k, v in t.items()},
        "zlib_level_1_one_host_thread_GBps": n_host * MEMBER / med(host_s) / 1e9,
        "zlib_level_1_ratio_last_body": host_out / MEMBER,
        "device": torch.cuda.get_device_name(0),
    }
    for x in b.values():
        x.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stateless_batch.json"))
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.members, a.reps)))
        return 0
    res, rc = {}, 0
    with tempfile.TemporaryFile("w+") as log:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--members", str(a.members)],
                               stdout=log, stderr=subprocess.STDOUT, timeout=LIMIT_S)
            code = p.returncode
        except subprocess.TimeoutExpired:
            code = 124
        log.seek(0)
        text = log.read()
    line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
    if code != 0 or not line:  # a fault, an abort, a failed assertion or the time limit
        res["stopped_at"] = {"exit": code, "tail": text[-2000:]}
        rc = 1
    else:
        res = json.loads(line[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k in ("input_GBps", "ms_per_GiB", "kernel_ms", "stopped_at", "ratio", "zlib_level_1_one_host_thread_GBps")}))
    return rc


if __name__ == "__main__":
    sys.exit(main())
