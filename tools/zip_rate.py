"""Device rate of the zip reader (kc_zip_read_dev: locate, inflate / store, finish; the directory states the sizes, one pass) beside
flate.InflateAllDevice on the same bodies laid end to end (no sizes supplied: sizing pass + write pass) and a plain device copy of
the decoded bytes.  GPU only.

  deflated: one archive of 8 192 members of 128 KiB of corpus T, deflated by zlib at level 6, device-resident, one wave per member
  stored:   the same bytes as 16 stored members of 64 MiB: one wave per 64 KiB chunk, the chunk CRCs combined per member

All arms of a workload run in the same process, warm-up first, alternating, three repeats, device events around each call; the
kernels apart are read from kc_last_timings (zip: prep_ms locate, match_ms inflate + store, other_ms finish; flate: prep_ms the
sizing pass, match_ms the write pass).  Each workload runs in a child process of its own under its own time limit; the first one
that fails, faults or runs out of time ends the run, and what was measured until then is written with `stopped_at`.  Nothing here
is a threshold: the file is the record.

    python tools/zip_rate.py [--reps 3] [--members 8192] [--out profiles/zip_batch.json]
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

MEMBER = 128 << 10
LIMIT_S = 420


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def _deflate(args):
    import zlib
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def measure(kind, members, reps):
    import multiprocessing
    import numpy as np
    import corpora
    import zip_builder as B
    host = corpora.corpus("T", members, MEMBER)
    total = members * MEMBER
    raw = None
    if kind == "deflated":
        # deflated by zlib in worker processes BEFORE this process touches the GPU; the workers are spawned: no child holds the device
        parts = [host[i * MEMBER:(i + 1) * MEMBER].tobytes() for i in range(members)]
        with multiprocessing.get_context("spawn").Pool(min(12, os.cpu_count() or 1)) as pool:
            raw = pool.map(_deflate, [(p, 6) for p in parts], chunksize=64)
        ms = [B.M("t/%05d.txt" % i, p, body=r) for i, (p, r) in enumerate(zip(parts, raw))]
    else:
        n_big = 16
        step = total // n_big
        ms = [B.M("big/%02d.bin" % i, host[i * step:(i + 1) * step].tobytes(), method=0) for i in range(n_big)]
    archive, _ = B.build(ms)
    del ms
    import torch
    from compress_amd import flate, zip as kzip
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    r = kzip.NewReader(archive)
    d_arc = torch.from_numpy(np.frombuffer(archive, dtype=np.uint8).copy()).cuda(0)
    d_ref = torch.from_numpy(host).cuda(0)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    d_cpy = torch.zeros(total, dtype=torch.uint8, device="cuda:0")

    def zip_read():
        oo, st = r.ReadAllDevice(d_arc.data_ptr(), d_out.data_ptr(), total)
        assert not st.any() and int(oo[-1]) == total

    runs = {"zip": zip_read, "copy": lambda: d_cpy.copy_(d_ref)}
    ctx = {"zip": r.ctx()}
    if raw is not None:
        off = np.zeros(len(raw) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in raw])
        d_raw = torch.from_numpy(np.frombuffer(b"".join(raw), dtype=np.uint8).copy()).cuda(0)
        bf = flate.Batch("kc_flate_inflate", flate._ERRORS)

        def flate_two_passes():
            oo, st, _ = bf.inflate(d_raw.data_ptr(), off, d_out.data_ptr(), total, True)
            assert not st.any() and int(oo[-1]) == total

        runs["flate"] = flate_two_passes
        ctx["flate"] = bf.ctx()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for k, fn in runs.items():  # warm-up: code objects, scratch growth; and the bytes are right
        d_out.zero_()
        fn()
        torch.cuda.synchronize()
        assert k == "copy" or torch.equal(d_out, d_ref), "decoded bytes differ from the source"
    t = {k: [] for k in runs}
    parts_ms = {k: {"prep_ms": [], "match_ms": [], "other_ms": []} for k in ctx}
    for _ in range(max(reps, 3)):
        for k, fn in runs.items():
            t[k].append(timed(fn))
            if k in ctx:
                tm = ctx[k].timings()
                for f in parts_ms[k]:
                    parts_ms[k][f].append(tm[f])
    med = statistics.median
    names = {"zip": {"prep_ms": "locate", "match_ms": "inflate" if kind == "deflated" else "store", "other_ms": "finish"},
             "flate": {"prep_ms": "sizing_pass", "match_ms": "write_pass", "other_ms": "other"}}
    res = {
        "what": ("%d members of %d KiB (corpus T, zlib level 6)" % (members, MEMBER >> 10) if kind == "deflated" else "16 stored members of %d MiB (corpus T)" % (total >> 24))
        + ", device-resident; ms per call between device events, the kernels apart from kc_last_timings",
        "decoded_bytes": total, "archive_bytes": len(archive), "reps": len(t["copy"]),
        "ms": {k: stats(v) for k, v in t.items()},
        "decoded_GBps": {k: total / med(v) / 1e6 for k, v in t.items()},
        "kernels_ms": {k: {names[k][f]: stats(v) for f, v in p.items()} for k, p in parts_ms.items()},
        "fraction_of_copy_rate": {k: med(t["copy"]) / med(v) for k, v in t.items() if k != "copy"},
        "device": torch.cuda.get_device_name(0),
    }
    if "flate" in t:
        res["single_pass_over_two_passes"] = med(t["flate"]) / med(t["zip"])
    r.Close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zip_batch.json"))
    ap.add_argument("--kind", help="(child) measure this workload and print its JSON")
    a = ap.parse_args()
    if a.kind is not None:
        print("RESULT " + json.dumps(measure(a.kind, a.members, a.reps)))
        return 0
    res = {"workloads": {}}
    rc = 0
    for kind in ("deflated", "stored"):
        with tempfile.TemporaryFile("w+") as log:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", kind, "--reps", str(a.reps), "--members", str(a.members)],
                                   stdout=log, stderr=subprocess.STDOUT, timeout=LIMIT_S)
                code = p.returncode
            except subprocess.TimeoutExpired:
                code = 124
            log.seek(0)
            text = log.read()
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if code != 0 or not line:  # a fault, an abort, a failed assertion or the time limit: nothing more is started on the device
            res["stopped_at"] = {"workload": kind, "exit": code, "tail": text[-2000:]}
            rc = 1
            break
        res["workloads"][kind] = json.loads(line[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {f: v for f, v in r.items() if f in ("decoded_GBps", "single_pass_over_two_passes", "fraction_of_copy_rate")} for k, r in res["workloads"].items()}))
    if rc:
        print(json.dumps(res["stopped_at"]))
    return rc


if __name__ == "__main__":
    sys.exit(main())
