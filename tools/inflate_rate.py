"""Device inflate rate of the flate / gzip batch path (kc_flate_inflate_dev, kc_gzip_inflate_dev: no sizes supplied, sizing pass +
write pass, gzip with CRC-32) beside a plain device copy of the decoded bytes and zlib.decompress on one host thread of the same
box.  GPU only.

  workload: 8 192 members of 128 KiB of corpus T, deflated by zlib at levels 1 and 9, device-resident, one wave per member

Per level, same process, warm-up first, alternating, device events around each call; the sizing pass and the write pass are read from
kc_last_timings (prep_ms / match_ms).  Each level runs in a child process of its own under its own time limit; the first one that
fails, faults or runs out of time ends the run, and what was measured until then is written with `stopped_at`.  Nothing here is a
threshold: the file is the record.

    python tools/inflate_rate.py [--reps 7] [--members 8192] [--out profiles/inflate_batch.json]
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


def _deflate(args):
    import zlib
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def measure(level, members, reps):
    import multiprocessing
    import struct
    import zlib
    import numpy as np
    import corpora
    # The members are deflated by zlib in worker processes BEFORE this process touches the GPU (torch.cuda is first used below), and
    # the workers are spawned, not forked: no child ever holds the device.
    host = corpora.corpus("T", members, MEMBER)
    total = members * MEMBER
    parts = [host[i * MEMBER:(i + 1) * MEMBER].tobytes() for i in range(members)]
    with multiprocessing.get_context("spawn").Pool(min(12, os.cpu_count() or 1)) as pool:   # (the writer is not what is measured)
        raw = pool.map(_deflate, [(p, level) for p in parts], chunksize=64)
    gz = [b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + r + struct.pack("<II", zlib.crc32(p), len(p)) for r, p in zip(raw, parts)]
    import torch
    from compress_amd import flate, gzip
    assert torch.cuda.is_available(), "a measurement needs the GPU"

    def pack(xs):
        off = np.zeros(len(xs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in xs])
        return torch.from_numpy(np.frombuffer(b"".join(xs), dtype=np.uint8).copy()).cuda(0), off

    d_raw, off_raw = pack(raw)
    d_gz, off_gz = pack(gz)
    d_ref = torch.from_numpy(host).cuda(0)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    d_cpy = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    bf = flate.Batch("kc_flate_inflate", flate._ERRORS)
    bg = flate.Batch("kc_gzip_inflate", gzip._ERRORS)

    def product(b, d_in, off):
        def f():
            oo, st, _ = b.inflate(d_in.data_ptr(), off, d_out.data_ptr(), total, True)
            assert not st.any() and int(oo[-1]) == total
        return f

    runs = {"flate": product(bf, d_raw, off_raw), "gzip": product(bg, d_gz, off_gz), "copy": lambda: d_cpy.copy_(d_ref)}
    ctx = {"flate": bf, "gzip": bg}

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
    size_ms, write_ms = {"flate": [], "gzip": []}, {"flate": [], "gzip": []}
    for _ in range(max(reps, 5)):
        for k, fn in runs.items():
            t[k].append(timed(fn))
            if k in ctx:
                tm = ctx[k].ctx().timings()
                size_ms[k].append(tm["prep_ms"])
                write_ms[k].append(tm["match_ms"])
    sample = raw[:max(1, members // 16)]    # one host thread of the same box: a sixteenth of the members, three rounds
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        for r in sample:
            zlib.decompress(r, -15)
        host_s.append(time.perf_counter() - t0)
    med = statistics.median
    res = {
        "what": "%d members of %d KiB (corpus T, zlib level %d), device-resident, one wave per member; ms per call between device events" % (members, MEMBER >> 10, level),
        "members": members, "decoded_bytes": total, "deflate_bytes": int(off_raw[-1]), "reps": len(t["copy"]),
        "ms": {k: stats(v) for k, v in t.items()},
        "decoded_GBps": {k: total / med(v) / 1e6 for k, v in t.items()},
        "sizing_pass_ms": {k: stats(v) for k, v in size_ms.items()},
        "write_pass_ms": {k: stats(v) for k, v in write_ms.items()},
        "sizing_pass_GBps": {k: total / med(v) / 1e6 for k, v in size_ms.items()},
        "write_pass_GBps": {k: total / med(v) / 1e6 for k, v in write_ms.items()},
        "fraction_of_copy_rate": {k: med(t["copy"]) / med(v) for k, v in t.items() if k != "copy"},
        "zlib_one_host_thread_GBps": len(sample) * MEMBER / med(host_s) / 1e9,
        "device": torch.cuda.get_device_name(0),
    }
    bf.close()
    bg.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_batch.json"))
    ap.add_argument("--level", type=int, help="(child) measure this zlib level and print its JSON")
    a = ap.parse_args()
    if a.level is not None:
        print("RESULT " + json.dumps(measure(a.level, a.members, a.reps)))
        return 0
    res = {"levels": {}}
    rc = 0
    for level in (1, 9):
        with tempfile.TemporaryFile("w+") as log:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--level", str(level), "--reps", str(a.reps), "--members", str(a.members)],
                                   stdout=log, stderr=subprocess.STDOUT, timeout=LIMIT_S)
                code = p.returncode
            except subprocess.TimeoutExpired:
                code = 124
            log.seek(0)
            text = log.read()
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if code != 0 or not line:  # a fault, an abort, a failed assertion or the time limit: nothing more is started on the device
            res["stopped_at"] = {"level": level, "exit": code, "tail": text[-2000:]}
            rc = 1
            break
        res["levels"][str(level)] = json.loads(line[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({lv: {k: v for k, v in r.items() if k in ("decoded_GBps", "sizing_pass_GBps", "write_pass_GBps", "zlib_one_host_thread_GBps")}
                      for lv, r in res["levels"].items()}))
    if rc:
        print(json.dumps(res["stopped_at"]))
    return rc


if __name__ == "__main__":
    sys.exit(main())
