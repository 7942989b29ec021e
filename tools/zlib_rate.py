"""What the zlib container costs on the device: the SAME DEFLATE bodies inflated raw (kc_flate_inflate_dev), as gzip members
(kc_gzip_inflate_dev: CRC-32 in the write pass) and as zlib streams (kc_zlib_inflate_dev: Adler-32 in the write pass), in one run
on one box, beside a plain device copy of the decoded bytes.  GPU only.

  workload: 8 192 members of 128 KiB of corpus T, deflated by zlib at levels 1 and 9, device-resident, one wave per member

Per level one child process under its own time limit: warm-up, then the four calls alternating, device events around each call, the
sizing pass and the write pass read from kc_last_timings (prep_ms / match_ms).  Every measurement — the median of --reps calls — is
REPEATED three times in that process; the spread between the three repeats of one measurement is the margin within which two
measurements count as equal.  The first child that fails, faults or runs out of time ends the run, and what was measured until then
is written with `stopped_at`.  Nothing here is a threshold: the file is the record.

--ab-old DIR: a checkout of the parent commit with its library built (tools/ab_old_new.sh's tools/_ab/old).  The raw flate call is
then measured in child processes that alternate between DIR's library and this tree's (old, new, old, new), level 1, to show that
the flate kernels were not disturbed.

    python tools/zlib_rate.py [--reps 5] [--members 8192] [--ab-old tools/_ab/old] [--out profiles/zlib_batch.json]
"""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBER = 128 << 10
LIMIT_S = 300
REPEATS = 3


def _deflate(args):
    import zlib
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def prepare(level, members, path):
    """The members deflated by zlib in spawned worker processes (no child ever holds the device) -> a file the measuring children read."""
    import multiprocessing
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import corpora
    host = corpora.corpus("T", members, MEMBER)
    parts = [host[i * MEMBER:(i + 1) * MEMBER].tobytes() for i in range(members)]
    with multiprocessing.get_context("spawn").Pool(min(12, os.cpu_count() or 1)) as pool:   # (the writer is not what is measured)
        raw = pool.map(_deflate, [(p, level) for p in parts], chunksize=64)
    with open(path, "wb") as f:
        pickle.dump((host.tobytes(), raw), f)


def measure(path, level, reps, root, flate_only):
    import struct
    import zlib
    import numpy as np
    sys.path.insert(0, root)   # the tree whose library is measured
    with open(path, "rb") as f:
        host, raw = pickle.load(f)
    members, total = len(raw), len(host)
    parts = [host[i * MEMBER:(i + 1) * MEMBER] for i in range(members)]
    import torch
    from compress_amd import flate
    assert torch.cuda.is_available(), "a measurement needs the GPU"

    def pack(xs):
        off = np.zeros(len(xs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in xs])
        return torch.from_numpy(np.frombuffer(b"".join(xs), dtype=np.uint8).copy()).cuda(0), off

    d_ref = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).cuda(0)
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    d_cpy = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    batches = {"flate": (flate.Batch("kc_flate_inflate", flate._ERRORS),) + pack(raw)}
    if not flate_only:
        from compress_amd import gzip, zlib as kzlib
        gz = [b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + r + struct.pack("<II", zlib.crc32(p), len(p)) for r, p in zip(raw, parts)]
        zl = [b"\x78\x9c" + r + struct.pack(">I", zlib.adler32(p)) for r, p in zip(raw, parts)]
        batches["gzip"] = (flate.Batch("kc_gzip_inflate", gzip._ERRORS),) + pack(gz)
        batches["zlib"] = (flate.Batch("kc_zlib_inflate", kzlib._ERRORS),) + pack(zl)

    def product(b, d_in, off):
        def f():
            oo, st, _ = b.inflate(d_in.data_ptr(), off, d_out.data_ptr(), total, True)
            assert not st.any() and int(oo[-1]) == total
        return f

    runs = {k: product(*v) for k, v in batches.items()}
    runs["copy"] = lambda: d_cpy.copy_(d_ref)

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
    med = statistics.median
    repeats = []
    for _ in range(REPEATS):
        t = {k: [] for k in runs}
        size_ms, write_ms = {k: [] for k in batches}, {k: [] for k in batches}
        for _ in range(reps):
            for k, fn in runs.items():
                t[k].append(timed(fn))
                if k in batches:
                    tm = batches[k][0].ctx().timings()
                    size_ms[k].append(tm["prep_ms"])
                    write_ms[k].append(tm["match_ms"])
        repeats.append({"call_ms": {k: med(v) for k, v in t.items()}, "sizing_pass_ms": {k: med(v) for k, v in size_ms.items()},
                        "write_pass_ms": {k: med(v) for k, v in write_ms.items()}})
    for b in batches.values():
        b[0].close()

    def across(key):
        out = {}
        for k in repeats[0][key]:
            v = [r[key][k] for r in repeats]
            out[k] = {"repeats": v, "median": med(v), "spread": max(v) - min(v)}
        return out

    res = {"what": "%d members of %d KiB (corpus T, zlib level %d), device-resident, one wave per member; ms between device events; every "
                   "figure the median of %d calls, repeated %d times" % (members, MEMBER >> 10, level, reps, REPEATS),
           "members": members, "decoded_bytes": total, "deflate_bytes": sum(len(r) for r in raw), "library": os.path.relpath(root, ROOT),
           "call_ms": across("call_ms"), "sizing_pass_ms": across("sizing_pass_ms"), "write_pass_ms": across("write_pass_ms"),
           "device": torch.cuda.get_device_name(0)}
    if not flate_only:
        w = res["write_pass_ms"]
        res["write_pass_over_raw_ms"] = {k: w[k]["median"] - w["flate"]["median"] for k in ("gzip", "zlib")}
        res["write_pass_spread_ms"] = max(w[k]["spread"] for k in ("flate", "gzip", "zlib"))
        res["write_pass_GBps"] = {k: total / w[k]["median"] / 1e6 for k in w}
    return res


def child(args, limit=LIMIT_S):
    """-> (exit code, the RESULT of a measuring child or None, the end of its output)"""
    with tempfile.TemporaryFile("w+") as log:
        try:
            code = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=log, stderr=subprocess.STDOUT, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            code = 124
        log.seek(0)
        text = log.read()
    line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
    return code, (json.loads(line[-1][len("RESULT "):]) if code == 0 and line else None), text[-2000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--ab-old", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zlib_batch.json"))
    ap.add_argument("--prepare", help="(child) deflate the members into this file")
    ap.add_argument("--measure", help="(child) measure over this file and print the JSON")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--flate-only", action="store_true")
    a = ap.parse_args()
    if a.prepare:
        prepare(a.level, a.members, a.prepare)
        return 0
    if a.measure:
        print("RESULT " + json.dumps(measure(a.measure, a.level, a.reps, os.path.abspath(a.root), a.flate_only)))
        return 0
    res = {"levels": {}}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(str(lv), lv, ROOT, False) for lv in (1, 9)]
        if a.ab_old:
            jobs += [("%s-%d" % (w, k), 1, os.path.abspath(a.ab_old) if w == "old" else ROOT, True) for k in (1, 2) for w in ("old", "new")]
        have = None
        for name, level, root, flate_only in jobs:
            path = os.path.join(tmp, "members-%d.pkl" % level)
            if have != level:   # (not on the device: the members of one level are deflated once)
                code, _, tail = child(["--prepare", path, "--level", str(level), "--members", str(a.members)])
                have = level
            if code == 0:
                code, r, tail = child(["--measure", path, "--level", str(level), "--reps", str(a.reps), "--root", root] + (["--flate-only"] if flate_only else []))
            if code != 0 or r is None:  # a fault, an abort, a failed assertion or the time limit: nothing more is started on the device
                res["stopped_at"] = {"job": name, "exit": code, "tail": tail}
                break
            print("measured: %s" % name, flush=True)
            if flate_only:
                res.setdefault("raw_flate_old_vs_new", {})[name] = {k: r[k]["flate"] for k in ("call_ms", "sizing_pass_ms", "write_pass_ms")}
            else:
                res["levels"][name] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({lv: {k: r[k] for k in ("write_pass_over_raw_ms", "write_pass_spread_ms", "write_pass_GBps")} for lv, r in res["levels"].items()}))
    print(json.dumps(res.get("raw_flate_old_vs_new", {})))
    if "stopped_at" in res:
        print(json.dumps(res["stopped_at"]))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
