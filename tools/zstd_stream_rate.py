"""Stream reader against DecodeAll on one frame of many blocks: 256 MiB of corpus T through the device's own Encoder.Write / Close
(SpeedFastest, checksum on) — the shape a `.zst` file has — decoded by zstd.NewReader(r) (kc_zstd_dstream_feed: every block's entropy
stage on a wave of its own, one wave executing in order) and, alternating with it, by DecodeAll of the same frame (one wave for the
whole frame: before the stream reader the only way to decode it here).  Same process, warm-up first, host clocks around calls with
the device synchronised on both sides, outputs compared byte for byte.  The three kernels' shares of the reader's device time come from
a second run of this script in a process of its own under `rocprofv3 --kernel-trace --stats` (one decode, nothing else traced).

    python tools/zstd_stream_rate.py [--mib 256] [--reps 7] [--out profiles/zstd_stream_reader.json]
"""
import argparse
import csv
import glob
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from compress_amd import zstd  # noqa: E402
import corpora  # noqa: E402

KERNELS = ("kc_zstd_dstream_entropy_kernel", "kc_zstd_dstream_execute_kernel", "kc_xxh64_stream_kernel")


def make_frame(mib):
    src = corpora.corpus("T", mib * 8, 128 << 10).tobytes()
    w = io.BytesIO()
    enc = zstd.NewWriter(w, zstd.WithEncoderLevel(zstd.SpeedFastest), zstd.WithEncoderCRC(True))
    enc.Write(src)
    enc.Close()
    return src, w.getvalue()


def read_stream(d, z, out):
    d.Reset(io.BytesIO(z))
    n = d._sb.read_into(out)
    assert n == len(out) and d.Read(bytearray(1)) == 0
    return n


def kernel_shares(mib):
    """One decode under the profiler, in a child process; device time per kernel from the dispatch trace."""
    with tempfile.TemporaryDirectory() as t:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", t, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--mib", str(mib), "--one-pass"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        if r.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (r.returncode, r.stdout.decode(errors="replace")[-400:])}
        ns = {k: 0 for k in KERNELS}
        calls = {k: 0 for k in KERNELS}
        for f in glob.glob(t + "/**/*kernel_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if row["Kernel_Name"].startswith(k):
                        ns[k] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                        calls[k] += 1
        total = sum(ns.values())
        if total == 0:
            return {"error": "no dispatch of the three kernels in the trace"}
        return {k: {"ms": ns[k] / 1e6, "dispatches": calls[k], "share": ns[k] / total} for k in KERNELS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_stream_reader.json"))
    ap.add_argument("--one-pass", action="store_true", help="encode, decode once with the reader, compare (the profiler's run)")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    src, z = make_frame(a.mib)
    out = bytearray(len(src))
    rd = zstd.NewReader(None)
    if a.one_pass:
        read_stream(rd, z, out)
        assert bytes(out) == src
        rd.Close()
        return
    da = zstd.NewReader(None, zstd.WithDecoderMaxMemory(len(src)))
    zin, zoff = np.frombuffer(z, dtype=np.uint8), np.array([0, len(z)], dtype=np.uint64)

    def reader():
        read_stream(rd, z, out)

    got = {}

    def decode_all():
        o, _, st = da.DecodeUnits(zin, zoff)
        assert st[0] == 0 and len(o) == len(src)
        got["o"] = o

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    reader()  # warm-up: code objects, scratch growth
    decode_all()
    print("warm-up done", file=sys.stderr, flush=True)
    assert bytes(out) == src and got["o"].tobytes() == src, "decoded bytes differ from the source"
    tr, ta = [], []
    for _ in range(max(a.reps, 7)):
        tr.append(timed(reader))
        ta.append(timed(decode_all))
        print("rep %d: reader %.1f ms, DecodeAll %.1f ms" % (len(tr), tr[-1], ta[-1]), file=sys.stderr, flush=True)
    assert bytes(out) == got["o"].tobytes()
    med = statistics.median
    spread = max(max(tr) - min(tr), max(ta) - min(ta))
    res = {
        "what": "one stream frame of %d MiB (corpus T, SpeedFastest, checksum on, %d bytes encoded), host buffers in and out, ms per "
                "decode on host clocks with the device synchronised" % (a.mib, len(z)),
        "decoded_bytes": len(src), "encoded_bytes": len(z), "reps": len(tr),
        "reader_ms": {"median": med(tr), "min": min(tr), "max": max(tr), "spread": max(tr) - min(tr), "all": tr},
        "decode_all_ms": {"median": med(ta), "min": min(ta), "max": max(ta), "spread": max(ta) - min(ta), "all": ta},
        "spread_ms": spread,
        "reader_decoded_GBps": len(src) / med(tr) / 1e6,
        "decode_all_decoded_GBps": len(src) / med(ta) / 1e6,
        "reader_below_decode_all_by_more_than_the_spread": med(tr) + spread < med(ta),
        "reader_kernels": {"not collected": True} if a.no_profile else kernel_shares(a.mib),
        "note": "the executor runs a launch's blocks in order on one wave: it bounds the reader once the entropy stage is spread over the blocks",
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "what"}))
    rd.Close()
    da.Close()


if __name__ == "__main__":
    main()
