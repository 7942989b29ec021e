"""The S2 stream reader against DecodeStreams on one long stream: corpus J through the device's own s2.Writer at block sizes 64 KiB,
1 MiB (the writer's default) and 4 MiB — the shape a `.s2` file has — read by s2.StreamReader (kc_s2_rstream_feed: one window of up to
KC_OPT_S2_RSTREAM_CHUNKS data chunks per launch, one wave per chunk) with a dst of 32 MiB, 256 MiB and 1 GiB and 64 / 256 / 1024 / 4096
chunks per launch, alternating with Reader.DecodeStreams of the same stream as one call (before the stream reader the only way to
decode it here).  Same process, warm-up first (its output compared byte for byte with the source), host clocks around calls that end
in a synchronise, median and spread of at least 7 repetitions.  The shares of H2D, kernel and D2H come from one decode in a child
process under `rocprofv3 --kernel-trace --memory-copy-trace --stats` (no counters), under a time limit.

    python tools/s2_stream_rate.py [--mib 1024] [--reps 7] [--out profiles/s2_stream_reader.json]
"""
import argparse
import csv
import glob
import io
import json
import os
import signal
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

from compress_amd import _lib, s2  # noqa: E402
import corpora  # noqa: E402

BLOCKS = (64 << 10, 1 << 20, 4 << 20)
DSTS = (32 << 20, 256 << 20, 1 << 30)
CHUNKS = (64, 256, 512, 1024, 4096)  # (512: what a 32 MiB dst caps a window of 64 KiB blocks at)
KERNEL = "kc_s2_rstream_kernel"


def make_stream(src, block):
    w = io.BytesIO()
    sw = s2.NewWriter(w, s2.WriterBlockSize(block), device=0)
    step = 64 << 20
    for i in range(0, len(src), step):
        sw.Write(src[i:i + step])
    sw.Close()
    return w.getvalue()


def open_reader(z, dst, chunks):
    rd = s2.NewStreamReader(io.BytesIO(b""), batch_bytes=dst)
    rd.ctx().set_option(_lib.OPT_S2_RSTREAM_CHUNKS, chunks)
    rd.Reset(io.BytesIO(z))  # (a stream takes the option when it is made)
    return rd


def profile_shares(mib, block, dst, chunks):
    """One decode under the profiler, in a child process: device time of the kernel and of the copies in each direction."""
    with tempfile.TemporaryDirectory() as t:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", t, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--mib", str(mib), "--one-pass", "%d,%d,%d" % (block, dst, chunks)]
        # a session of its own: at the time limit the whole group goes, the profiler and the process under it that holds the GPU
        pr = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
        try:
            log, _ = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            os.killpg(pr.pid, signal.SIGKILL)
            pr.wait()
            return {"error": "the profiled run did not end within its time limit"}
        if pr.returncode != 0:
            return {"error": "rocprofv3 run failed (%d): %s" % (pr.returncode, log.decode(errors="replace")[-400:])}
        ns = {"kernel": 0, "h2d": 0, "d2h": 0}
        n = {"kernel": 0, "h2d": 0, "d2h": 0}
        for f in glob.glob(t + "/**/*kernel_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                if row["Kernel_Name"].startswith(KERNEL):
                    ns["kernel"] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    n["kernel"] += 1
        for f in glob.glob(t + "/**/*memory_copy_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                d = row.get("Direction", "").upper()
                k = "h2d" if "HOST_TO_DEVICE" in d else "d2h" if "DEVICE_TO_HOST" in d else None
                if k:
                    ns[k] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    n[k] += 1
        total = sum(ns.values())
        if ns["kernel"] == 0:
            return {"error": "no dispatch of %s in the trace" % KERNEL}
        return {k: {"ms": ns[k] / 1e6, "count": n[k], "share": ns[k] / total} for k in ns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_stream_reader.json"))
    ap.add_argument("--one-pass", default=None, help="block,dst,chunks: encode, read once with the reader, compare (the profiler's run)")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    src = corpora.corpus("J", a.mib * 16, 64 << 10).tobytes()
    if a.one_pass:
        block, dst, chunks = (int(x) for x in a.one_pass.split(","))
        rd = open_reader(make_stream(src, block), dst, chunks)
        out = bytearray(len(src))
        assert rd.Read(out) == len(src) and bytes(out) == src
        rd.Close()
        return

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = statistics.median
    rows = []
    whole = s2.NewReader(None, device=0)
    for block in BLOCKS:
        z = make_stream(src, block)
        zin, zoff = np.frombuffer(z, dtype=np.uint8), np.array([0, len(z)], dtype=np.uint64)
        got = {}

        def decode_streams():
            got["o"] = whole.DecodeStreams(zin, zoff)[0]

        decode_streams()  # warm-up, and whether the one call is served at all
        refused = got["o"].name if isinstance(got["o"], s2.S2DecodeError) else None
        if refused is None:
            assert got["o"] == src, "DecodeStreams differs from the source"
        got.clear()
        for dst in DSTS:
            for chunks in CHUNKS:
                rd = open_reader(z, dst, chunks)
                out = bytearray(len(src))
                assert rd.Read(out) == len(src) and rd.Read(bytearray(1)) == 0 and bytes(out) == src, "the reader's bytes differ from the source"
                tr, ta = [], []

                def reader():  # Reset keeps the stream, its device window and the host buffer; like DecodeStreams it leaves 1 x the bytes in host memory
                    rd.Reset(io.BytesIO(z))
                    assert rd.Read(out) == len(src)

                for _ in range(max(a.reps, 7)):
                    tr.append(timed(reader))
                    if refused is None:
                        ta.append(timed(decode_streams))
                        got.clear()
                assert bytes(out) == src
                del out
                rd.Close()
                row = {"block": block, "dst": dst, "chunks": chunks, "encoded_bytes": len(z),
                       "reader_ms": {"median": med(tr), "min": min(tr), "max": max(tr), "spread": max(tr) - min(tr)},
                       "reader_decoded_GBps": len(src) / med(tr) / 1e6}
                if refused is None:
                    row["decode_streams_ms"] = {"median": med(ta), "min": min(ta), "max": max(ta), "spread": max(ta) - min(ta)}
                    row["decode_streams_decoded_GBps"] = len(src) / med(ta) / 1e6
                else:
                    row["decode_streams"] = "refused: " + refused
                rows.append(row)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out + ".partial", "w") as f:  # (a run that is cut short leaves what it measured)
                    json.dump({"rows": rows}, f)
                print("block %d dst %d chunks %d: reader %.1f ms (spread %.1f)%s" % (block, dst, chunks, med(tr), max(tr) - min(tr),
                      ", DecodeStreams %.1f ms" % med(ta) if ta else ", DecodeStreams " + str(refused)), file=sys.stderr, flush=True)
    whole.Close()
    # the default of KC_OPT_S2_RSTREAM_CHUNKS: the smallest value within the run-to-run spread of the best rate at 64 KiB blocks
    small = [r for r in rows if r["block"] == BLOCKS[0]]
    best = {c: min((r for r in small if r["chunks"] == c), key=lambda r: r["reader_ms"]["median"]) for c in CHUNKS}
    top = min(best.values(), key=lambda r: r["reader_ms"]["median"])
    spread = max(r["reader_ms"]["spread"] for r in best.values())
    default = min(c for c in CHUNKS if best[c]["reader_ms"]["median"] <= top["reader_ms"]["median"] + spread)
    by_dst = {}
    for r in rows:
        if r["block"] == 1 << 20:
            by_dst.setdefault(r["dst"], []).append(r["reader_decoded_GBps"])
    res = {
        "what": "one stream of %d MiB of corpus J from the device's s2.Writer per block size, host buffers in and out, ms per read of the "
                "whole stream on host clocks with the device synchronised; the reader keeps its stream, device window and host buffer over the "
                "repetitions (Reset) and fills one preallocated buffer, DecodeStreams returns a new bytes object" % a.mib,
        "decoded_bytes": len(src), "reps": max(a.reps, 7), "rows": rows,
        "default_chunks": {"value": default, "best_ms_per_chunks_at_64KiB": {str(c): best[c]["reader_ms"]["median"] for c in CHUNKS}, "spread_ms": spread,
                           "rule": "the smallest value whose best median at 64 KiB blocks lies within the largest run-to-run spread of the best one"},
        "rate_grows_with_dst_at_1MiB_blocks": {"best_GBps_per_dst": {str(d): max(v) for d, v in by_dst.items()},
                                               "confirmed": all(max(by_dst[DSTS[i]]) < max(by_dst[DSTS[i + 1]]) for i in range(len(DSTS) - 1))},
        "shares": {"not collected": True} if a.no_profile else profile_shares(a.mib, 1 << 20, 256 << 20, default),
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    os.remove(a.out + ".partial")
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "rows")}))


if __name__ == "__main__":
    main()
