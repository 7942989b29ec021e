"""Device decode rate: the product path (kc_zstd_decode_all_dev: no sizes supplied, plan + decode + checksum + compaction) beside the
verifier (kc_zstd_decode_units_dev: given every frame's decoded length), on frames the device encoder wrote — corpus T, units of
128 KiB, SpeedFastest, checksum on.  Same process, warm-up first, the two alternating, device events around each call, outputs
compared byte for byte.  Writes the medians, the spread of each, the plan kernel's share and the decoded GB/s as JSON.

    python tools/decode_rate.py [--units 8192] [--reps 9] [--out profiles/zstd_decode_all.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from compress_amd import zstd  # noqa: E402
import corpora  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_decode_all.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, usz = a.units, 128 << 10
    host = corpora.corpus("T", n, usz)
    off = np.arange(n + 1, dtype=np.uint64) * usz
    d_src = torch.from_numpy(host).cuda(0)
    enc = zstd.NewWriter(None, zstd.WithEncoderLevel(zstd.SpeedFastest))
    cap = n * ((enc.MaxEncodedSize(usz) + 15) & ~15) + 64
    d_enc = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    eoff = enc.EncodeUnitsDevice(d_src.data_ptr(), off, d_enc.data_ptr(), cap)
    dec = zstd.NewReader(None)
    d_ver = torch.zeros(n * usz, dtype=torch.uint8, device="cuda:0")
    d_all = torch.zeros(n * usz, dtype=torch.uint8, device="cuda:0")

    def verifier():
        st = enc.DecodeUnitsDevice(d_enc.data_ptr(), eoff, d_ver.data_ptr(), off)
        assert not st.any()

    def product():
        oo, st = dec.DecodeAllDevice(d_enc.data_ptr(), eoff, d_all.data_ptr(), n * usz)
        assert not st.any() and np.array_equal(oo, off)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):  # warm-up: code objects, scratch growth
        verifier()
        product()
    assert torch.equal(d_ver, d_src) and torch.equal(d_all, d_src), "decoded bytes differ from the source"
    tv, tp, plan, decode, other = [], [], [], [], []
    for _ in range(max(a.reps, 7)):
        tv.append(timed(verifier))
        tp.append(timed(product))
        t = dec.ctx().timings()
        plan.append(t["prep_ms"]); decode.append(t["match_ms"]); other.append(t["other_ms"])
    assert torch.equal(d_ver, d_all)
    med = statistics.median
    res = {
        "what": "decode of %d frames of 128 KiB (corpus T, SpeedFastest, checksum on), device-resident, ms per call between device events" % n,
        "units": n, "decoded_bytes": n * usz, "encoded_bytes": int(eoff[n]), "reps": len(tv),
        "verifier_ms": {"median": med(tv), "min": min(tv), "max": max(tv), "spread": max(tv) - min(tv), "all": tv},
        "decode_all_ms": {"median": med(tp), "min": min(tp), "max": max(tp), "spread": max(tp) - min(tp), "all": tp},
        "decode_all_kernels_ms": {"plan": med(plan), "decode": med(decode), "checksum_and_compaction": med(other)},
        "plan_share_of_kernel_time": med(plan) / (med(plan) + med(decode) + med(other)),
        "verifier_decoded_GBps": n * usz / med(tv) / 1e6,
        "decode_all_decoded_GBps": n * usz / med(tp) / 1e6,
        "decode_all_over_verifier": med(tp) / med(tv),
        "within_bar": med(tp) <= med(tv) + max(max(tv) - min(tv), max(tp) - min(tp)),
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "what"}))
    enc.Close()
    dec.Close()


if __name__ == "__main__":
    main()
