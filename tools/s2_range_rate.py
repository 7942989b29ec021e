"""Rate of ranged reads through the S2 index (kc_s2_read_ranges_dev) beside the only way to get the same bytes without them: decoding
the streams whole (kc_s2_decode_streams_dev).  GPU only; not a test.

  64 device-resident streams of 16 MiB (J corpus, 256 blocks of 64 KiB each, written by the device encoder), each with the index
  IndexStream builds for it (the Writer's: one entry per MiB); 8 192 requests of 4 KiB at seeded offsets.

Same process, warm-up first, alternating, wall-clock around each synchronous call (the calls return when their results are on the
host).  Writes both medians and their ratio.

    python tools/s2_range_rate.py [--reps 7] [--out profiles/s2_read_ranges.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_STREAMS, N_BLOCKS, BS, N_REQ, REQ_LEN, SEED = 64, 256, 64 << 10, 8192, 4096, 0x52D0003


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2_read_ranges.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from compress_amd import s2
    import corpora
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    per = N_BLOCKS * BS
    blk_off = np.arange(N_BLOCKS + 1, dtype=np.uint64) * BS
    enc = s2.BlockEncoder(level=s2.LevelDefault)
    cap = N_BLOCKS * ((s2.MaxEncodedLen(BS) + 8 + 15) & ~15) + 64
    d_one = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    parts, indexes, in_off, sources = [], [], [0], []
    for k in range(N_STREAMS):
        host = corpora.corpus("J", N_BLOCKS, BS, first_unit=k * N_BLOCKS)
        d_src = torch.from_numpy(host).cuda(0)
        oo = enc.EncodeStreamDevice(d_src.data_ptr(), blk_off, d_one.data_ptr(), cap)
        part = d_one[:int(oo[-1])].clone()
        ix = s2.Index()
        ix.Load(s2.IndexStream(part.cpu().numpy().tobytes()))
        assert len(ix.info) == per >> 20
        parts.append(part)
        indexes.append(ix)
        in_off.append(in_off[-1] + part.numel())
        sources.append(d_src)
    enc.Close()
    d_streams = torch.cat(parts)
    del parts
    in_off = np.array(in_off, dtype=np.uint64)
    rnd = random.Random(SEED)
    requests = [(rnd.randrange(N_STREAMS), rnd.randrange(per - REQ_LEN), REQ_LEN) for _ in range(N_REQ)]
    d_rng = torch.zeros(N_REQ * REQ_LEN, dtype=torch.uint8, device="cuda:0")
    d_all = torch.zeros(N_STREAMS * per, dtype=torch.uint8, device="cuda:0")
    rd = s2.NewReader(None)

    def ranged():
        _, got, st = rd.ReadRangesDevice(d_streams.data_ptr(), in_off, requests, d_rng.data_ptr(), d_rng.numel(), indexes)
        assert not st.any() and int(got.sum()) == N_REQ * REQ_LEN

    def whole():
        oo, st = rd.DecodeStreamsDevice(d_streams.data_ptr(), in_off, d_all.data_ptr(), d_all.numel())
        assert not st.any() and int(oo[-1]) == N_STREAMS * per

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):  # warm-up: code objects, scratch growth
        ranged()
        whole()
    for j in rnd.sample(range(N_REQ), 64):  # the bytes, against the source
        s, off, ln = requests[j]
        assert torch.equal(d_rng[j * REQ_LEN:(j + 1) * REQ_LEN], sources[s][off:off + ln]), j
    tr, tw = [], []
    for _ in range(a.reps):
        tr.append(timed(ranged))
        tw.append(timed(whole))
    rd.Close()
    res = {"shape": {"streams": N_STREAMS, "stream_bytes": per, "block": BS, "requests": N_REQ, "request_bytes": REQ_LEN, "seed": SEED,
                     "compressed_bytes": int(in_off[-1])},
           "read_ranges_ms": stats(tr), "decode_whole_ms": stats(tw),
           "ratio_whole_over_ranges": statistics.median(tw) / statistics.median(tr),
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shape"}))


if __name__ == "__main__":
    main()
