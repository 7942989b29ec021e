#pragma once
// kc_s2ranges_host.h — host side of s2.ReadSeeker.ReadAt over a batch of (input, offset, length) requests, written against
// KcDecDevice alone (kc_s2_ranges_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator over plain memory).
//
// One call: the host asks each request's index where to start (Index.Find; no index: the input's start) and lays the output out
// as the prefix sum of the lengths.  The ranged plan's first pass (kc_s2_ranges.hip) sizes every request — covered chunks, the bytes
// it will get, the scratch its clipped chunks take, the first header-level status; the requests then go through the second pass
// and the clipped decode in batches whose chunk records and clip slots fit the scratch budget.  The host settles every request as
// kc_s2dec_host.h settles an input: the first failing covered chunk in stream order, else the plan's status; a failed request's
// whole range is zero-filled, a short read's tail is.
#include <limits.h>
#include "kc_s2_index.h"
#include "kc_s2dec_host.h"

enum { SR_REQ, SR_PLAN, SR_CHUNKS, SR_CSTATUS, SR_SLOTS, SR_N };

// The layout, and where every request starts (Index.Find).  R: every request resolved; pre[j] != 0: settled here already (Find
// refused it), nothing of it goes to the device.  Returns KC_OK, or KC_ERR_BAD_ARG / KC_ERR_DST_TOO_SMALL with *why (nothing written).
static inline int kc_s2r_resolve(const uint64_t* in_off, uint32_t n_streams, const kc_s2_index* const* index, const uint32_t* req_stream,
                                 const uint64_t* req_off, const uint64_t* req_len, uint32_t m, uint64_t dst_cap, uint64_t* out_off,
                                 std::vector<KcS2Req>& R, std::vector<uint32_t>& pre, const char** why) {
    out_off[0] = 0;
    for (uint32_t j = 0; j < m; j++) {
        if (req_stream[j] >= n_streams) { *why = "a request names an input that does not exist"; return KC_ERR_BAD_ARG; }
        if (req_off[j] + req_len[j] < req_off[j] || out_off[j] + req_len[j] < out_off[j]) { *why = "a request's range wraps"; return KC_ERR_BAD_ARG; }
        out_off[j + 1] = out_off[j] + req_len[j];
    }
    if (out_off[m] > dst_cap) { *why = "dst_cap too small for the requests"; return KC_ERR_DST_TOO_SMALL; }
    R.resize(m);
    pre.assign(m, 0);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t s = req_stream[j];
        KcS2Req& q = R[j];
        memset(&q, 0, sizeof(q));
        q.front = in_off[s]; q.end = in_off[s + 1]; q.pos = q.front;
        q.off = req_off[j]; q.len = req_len[j];
        const kc_s2_index* ix = index ? index[s] : nullptr;
        if (!ix) continue;
        int64_t cc = 0, uu = 0;
        const int rc = q.off > (uint64_t)INT64_MAX ? (int)KC_S2I_UNEXPECTED_EOF : kc_s2_index_find(ix, (int64_t)q.off, &cc, &uu);
        if (rc) { pre[j] = (uint32_t)rc; continue; }
        if (cc > 0) {  // (0: the walk starts at the input's front, identifier and all)
            q.pos = (uint64_t)cc > q.end - q.front ? q.end : q.front + (uint64_t)cc;
            q.flags = KC_S2R_MID;
        }
        q.u = (uint64_t)uu;
    }
    return KC_OK;
}

static const uint64_t kS2rPerChunk = sizeof(KcS2RChunk) + 4;  // device scratch one covered chunk takes besides a slot: its record and its verdict

// d_dst + out_off[j] is request j's range.
static inline int kc_s2r_read(KcDecDevice* dev, const KcS2dMode& o, const uint8_t* d_src, const std::vector<KcS2Req>& R, const std::vector<uint32_t>& pre,
                              uint8_t* d_dst, const uint64_t* out_off, uint64_t* got, uint32_t* status, KcDecTimes& T) {
    const uint32_t m = (uint32_t)R.size();
    std::vector<uint32_t> live;  // the requests that reach the device
    std::vector<KcS2Req> Q;
    int s;
    for (uint32_t j = 0; j < m; j++) {
        if (pre[j]) {
            status[j] = pre[j];
            got[j] = 0;
            if (R[j].len && (s = dev->zero(d_dst + out_off[j], (size_t)R[j].len))) return s;
            continue;
        }
        live.push_back(j);
        Q.push_back(R[j]);
        Q.back().out0 = out_off[j];
    }
    const uint32_t n = (uint32_t)live.size();
    if (n == 0) return dev->sync();
    KcS2RangePlanParams P;
    memset(&P, 0, sizeof(P));
    if ((s = kc_dec_reserve(dev, SR_REQ, n, &P.reqs)) || (s = kc_dec_reserve(dev, SR_PLAN, n, &P.plan)) ||
        (s = dev->h2d(P.reqs, Q.data(), (size_t)n * sizeof(KcS2Req))))
        return s;
    P.src = d_src;
    P.m = n;
    P.max_block = o.max_block;
    P.max_buf = o.max_buf;
    P.ignore_id = o.ignore_id;
    std::vector<KcS2ReqPlan> H;
    if ((s = dev->mark(0))) return s;
    kc_launch_s2_range_plan(P, dev->stream);
    if ((s = dev->mark(1)) || (s = kc_dec_fetch(dev, H, (const KcS2ReqPlan*)P.plan, n)) || (s = dev->sync())) return s;
    T.prep_ms += dev->span(0, 1);
    const uint64_t budget = dev->budget();
    std::vector<uint32_t> cstatus;
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: requests i0 .. i1 whose chunk records and clip slots fit the budget (reserve() may over-allocate by 1/8) ----
        uint32_t i1 = i0, nc = 0;
        uint64_t slots = 0;
        while (i1 < n) {
            const uint64_t all = ((uint64_t)nc + H[i1].n_chunks) * kS2rPerChunk + slots + H[i1].slot_bytes;
            kc_dec_need(T, (uint64_t)H[i1].n_chunks * kS2rPerChunk + H[i1].slot_bytes);
            if (i1 > i0 && (all + (all >> 3) > budget || (uint64_t)nc + H[i1].n_chunks > 0x3FFFFFFFu)) break;
            Q[i1].chunk0 = nc;
            Q[i1].slot0 = slots;
            nc += H[i1].n_chunks;
            slots += H[i1].slot_bytes;
            i1++;
        }
        const uint32_t nb = i1 - i0;
        if (nc) {
            KcS2RangePlanParams Q2 = P;  // second pass over this batch's requests: the records
            KcS2RangeDecodeParams D;
            memset(&D, 0, sizeof(D));
            if ((s = kc_dec_reserve(dev, SR_CHUNKS, nc, &Q2.chunks)) || (s = kc_dec_reserve(dev, SR_CSTATUS, nc, &D.status)) ||
                (s = kc_dec_reserve(dev, SR_SLOTS, (size_t)slots + 64, &D.slots)) || (s = dev->h2d(P.reqs + i0, Q.data() + i0, (size_t)nb * sizeof(KcS2Req))))
                return s;
            Q2.reqs = P.reqs + i0;
            Q2.m = nb;
            Q2.plan = nullptr;
            D.src = d_src;
            D.chunks = Q2.chunks;
            D.n_chunks = nc;
            D.dst = d_dst;
            D.ignore_crc = o.ignore_crc;
            if ((s = dev->mark(0))) return s;
            kc_launch_s2_range_plan(Q2, dev->stream);
            if ((s = dev->mark(1))) return s;
            kc_launch_s2_range_decode(D, dev->stream);
            if ((s = dev->mark(2)) || (s = kc_dec_fetch(dev, cstatus, (const uint32_t*)D.status, nc)) || (s = dev->sync())) return s;
            T.prep_ms += dev->span(0, 1);
            T.match_ms += dev->span(1, 2);
        }
        // ---- settle: the first failing covered chunk in stream order, else the plan's status (kc_s2dec_host.h) ----
        for (uint32_t i = i0; i < i1; i++) {
            const uint32_t j = live[i];
            const uint64_t len = Q[i].len;
            uint32_t v = KCS2D_OK;
            for (uint32_t k = 0; k < H[i].n_chunks && !v; k++) v = cstatus[Q[i].chunk0 + k];
            if (!v) v = H[i].status;
            status[j] = v;
            uint64_t g = (v == KCS2D_OK || v == KCS2D_EOF) ? H[i].got : 0;
            if (g > len) g = len;
            got[j] = g;
            if (g < len && (s = dev->zero(d_dst + out_off[j] + g, (size_t)(len - g)))) return s;
        }
        T.batches++;
        i0 = i1;
    }
    return dev->sync();
}
