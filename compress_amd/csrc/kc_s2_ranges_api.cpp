// kc_s2_ranges_api.cpp — s2.ReadSeeker.ReadAt over a batch of (input, offset, length) requests: kc_s2_read_ranges[_dev] of
// include/kcgpu.h.
//
// One call: the host asks each request's index where to start (Index.Find; no index: the input's start) and lays the output out
// as the prefix sum of the lengths.  The ranged plan's first pass (kc_s2_ranges.hip) sizes every request — covered chunks, the bytes
// it will get, the scratch its clipped chunks take, the first header-level status; the requests then go through the second pass
// and the clipped decode in batches whose chunk records and clip slots fit the scratch budget.  The host settles every request as
// kc_s2_dec_api.cpp settles an input: the first failing covered chunk in stream order, else the plan's status; a failed request's
// whole range is zero-filled, a short read's tail is.
#include "kc_host.h"
#include "kc_s2_index.h"
#include "kc_s2_plan_dev.h"

namespace {

enum { SR_REQ = 8, SR_PLAN, SR_CHUNKS, SR_CSTATUS, SR_SLOTS };  // c->s2d[]

uint32_t max_buf_of(const kc_s2_ropts* o) { return (uint32_t)kc_s2_max_encoded_len((int64_t)o->max_block) + 4u; }  // Reader.maxBufSize (s2/reader.go:42)

const uint64_t kPerChunk = sizeof(KcS2RChunk) + 4;  // device scratch one covered chunk takes besides a slot: its record and its verdict

// R: every request resolved (where its walk starts); pre[j] != 0: settled on the host already (Find refused it), nothing of it goes
// to the device.  d_dst + out_off[j] is request j's range.
kc_status ranges_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const std::vector<KcS2Req>& R, const std::vector<uint32_t>& pre,
                     uint8_t* d_dst, const uint64_t* out_off, uint64_t* got, uint32_t* status) {
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last_batches = 0;
    const uint32_t m = (uint32_t)R.size();
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf* z = c->s2d;
    std::vector<uint32_t> live;  // the requests that reach the device
    std::vector<KcS2Req> Q;
    for (uint32_t j = 0; j < m; j++) {
        if (pre[j]) {
            status[j] = pre[j];
            got[j] = 0;
            if (R[j].len) HIPCHK(c, hipMemsetAsync(d_dst + out_off[j], 0, (size_t)R[j].len, st));
            continue;
        }
        live.push_back(j);
        Q.push_back(R[j]);
        Q.back().out0 = out_off[j];
    }
    const uint32_t n = (uint32_t)live.size();
    if (n == 0) {
        HIPCHK(c, hipStreamSynchronize(st));
        return KC_OK;
    }
    kc_status s;
    if ((s = ensure(c, z[SR_REQ], (size_t)n * sizeof(KcS2Req))) || (s = ensure(c, z[SR_PLAN], (size_t)n * sizeof(KcS2ReqPlan)))) return s;
    HIPCHK(c, hipMemcpyAsync(z[SR_REQ].p, Q.data(), (size_t)n * sizeof(KcS2Req), hipMemcpyHostToDevice, st));
    KcS2RangePlanParams P;
    memset(&P, 0, sizeof(P));
    P.src = d_src;
    P.reqs = (KcS2Req*)z[SR_REQ].p;
    P.m = n;
    P.max_block = o->max_block;
    P.max_buf = max_buf_of(o);
    P.ignore_id = o->ignore_id;
    P.plan = (KcS2ReqPlan*)z[SR_PLAN].p;
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    kc_launch_s2_range_plan(P, st);
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    std::vector<KcS2ReqPlan> H(n);
    HIPCHK(c, hipMemcpyAsync(H.data(), P.plan, (size_t)n * sizeof(KcS2ReqPlan), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
    c->last.prep_ms += t;
    const uint64_t budget = scratch_budget(c);
    std::vector<uint32_t> cstatus;
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: requests i0 .. i1 whose chunk records and clip slots fit the budget (ensure() over-allocates by 1/8) ----
        uint32_t i1 = i0, nc = 0;
        uint64_t slots = 0;
        while (i1 < n) {
            const uint64_t all = ((uint64_t)nc + H[i1].n_chunks) * kPerChunk + slots + H[i1].slot_bytes;
            if (i1 > i0 && (all + (all >> 3) > budget || (uint64_t)nc + H[i1].n_chunks > 0x3FFFFFFFu)) break;
            Q[i1].chunk0 = nc;
            Q[i1].slot0 = slots;
            nc += H[i1].n_chunks;
            slots += H[i1].slot_bytes;
            i1++;
        }
        const uint32_t nb = i1 - i0;
        if (nc) {
            if ((s = ensure(c, z[SR_CHUNKS], (size_t)nc * sizeof(KcS2RChunk))) || (s = ensure(c, z[SR_CSTATUS], (size_t)nc * 4)) ||
                (s = ensure(c, z[SR_SLOTS], (size_t)slots + 64)))
                return s;
            HIPCHK(c, hipMemcpyAsync((KcS2Req*)z[SR_REQ].p + i0, Q.data() + i0, (size_t)nb * sizeof(KcS2Req), hipMemcpyHostToDevice, st));
            KcS2RangePlanParams Q2 = P;  // second pass over this batch's requests: the records
            Q2.reqs = P.reqs + i0;
            Q2.m = nb;
            Q2.plan = nullptr;
            Q2.chunks = (KcS2RChunk*)z[SR_CHUNKS].p;
            KcS2RangeDecodeParams D;
            memset(&D, 0, sizeof(D));
            D.src = d_src;
            D.chunks = Q2.chunks;
            D.n_chunks = nc;
            D.dst = d_dst;
            D.slots = (uint8_t*)z[SR_SLOTS].p;
            D.ignore_crc = o->ignore_crc;
            D.status = (uint32_t*)z[SR_CSTATUS].p;
            HIPCHK(c, hipEventRecord(c->ev[0], st));
            kc_launch_s2_range_plan(Q2, st);
            HIPCHK(c, hipEventRecord(c->ev[1], st));
            kc_launch_s2_range_decode(D, st);
            HIPCHK(c, hipEventRecord(c->ev[2], st));
            cstatus.resize(nc);
            HIPCHK(c, hipMemcpyAsync(cstatus.data(), D.status, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            float t01 = 0, t12 = 0;
            (void)hipEventElapsedTime(&t01, c->ev[0], c->ev[1]);
            (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
            c->last.prep_ms += t01;
            c->last.match_ms += t12;
        }
        // ---- settle: the first failing covered chunk in stream order, else the plan's status (kc_s2_dec_api.cpp) ----
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
            if (g < len) HIPCHK(c, hipMemsetAsync(d_dst + out_off[j] + g, 0, (size_t)(len - g), st));
        }
        c->last_batches++;
        i0 = i1;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    c->last.total_ms = c->last.prep_ms + c->last.match_ms;
    return KC_OK;
}

// the arguments both forms check, the layout, and where every request starts (Index.Find)
kc_status resolve(kc_ctx* c, const kc_s2_ropts* o, const void* src, const uint64_t* in_off, uint32_t n_streams, const kc_s2_index* const* index,
                  const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len, uint32_t m, const void* dst, uint64_t dst_cap,
                  uint64_t* out_off, uint64_t* got, uint32_t* status, std::vector<KcS2Req>& R, std::vector<uint32_t>& pre) {
    if (!c || !o || !out_off || (n_streams && (!in_off || !src)) || (m && (!req_stream || !req_off || !req_len || !got || !status))) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    for (uint32_t i = 0; i < n_streams; i++)
        if (in_off[i + 1] < in_off[i]) { c->err = "in_off not ascending"; return KC_ERR_BAD_ARG; }
    out_off[0] = 0;
    for (uint32_t j = 0; j < m; j++) {
        if (req_stream[j] >= n_streams) { c->err = "a request names an input that does not exist"; return KC_ERR_BAD_ARG; }
        if (req_off[j] + req_len[j] < req_off[j] || out_off[j] + req_len[j] < out_off[j]) { c->err = "a request's range wraps"; return KC_ERR_BAD_ARG; }
        out_off[j + 1] = out_off[j] + req_len[j];
    }
    if (out_off[m] > dst_cap) { c->err = "dst_cap too small for the requests"; return KC_ERR_DST_TOO_SMALL; }  // (nothing written yet)
    if (out_off[m] && !dst) return KC_ERR_BAD_ARG;
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

}  // namespace

extern "C" {

kc_status kc_s2_read_ranges_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n_streams,
                                const kc_s2_index* const* index, const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len,
                                uint32_t m, uint8_t* d_dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* got, uint32_t* status) {
    std::vector<KcS2Req> R;
    std::vector<uint32_t> pre;
    try {
        kc_status s = resolve(c, o, d_src, in_off, n_streams, index, req_stream, req_off, req_len, m, d_dst, dst_cap, out_off, got, status, R, pre);
        if (s != KC_OK || m == 0) return s;
        return ranges_dev(c, o, d_src, R, pre, d_dst, out_off, got, status);
    } catch (const std::bad_alloc&) {
        c->err = "host memory exhausted";
        return KC_ERR_INTERNAL;
    }
}

// Host buffers: per request the compressed bytes from where its walk starts up to the first index entry at or above off + len (the
// input's end where the index has none) are staged back to back; groups of consecutive requests whose staged bytes and lengths fit
// a quarter of the scratch budget run as one device call each.
kc_status kc_s2_read_ranges(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n_streams,
                            const kc_s2_index* const* index, const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len, uint32_t m,
                            uint8_t* dst, uint64_t dst_cap, uint64_t* out_off, uint64_t* got, uint32_t* status) {
    std::vector<KcS2Req> R;
    std::vector<uint32_t> pre;
    try {
        kc_status s = resolve(c, o, src, in_off, n_streams, index, req_stream, req_off, req_len, m, dst, dst_cap, out_off, got, status, R, pre);
        if (s != KC_OK || m == 0) return s;
        for (uint32_t j = 0; j < m; j++) {  // the slice each request needs, and the reader's state at its start
            KcS2Req& q = R[j];
            if (pre[j]) { q.pos = q.end = q.front; continue; }
            if (q.flags & KC_S2R_MID) {
                bool snappy = false;
                const uint32_t f = kc_s2_front_state(src, q.front, q.end, o->ignore_id != 0, &snappy);
                if (f) { pre[j] = f; q.pos = q.end = q.front; continue; }
                q.flags |= KC_S2R_KNOWN | (snappy ? KC_S2R_SNAPPY : 0u);
            }
            const kc_s2_index* ix = index ? index[req_stream[j]] : nullptr;
            if (ix) {
                const uint64_t hi = q.off + q.len;
                const auto it = std::lower_bound(ix->u_off.begin(), ix->u_off.end(), hi, [](int64_t u, uint64_t h) { return (uint64_t)u < h; });
                if (it != ix->u_off.end()) {
                    const uint64_t ce = (uint64_t)ix->c_off[(size_t)(it - ix->u_off.begin())];
                    if (ce <= q.end - q.front && q.front + ce >= q.pos) q.end = q.front + ce;
                }
            }
        }
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t st = c->stream;
        kc_timings sum = {0, 0, 0, 0, 0, 0};
        int batches = 0;
        std::vector<uint8_t> stage;
        std::vector<KcS2Req> G;
        std::vector<uint32_t> gpre, gst;
        std::vector<uint64_t> goo, ggot;
        uint32_t i0 = 0;
        while (i0 < m) {
            const uint64_t quarter = scratch_budget(c) / 4;
            auto cost = [&](uint32_t j) { return (R[j].end - R[j].pos) + R[j].len; };
            if (cost(i0) > quarter) {
                status[i0] = KC_S2D_SIZE_EXCEEDED;
                got[i0] = 0;
                if (R[i0].len) memset(dst + out_off[i0], 0, (size_t)R[i0].len);
                i0++;
                continue;
            }
            uint32_t i1 = i0;
            uint64_t acc = 0;
            while (i1 < m && acc + cost(i1) <= quarter) acc += cost(i1++);
            const uint32_t nb = i1 - i0;
            stage.clear();
            G.assign(R.begin() + i0, R.begin() + i1);
            gpre.assign(pre.begin() + i0, pre.begin() + i1);
            goo.resize(nb + 1); ggot.resize(nb); gst.resize(nb);
            for (uint32_t k = 0; k < nb; k++) {
                KcS2Req& q = G[k];
                const uint64_t bytes = q.end - q.pos, at = stage.size();
                if (bytes) stage.insert(stage.end(), src + q.pos, src + q.end);
                q.front = q.pos = at;  // (a walk from the input's front starts at the slice's front; a later start knows its state)
                q.end = at + bytes;
                goo[k] = out_off[i0 + k] - out_off[i0];
            }
            goo[nb] = out_off[i1] - out_off[i0];
            const uint64_t need = goo[nb];
            if ((s = ensure(c, c->tmp_src, stage.size() + 64)) || (s = ensure(c, c->tmp_dst, (size_t)need + 64))) return s;
            if (!stage.empty()) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
            if ((s = ranges_dev(c, o, (const uint8_t*)c->tmp_src.p, G, gpre, (uint8_t*)c->tmp_dst.p, goo.data(), ggot.data(), gst.data())) != KC_OK) return s;
            if (need) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            for (uint32_t k = 0; k < nb; k++) { status[i0 + k] = gst[k]; got[i0 + k] = ggot[k]; }
            sum.prep_ms += c->last.prep_ms; sum.match_ms += c->last.match_ms; sum.total_ms += c->last.total_ms;
            batches += c->last_batches;
            i0 = i1;
        }
        c->last = sum;
        c->last_batches = batches;
        return KC_OK;
    } catch (const std::bad_alloc&) {
        c->err = "host memory exhausted";
        return KC_ERR_INTERNAL;
    }
}

}  // extern "C"
