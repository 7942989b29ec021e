// kc_s2_ranges_api.cpp — s2.ReadSeeker.ReadAt over a batch of (input, offset, length) requests: kc_s2_read_ranges[_dev] of
// include/kcgpu.h.  The sequence of one device call is kc_s2ranges_host.h's; this file gives it the device (HipDevice over
// kc_ctx::s2r), checks the arguments and serves host buffers.
#include "kc_decdev_hip.h"
#include "kc_s2ranges_host.h"
#include "kc_s2_plan_dev.h"

namespace {

static_assert(SR_N == sizeof(kc_ctx::s2r) / sizeof(DevBuf), "kc_ctx::s2r has one slot per SR_* buffer");

kc_status ranges_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const std::vector<KcS2Req>& R, const std::vector<uint32_t>& pre,
                     uint8_t* d_dst, const uint64_t* out_off, uint64_t* got, uint32_t* status) {
    KcDecTimes T;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->s2r);
    return take_outcome(c, T, kc_s2r_read(&dev, mode_of(o), d_src, R, pre, d_dst, out_off, got, status, T), "");
}

// the arguments both forms check, the layout, and where every request starts (Index.Find)
kc_status resolve(kc_ctx* c, const kc_s2_ropts* o, const void* src, const uint64_t* in_off, uint32_t n_streams, const kc_s2_index* const* index,
                  const uint32_t* req_stream, const uint64_t* req_off, const uint64_t* req_len, uint32_t m, const void* dst, uint64_t dst_cap,
                  uint64_t* out_off, uint64_t* got, uint32_t* status, std::vector<KcS2Req>& R, std::vector<uint32_t>& pre) {
    if (!c || !o || !out_off || (m && (!req_stream || !req_off || !req_len || !got || !status))) return KC_ERR_BAD_ARG;
    const uint64_t none = 0;  // (no inputs: their offsets may be absent)
    kc_status s = check_batch_args(c, src, n_streams || in_off ? in_off : &none, n_streams);
    if (s != KC_OK) return s;
    const char* why = "";
    if ((s = (kc_status)kc_s2r_resolve(in_off, n_streams, index, req_stream, req_off, req_len, m, dst_cap, out_off, R, pre, &why)) != KC_OK) {
        c->err = why;
        return s;
    }
    if (out_off[m] && !dst) return KC_ERR_BAD_ARG;
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
        GroupSum sum;
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
            sum.add(c);
            i0 = i1;
        }
        sum.give(c);
        return KC_OK;
    } catch (const std::bad_alloc&) {
        c->err = "host memory exhausted";
        return KC_ERR_INTERNAL;
    }
}

}  // extern "C"
