// kc_stateless_api.cpp — flate.StatelessDeflate / gzip.NewWriterLevel(w, gzip.StatelessCompression) over a batch of independent inputs:
// the options and the entry points kc_flate_stateless_deflate[_dev] / kc_gzip_stateless_deflate[_dev] / kc_flate_stateless_bound of
// include/kcgpu.h.  The sequence of one device call is kc_stateless_host.h's; this file gives it the device (HipDevice over
// kc_ctx::sl), checks the arguments and serves host buffers.
#include "kc_decdev_hip.h"
#include "kc_stateless_host.h"

struct kc_flate_swopts {
    KcSlOpts o;
};

namespace {

static_assert(SL_N == sizeof(kc_ctx::sl) / sizeof(DevBuf), "kc_ctx::sl has one slot per SL_* buffer");

kc_status check_args(kc_ctx* c, const kc_flate_swopts* o, const void* src, const uint64_t* in_off, uint32_t n, const void* dst, uint64_t dst_cap,
                     const uint64_t* out_off) {
    if (!out_off || !o) return KC_ERR_BAD_ARG;
    const kc_status s = check_batch_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    return n && !dst && dst_cap ? KC_ERR_BAD_ARG : KC_OK;
}

KcSlOpts opts_of(const kc_flate_swopts* o, uint32_t gzip) {
    KcSlOpts f = o->o;
    f.gzip = gzip;
    if (gzip) f.dict.clear();  // the reference's gzip writer passes nil
    return f;
}

const char* const TOO_SMALL = "dst_cap below the exact size of the batch";

// take_outcome, and the emit kernel's time where kc_timings has the bitstream kernels (match_ms: match, prep_ms: plan, other_ms: chain)
kc_status outcome(kc_ctx* c, const KcDecTimes& T, int s, const char* too_small) {
    const kc_status r = take_outcome(c, T, s, too_small);
    c->last.entropy_ms = T.emit_ms;
    if (r == KC_OK) c->last.total_ms += T.emit_ms;
    return r;
}

kc_status deflate_dev(kc_ctx* c, const kc_flate_swopts* o, uint32_t gzip, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                      uint64_t dst_cap, uint64_t* out_off) {
    kc_status s = check_args(c, o, d_src, in_off, n, d_dst, dst_cap, out_off);
    if (s != KC_OK) return s;
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->sl);
    return outcome(c, T, kc_sl_deflate(&dev, opts_of(o, gzip), d_src, in_off, n, d_dst, dst_cap, out_off, T), TOO_SMALL);
}

// Host buffers: groups of inputs, cut between inputs, whose bytes and bound together stay within a tenth of the scratch budget (one
// input at least; the device sequence takes four more bytes of tokens per byte); each group is staged, written into the context's
// output staging by the device sequence, and copied out.
kc_status deflate_host(kc_ctx* c, const kc_flate_swopts* o, uint32_t gzip, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* out_off) {
    kc_status s = check_args(c, o, src, in_off, n, dst, dst_cap, out_off);
    if (s != KC_OK) return s;
    KcDecTimes T;
    (void)take_outcome(c, T, KC_OK, "");
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->sl);
    const KcSlOpts f = opts_of(o, gzip);
    const uint64_t part = scratch_budget(c) / 10;
    auto cost = [&](uint32_t i) { const uint64_t len = in_off[i + 1] - in_off[i]; return len + kc_sl_bound(len, f.dict.size()) + (gzip ? KCSL_GZIP_EXTRA : 0); };
    std::vector<uint64_t> rel, oo;
    for (uint32_t i0 = 0; i0 < n;) {
        uint64_t sum = cost(i0);
        uint32_t i1 = i0 + 1;
        while (i1 < n && sum + cost(i1) <= part) sum += cost(i1++);
        const uint64_t in_bytes = in_off[i1] - in_off[i0], cap = sum - in_bytes;
        if ((s = stage_group(c, src, in_off, i0, i1, rel)) != KC_OK || (s = ensure(c, c->tmp_dst, (size_t)cap + 64)) != KC_OK) return s;
        oo.resize((size_t)(i1 - i0) + 1);
        KcDecTimes G;
        s = (kc_status)kc_sl_deflate(&dev, f, (const uint8_t*)c->tmp_src.p, rel.data(), i1 - i0, (uint8_t*)c->tmp_dst.p, cap, oo.data(), G);
        if (s == KC_ERR_DST_TOO_SMALL) { c->err = "a group's output exceeds kc_flate_stateless_bound"; return KC_ERR_INTERNAL; }
        if (s != KC_OK) return s;
        for (uint32_t k = 1; k <= i1 - i0; k++) out_off[i0 + k] = out_off[i0] + oo[k];
        if (out_off[i1] > dst_cap) return outcome(c, T, KC_ERR_DST_TOO_SMALL, TOO_SMALL);
        if (oo[i1 - i0]) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)oo[i1 - i0], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        T.prep_ms += G.prep_ms; T.match_ms += G.match_ms; T.other_ms += G.other_ms; T.emit_ms += G.emit_ms; T.batches += G.batches;
        i0 = i1;
    }
    return outcome(c, T, KC_OK, "");
}

}  // namespace

extern "C" {

kc_flate_swopts* kc_flate_swopts_default(void) {
    try { return new kc_flate_swopts(); } catch (...) { return nullptr; }
}
void kc_flate_swopts_free(kc_flate_swopts* o) { delete o; }
kc_status kc_flate_swopts_eof(kc_flate_swopts* o, int eof) {  // StatelessDeflate's eof, flate/stateless.go:76
    if (!o) return KC_ERR_BAD_ARG;
    o->o.eof = eof ? 1u : 0u;
    return KC_OK;
}
kc_status kc_flate_swopts_dict(kc_flate_swopts* o, const uint8_t* dict, uint64_t len) {  // truncated to its last 8192 bytes, :93-95
    if (!o || (len && !dict)) return KC_ERR_BAD_ARG;
    if (len > KCSL_MAX_DICT) { dict += len - KCSL_MAX_DICT; len = KCSL_MAX_DICT; }
    try { o->o.dict.assign(dict, dict + len); } catch (...) { return KC_ERR_INTERNAL; }
    return KC_OK;
}
uint64_t kc_flate_stateless_bound(uint64_t len, uint64_t dict_len) { return kc_sl_bound(len, dict_len); }

// flate.StatelessDeflate(out, input, eof, dict) per input: flate/stateless.go:76-162
kc_status kc_flate_stateless_deflate_dev(kc_ctx* c, const kc_flate_swopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                         uint64_t dst_cap, uint64_t* out_off) {
    return deflate_dev(c, o, 0, d_src, in_off, n, d_dst, dst_cap, out_off);
}
kc_status kc_flate_stateless_deflate(kc_ctx* c, const kc_flate_swopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                                     uint64_t dst_cap, uint64_t* out_off) {
    return deflate_host(c, o, 0, src, in_off, n, dst, dst_cap, out_off);
}
// gzip.NewWriterLevel(w, gzip.StatelessCompression); Write(input); Close() per input: gzip/gzip.go:171-235, :264-290
kc_status kc_gzip_stateless_deflate_dev(kc_ctx* c, const kc_flate_swopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                        uint64_t dst_cap, uint64_t* out_off) {
    return deflate_dev(c, o, 1, d_src, in_off, n, d_dst, dst_cap, out_off);
}
kc_status kc_gzip_stateless_deflate(kc_ctx* c, const kc_flate_swopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                                    uint64_t dst_cap, uint64_t* out_off) {
    return deflate_host(c, o, 1, src, in_off, n, dst, dst_cap, out_off);
}

}  // extern "C"
