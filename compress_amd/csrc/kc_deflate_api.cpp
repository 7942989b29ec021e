// kc_deflate_api.cpp — flate.NewWriter / gzip.NewWriterLevel at flate.HuffmanOnly over a batch of independent inputs: the writer
// options and the entry points kc_flate_deflate[_dev] / kc_gzip_deflate[_dev] / kc_flate_deflate_bound of include/kcgpu.h.  The
// sequence of one device call is kc_deflate_host.h's; this file gives it the device (HipDevice over kc_ctx::df), checks the arguments
// and serves host buffers.
#include "kc_decdev_hip.h"
#include "kc_deflate_host.h"

struct kc_flate_wopts {
    KcDfOpts o;
};

namespace {

static_assert(DF_N == sizeof(kc_ctx::df) / sizeof(DevBuf), "kc_ctx::df has one slot per DF_* buffer");

kc_status check_deflate_args(kc_ctx* c, const kc_flate_wopts* o, const void* src, const uint64_t* in_off, uint32_t n, const void* dst, uint64_t dst_cap,
                             const uint64_t* out_off) {
    if (!out_off || !o) return KC_ERR_BAD_ARG;
    const kc_status s = check_batch_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    return n && !dst && dst_cap ? KC_ERR_BAD_ARG : KC_OK;
}

KcDfOpts opts_of(const kc_flate_wopts* o, uint32_t gzip) {
    KcDfOpts f = o->o;
    f.gzip = gzip;
    return f;
}

const char* const TOO_SMALL = "dst_cap below the exact size of the batch";

kc_status deflate_dev(kc_ctx* c, const kc_flate_wopts* o, uint32_t gzip, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                      uint64_t dst_cap, uint64_t* out_off) {
    kc_status s = check_deflate_args(c, o, d_src, in_off, n, d_dst, dst_cap, out_off);
    if (s != KC_OK) return s;
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->df);
    return take_outcome(c, T, kc_df_deflate(&dev, opts_of(o, gzip), d_src, in_off, n, d_dst, dst_cap, out_off, T), TOO_SMALL);
}

// Host buffers: groups of inputs, cut between inputs, whose bytes and bound together stay within half of the scratch budget (one
// input at least); each group is staged, written into the context's output staging by the device sequence, and copied out.
kc_status deflate_host(kc_ctx* c, const kc_flate_wopts* o, uint32_t gzip, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* out_off) {
    kc_status s = check_deflate_args(c, o, src, in_off, n, dst, dst_cap, out_off);
    if (s != KC_OK) return s;
    KcDecTimes T;
    (void)take_outcome(c, T, KC_OK, "");
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->df);
    const KcDfOpts f = opts_of(o, gzip);
    const uint64_t half = scratch_budget(c) / 2;
    auto cost = [&](uint32_t i) { const uint64_t len = in_off[i + 1] - in_off[i]; return len + kc_df_bound(len, f.block) + (gzip ? 18 : 0); };
    std::vector<uint64_t> rel, oo;
    for (uint32_t i0 = 0; i0 < n;) {
        uint64_t sum = cost(i0);
        uint32_t i1 = i0 + 1;
        while (i1 < n && sum + cost(i1) <= half) sum += cost(i1++);
        const uint64_t in_bytes = in_off[i1] - in_off[i0], cap = sum - in_bytes;
        if ((s = stage_group(c, src, in_off, i0, i1, rel)) != KC_OK || (s = ensure(c, c->tmp_dst, (size_t)cap + 64)) != KC_OK) return s;
        oo.resize((size_t)(i1 - i0) + 1);
        KcDecTimes G;
        s = (kc_status)kc_df_deflate(&dev, f, (const uint8_t*)c->tmp_src.p, rel.data(), i1 - i0, (uint8_t*)c->tmp_dst.p, cap, oo.data(), G);
        if (s == KC_ERR_DST_TOO_SMALL) { c->err = "a group's output exceeds kc_flate_deflate_bound"; return KC_ERR_INTERNAL; }
        if (s != KC_OK) return s;
        for (uint32_t k = 1; k <= i1 - i0; k++) out_off[i0 + k] = out_off[i0] + oo[k];
        if (out_off[i1] > dst_cap) return take_outcome(c, T, KC_ERR_DST_TOO_SMALL, TOO_SMALL);
        if (oo[i1 - i0]) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)oo[i1 - i0], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        T.prep_ms += G.prep_ms; T.match_ms += G.match_ms; T.other_ms += G.other_ms; T.batches += G.batches;
        i0 = i1;
    }
    return take_outcome(c, T, KC_OK, "");
}

}  // namespace

extern "C" {

kc_flate_wopts* kc_flate_wopts_default(void) {
    try { return new kc_flate_wopts(); } catch (...) { return nullptr; }
}
void kc_flate_wopts_free(kc_flate_wopts* o) { delete o; }
kc_status kc_flate_wopts_level(kc_flate_wopts* o, int level) {  // flate.NewWriter's level: compressor.init, flate/deflate.go:787-827
    if (!o) return KC_ERR_BAD_ARG;
    if (level != -2) return KC_ERR_UNSUPPORTED;
    o->o.level = level;
    return KC_OK;
}
kc_status kc_flate_wopts_end(kc_flate_wopts* o, int end) {  // close :865-880 or syncFlush :772-785
    if (!o || (end != KC_FL_END_CLOSE && end != KC_FL_END_FLUSH)) return KC_ERR_BAD_ARG;
    o->o.end = end == KC_FL_END_FLUSH ? KCDF_END_FLUSH : KCDF_END_CLOSE;
    return KC_OK;
}
kc_status kc_flate_wopts_block(kc_flate_wopts* o, uint32_t bytes, uint32_t penalty) {  // d.window and d.w.logNewTablePenalty, :795-799
    if (!o || bytes == 0 || bytes > 65535 || penalty > 31) return KC_ERR_BAD_ARG;
    o->o.block = bytes;
    o->o.penalty = penalty;
    return KC_OK;
}
uint64_t kc_flate_deflate_bound(uint64_t len, uint32_t block) { return kc_df_bound(len, block); }

// flate.NewWriter(w, flate.HuffmanOnly); Write(input); Close() per input: flate/deflate.go:755-770, 701-708, 865-880;
// flate/huffman_bit_writer.go:987-1174
kc_status kc_flate_deflate_dev(kc_ctx* c, const kc_flate_wopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                               uint64_t* out_off) {
    return deflate_dev(c, o, 0, d_src, in_off, n, d_dst, dst_cap, out_off);
}
kc_status kc_flate_deflate(kc_ctx* c, const kc_flate_wopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* out_off) {
    return deflate_host(c, o, 0, src, in_off, n, dst, dst_cap, out_off);
}
// gzip.NewWriterLevel(w, gzip.HuffmanOnly); Write(input); Close() per input: gzip/gzip.go:171-243, 264-290
kc_status kc_gzip_deflate_dev(kc_ctx* c, const kc_flate_wopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                              uint64_t* out_off) {
    return deflate_dev(c, o, 1, d_src, in_off, n, d_dst, dst_cap, out_off);
}
kc_status kc_gzip_deflate(kc_ctx* c, const kc_flate_wopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                          uint64_t* out_off) {
    return deflate_host(c, o, 1, src, in_off, n, dst, dst_cap, out_off);
}

}  // extern "C"
