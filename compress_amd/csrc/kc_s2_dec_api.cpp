// kc_s2_dec_api.cpp — s2.Reader and s2.Decode over a batch of independent inputs: the reader options and the entry points
// kc_s2_decode_streams[_bound][_dev] / kc_s2_decode_blocks_all[_bound][_dev] of include/kcgpu.h.  The sequence of one device call
// is kc_s2dec_host.h's; this file gives it the device (HipDevice over kc_ctx::s2d), checks the arguments and serves host buffers.
#include "kc_decdev_hip.h"
#include "kc_s2_plan_dev.h"

namespace {

static_assert(SD_N == sizeof(kc_ctx::s2d) / sizeof(DevBuf), "kc_ctx::s2d has one slot per SD_* buffer");

typedef KcS2dMode Mode;
Mode mode_blocks() {
    Mode m;
    m.max_buf = max_buf_of(m.max_block);
    m.blocks = 1;
    return m;
}

// the walk of one input on the host: the same function the plan kernel runs
KcS2Walk walk_host(const Mode& m, const uint8_t* src, uint64_t pos, uint64_t end) {
    auto none = [](uint32_t, uint64_t, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t) {};
    if (!m.blocks) return kc_s2_walk(src, pos, end, m.max_block, m.max_buf, m.ignore_id != 0, none);
    KcS2Walk W;
    W.status = KCS2D_OK; W.n_chunks = 0; W.total = 0;
    uint32_t dl = 0, hdr = 0;
    if (end - pos > 0xffffffffull) W.status = KCS2D_SIZE;
    else if (!kc_s2_decoded_len(src, pos, end, &dl, &hdr)) W.status = KCS2D_CORRUPT;
    else { W.n_chunks = 1; W.total = dl; }
    return W;
}

kc_status decode_dev(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                     uint64_t* out_off, uint32_t* status) {
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->s2d);
    return take_outcome(c, T, kc_s2d_decode(&dev, m, d_src, in_off, n, d_dst, dst_cap, out_off, status, T), "dst_cap too small for the planned layout");
}

kc_status bound_dev(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_batch_args(c, d_src, in_off, n);
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->s2d);
    KcDecTimes T;
    KcS2dPlan H;
    if ((s = take_outcome(c, T, kc_s2d_plan_inputs(&dev, m, d_src, in_off, n, H, T), "", false)) != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) { bound[i] = H.bound[i]; status[i] = H.status[i]; }
    return KC_OK;
}

kc_status bound_host(kc_ctx* c, const Mode& m, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_batch_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) {  // the headers are in host memory: the walk runs where they are
        const KcS2Walk W = walk_host(m, src, in_off[i], in_off[i + 1]);
        bound[i] = W.total;
        status[i] = W.status;
    }
    return KC_OK;
}

// Host buffers: the walk runs on the host first (the layout, and DST_TOO_SMALL before anything is written); the inputs then go to
// the device in groups, cut between inputs, whose bytes and decoded bytes together fit a quarter of the scratch budget.  An input
// that does not fit alone gets KC_S2D_SIZE_EXCEEDED: it keeps its planned range, zero-filled like any other failed input's.
kc_status decode_host(kc_ctx* c, const Mode& m, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                      uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_batch_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !dst && dst_cap) return KC_ERR_BAD_ARG;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    std::vector<uint64_t> bound(n);
    for (uint32_t i = 0; i < n; i++) {
        bound[i] = walk_host(m, src, in_off[i], in_off[i + 1]).total;
        out_off[i + 1] = out_off[i] + bound[i];
    }
    if (out_off[n] > dst_cap) { c->err = "dst_cap too small for the planned layout"; return KC_ERR_DST_TOO_SMALL; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GroupSum sum;
    std::vector<uint64_t> rel, oo;
    std::vector<uint32_t> stt;
    uint32_t i0 = 0;
    while (i0 < n) {
        const uint64_t quarter = scratch_budget(c) / 4;
        auto cost = [&](uint32_t a, uint32_t b) { return (in_off[b] - in_off[a]) + (out_off[b] - out_off[a]); };
        if (cost(i0, i0 + 1) > quarter) {
            status[i0] = KC_S2D_SIZE_EXCEEDED;
            if (bound[i0]) memset(dst + out_off[i0], 0, (size_t)bound[i0]);
            i0++;
            continue;
        }
        uint32_t i1 = i0 + 1;
        while (i1 < n && cost(i0, i1 + 1) <= quarter) i1++;
        const uint32_t nb = i1 - i0;
        const uint64_t need = out_off[i1] - out_off[i0];
        if ((s = ensure(c, c->tmp_dst, (size_t)need + 64)) || (s = stage_group(c, src, in_off, i0, i1, rel))) return s;
        oo.resize(nb + 1); stt.resize(nb);
        if ((s = decode_dev(c, m, (const uint8_t*)c->tmp_src.p, rel.data(), nb, (uint8_t*)c->tmp_dst.p, need, oo.data(), stt.data())) != KC_OK) return s;
        if (oo[nb] != need) { c->err = "internal: the device plan and the host plan disagree"; return KC_ERR_INTERNAL; }
        if (need) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (uint32_t k = 0; k < nb; k++) status[i0 + k] = stt[k];
        sum.add(c);
        i0 = i1;
    }
    sum.give(c);
    return KC_OK;
}

kc_status decode_dev_checked(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                             uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_batch_args(c, d_src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !d_dst && dst_cap) return KC_ERR_BAD_ARG;
    return decode_dev(c, m, d_src, in_off, n, d_dst, dst_cap, out_off, status);
}

}  // namespace

extern "C" {

kc_s2_ropts* kc_s2_ropts_default(void) {
    try { return new kc_s2_ropts(); } catch (...) { return nullptr; }
}
void kc_s2_ropts_free(kc_s2_ropts* o) { delete o; }
int kc_s2_ropts_max_block_size(kc_s2_ropts* o, int64_t n) {  // ReaderMaxBlockSize, s2/reader.go:64-75
    if (!o || n <= 0 || n > (int64_t)KC_S2_MAX_FRAMED_BLOCK) return -1;
    o->max_block = (uint32_t)n;
    return 0;
}
int kc_s2_ropts_ignore_crc(kc_s2_ropts* o, int b) {  // ReaderIgnoreCRC, s2/reader.go:120-125
    if (!o) return -1;
    o->ignore_crc = b != 0;
    return 0;
}
int kc_s2_ropts_ignore_stream_identifier(kc_s2_ropts* o, int b) {  // ReaderIgnoreStreamIdentifier, s2/reader.go:95-100
    if (!o) return -1;
    o->ignore_id = b != 0;
    return 0;
}

// io.ReadAll(s2.NewReader(input)) per input: s2/reader.go:249-405
kc_status kc_s2_decode_streams_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                   uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return decode_dev_checked(c, mode_of(o), d_src, in_off, n, d_dst, dst_cap, out_off, status);
}
kc_status kc_s2_decode_streams(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                               uint64_t* out_off, uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return decode_host(c, mode_of(o), src, in_off, n, dst, dst_cap, out_off, status);
}
// the chunk headers of s2/reader.go:259-404 alone
kc_status kc_s2_decode_streams_bound_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                         uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return bound_dev(c, mode_of(o), d_src, in_off, n, bound, status);
}
kc_status kc_s2_decode_streams_bound(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                     uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return bound_host(c, mode_of(o), src, in_off, n, bound, status);
}
// N x s2.Decode(nil, block): s2/decode.go:58-76 -> s2Decode, s2/decode_other.go:22-290
kc_status kc_s2_decode_blocks_all_dev(kc_ctx* c, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                                      uint64_t* out_off, uint32_t* status) {
    return decode_dev_checked(c, mode_blocks(), d_src, in_off, n, d_dst, dst_cap, out_off, status);
}
kc_status kc_s2_decode_blocks_all(kc_ctx* c, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                                  uint32_t* status) {
    return decode_host(c, mode_blocks(), src, in_off, n, dst, dst_cap, out_off, status);
}
// N x s2.DecodedLen(block): s2/decode.go:29-47
kc_status kc_s2_decode_blocks_all_bound_dev(kc_ctx* c, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    return bound_dev(c, mode_blocks(), d_src, in_off, n, bound, status);
}
kc_status kc_s2_decode_blocks_all_bound(kc_ctx* c, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    return bound_host(c, mode_blocks(), src, in_off, n, bound, status);
}

}  // extern "C"
