#pragma once
// kc_decdev_hip.h — the decoders' device (kc_decdev_host.h) over HIP on a context's stream, and what the batch decoders' entry
// points (kc_zstd_dec_api.cpp, kc_s2_dec_api.cpp, kc_s2_ranges_api.cpp, kc_flate_api.cpp) share besides it.
#include "kc_host.h"
#include "kc_decdev_host.h"
#include "kc_s2dec_host.h"

namespace kci {

// Buffers: a batch decoder's are the context's (`ctx_bufs`: kc_ctx::zd / s2d / s2r / fl, kept from call to call and freed with the
// context's scratch); a stream reader's are the device's own, freed with it.  HIP failures leave their text in the context.
struct HipDevice : KcDecDevice {
    enum { OWN_N = 12 };
    kc_ctx* c;
    DevBuf own[OWN_N];
    DevBuf* buf;
    explicit HipDevice(kc_ctx* ctx, DevBuf* ctx_bufs = nullptr) : c(ctx), buf(ctx_bufs ? ctx_bufs : own) { stream = ctx->stream; }
    int reserve(int which, size_t bytes, void** p) override {
        const kc_status s = ensure(c, buf[which], bytes ? bytes : 1);
        *p = buf[which].p;
        return s;
    }
    int h2d(void* d, const void* h, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream));
        return KC_OK;
    }
    int d2h(void* h, const void* d, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, stream));
        return KC_OK;
    }
    int d2d(void* d, const void* s, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream));
        return KC_OK;
    }
    int zero(void* d, size_t n) override {
        if (n) HIPCHK(c, hipMemsetAsync(d, 0, n, stream));
        return KC_OK;
    }
    int sync() override {
        HIPCHK(c, hipStreamSynchronize(stream));
        HIPCHK(c, hipGetLastError());
        return KC_OK;
    }
    uint64_t budget() override { return scratch_budget(c); }
    int mark(int k) override {
        HIPCHK(c, hipEventRecord(c->ev[k], stream));
        return KC_OK;
    }
    float span(int a, int b) override {
        float t = 0;
        (void)hipEventElapsedTime(&t, c->ev[a], c->ev[b]);
        return t;
    }
    ~HipDevice() override {
        for (DevBuf& b : own) if (b.p) (void)hipFree(b.p);
    }
};

// what every batch entry point checks first: the context is free, the offsets ascend.  Clears the context's error text.
inline kc_status check_batch_args(kc_ctx* c, const void* src, const uint64_t* in_off, uint32_t n) {
    if (!c || !in_off || (n && !src)) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    for (uint32_t i = 0; i < n; i++)
        if (in_off[i + 1] < in_off[i]) { c->err = "in_off not ascending"; return KC_ERR_BAD_ARG; }
    return KC_OK;
}

// a sequence's outcome into the context: its timings, its batch count (where the call has one), the text of DST_TOO_SMALL
inline kc_status take_outcome(kc_ctx* c, const KcDecTimes& T, int s, const char* too_small, bool batches = true) {
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last.prep_ms = T.prep_ms; c->last.match_ms = T.match_ms; c->last.other_ms = T.other_ms;
    if (batches) c->last_batches = T.batches;
    if (s == KC_OK) c->last.total_ms = T.prep_ms + T.match_ms + T.other_ms;
    if (s == KC_ERR_DST_TOO_SMALL) c->err = too_small;
    return (kc_status)s;
}

// the reader's options as the S2 sequences take them (whole inputs and ranged reads)
inline KcS2dMode mode_of(const kc_s2_ropts* o) {
    KcS2dMode m;
    m.max_block = o->max_block; m.max_buf = max_buf_of(o->max_block); m.ignore_crc = o->ignore_crc; m.ignore_id = o->ignore_id;
    return m;
}

// host-buffer forms: the inputs i0 .. i1 into c->tmp_src (upload = false: they are there already), their offsets relative to the group
inline kc_status stage_group(kc_ctx* c, const uint8_t* src, const uint64_t* in_off, uint32_t i0, uint32_t i1, std::vector<uint64_t>& rel,
                             bool upload = true) {
    const uint64_t bytes = in_off[i1] - in_off[i0];
    kc_status s;
    if ((s = ensure(c, c->tmp_src, (size_t)bytes + 64)) != KC_OK) return s;
    if (bytes && upload) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src + in_off[i0], (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    rel.resize(i1 - i0 + 1);
    for (uint32_t k = 0; k <= i1 - i0; k++) rel[k] = in_off[i0 + k] - in_off[i0];
    return KC_OK;
}

// host-buffer forms: one group's timings and batches onto the call's
struct GroupSum {
    kc_timings t = {0, 0, 0, 0, 0, 0};
    int batches = 0;
    void add(const kc_ctx* c) {
        t.prep_ms += c->last.prep_ms; t.match_ms += c->last.match_ms; t.other_ms += c->last.other_ms; t.total_ms += c->last.total_ms;
        batches += c->last_batches;
    }
    void give(kc_ctx* c) const { c->last = t; c->last_batches = batches; }
};

}  // namespace kci
