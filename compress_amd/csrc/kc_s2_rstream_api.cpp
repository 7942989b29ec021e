// kc_s2_rstream_api.cpp — s2.NewReader(r).Read / Skip / ReadByte on the device: the entry points kc_s2_rstream_new / _feed / _skip /
// _skip_left / _on_skippable / _reset / _free of include/kcgpu.h.  The state machine is kc_s2rstream_host.h's; this file gives it the
// device: HipDevice (kc_decdev_hip.h) with buffers of the stream's own (one window of staged compressed bytes and its decoded bytes,
// the chunk records, the verdicts) on the context's stream.
#include "kc_decdev_hip.h"
#include "kc_s2rstream_host.h"

static_assert(RS_N <= HipDevice::OWN_N, "HipDevice holds every buffer of the stream");

struct kc_s2_rstream {
    HipDevice dev;
    KcS2rStream s;
    explicit kc_s2_rstream(kc_ctx* c) : dev(c) { s.dev = &dev; }
};

extern "C" {

kc_s2_rstream* kc_s2_rstream_new(kc_ctx* c, const kc_s2_ropts* o) {  // NewReader (s2/reader.go:31): a copy of the options
    if (!c || !o) return nullptr;
    try {
        kc_s2_rstream* z = new kc_s2_rstream(c);
        z->s.o.max_block = o->max_block;
        z->s.o.max_buf = max_buf_of(o->max_block);
        z->s.o.ignore_crc = o->ignore_crc;
        z->s.o.ignore_id = o->ignore_id;
        z->s.o.chunks = (uint32_t)c->cfg.s2_rstream_chunks;
        z->s.start();
        return z;
    } catch (...) {
        return nullptr;
    }
}

kc_status kc_s2_rstream_feed(kc_s2_rstream* z, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed,
                             uint64_t* produced, uint32_t* status) {  // Read, s2/reader.go:249-405
    if (!z || !consumed || !produced || !status || (n && !src) || (dst_cap && !dst)) return KC_ERR_BAD_ARG;
    kc_ctx* c = z->dev.c;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    HIPCHK(c, hipSetDevice(c->device));
    try {
        const int s = z->s.feed(src, n, eof, dst, dst_cap, consumed, produced, status);
        if (s == KC_ERR_DST_TOO_SMALL) c->err = "dst_cap is below the next chunk's decoded length";
        return (kc_status)s;
    } catch (const std::bad_alloc&) {
        c->err = "out of host memory";
        return KC_ERR_INTERNAL;
    }
}

kc_status kc_s2_rstream_skip(kc_s2_rstream* z, uint64_t n) {  // Skip, s2/reader.go:674-842: adds n to the pending skip
    if (!z || z->s.skip_left + n < n) return KC_ERR_BAD_ARG;
    z->s.skip_left += n;
    return KC_OK;
}

uint64_t kc_s2_rstream_skip_left(const kc_s2_rstream* z) { return z ? z->s.skip_left : 0; }

kc_status kc_s2_rstream_on_skippable(kc_s2_rstream* z, uint8_t id, kc_s2_skippable_fn fn, void* user) {  // ReaderSkippableCB, s2/reader.go:109
    if (!z) return KC_ERR_BAD_ARG;
    return (kc_status)z->s.on_skippable(id, fn, user);
}

kc_status kc_s2_rstream_reset(kc_s2_rstream* z) {  // Reset, s2/reader.go:177: the same buffers, options and callbacks; a new stream
    if (!z) return KC_ERR_BAD_ARG;
    z->s.reset();
    z->s.o.chunks = (uint32_t)z->dev.c->cfg.s2_rstream_chunks;  // (the context's option as it stands now, as at _new)
    return KC_OK;
}

void kc_s2_rstream_free(kc_s2_rstream* z) {
    if (!z) return;
    (void)hipSetDevice(z->dev.c->device);
    (void)hipStreamSynchronize(z->dev.c->stream);
    delete z;
}

}  // extern "C"
