// kc_zstd_dstream_api.cpp — zstd.NewReader(r) / Decoder.Read / WriteTo on the device: the entry points kc_zstd_dstream_new / _feed /
// _reset / _free of include/kcgpu.h.  The state machine is kc_zdstream_host.h's; this file gives it the device: HipDevice
// (kc_decdev_hip.h) with buffers of the stream's own on the context's stream.
#include "kc_decdev_hip.h"
#include "kc_zdstream_host.h"

static_assert(ZS_N <= HipDevice::OWN_N, "HipDevice holds every buffer of the stream");

struct kc_zstd_dstream {
    HipDevice dev;
    KcZsStream s;
    explicit kc_zstd_dstream(kc_ctx* c) : dev(c) { s.dev = &dev; }
};

extern "C" {

kc_zstd_dstream* kc_zstd_dstream_new(kc_ctx* c, const kc_zstd_dopts* o) {  // NewReader / Reset: a fresh stream
    if (!c || !o) return nullptr;
    try {
        kc_zstd_dstream* z = new kc_zstd_dstream(c);
        static_cast<KcZdOpts&>(z->s.o) = *o;
        z->s.o.blocks = (uint32_t)c->cfg.dstream_blocks;
        return z;
    } catch (...) {
        return nullptr;
    }
}

kc_status kc_zstd_dstream_feed(kc_zstd_dstream* z, const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed,
                               uint64_t* produced, uint32_t* status) {
    if (!z || !consumed || !produced || !status || (n && !src) || (dst_cap && !dst)) return KC_ERR_BAD_ARG;
    kc_ctx* c = z->dev.c;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    HIPCHK(c, hipSetDevice(c->device));
    try {
        const int s = z->s.feed(src, n, eof, dst, dst_cap, consumed, produced, status);
        if (s == KC_ERR_DST_TOO_SMALL) c->err = "dst_cap is below one block's bound";
        return (kc_status)s;
    } catch (const std::bad_alloc&) {
        c->err = "out of host memory";
        return KC_ERR_INTERNAL;
    }
}

kc_status kc_zstd_dstream_reset(kc_zstd_dstream* z) {  // Decoder.Reset: the same buffers, a new stream
    if (!z) return KC_ERR_BAD_ARG;
    z->s.reset();
    return KC_OK;
}

void kc_zstd_dstream_free(kc_zstd_dstream* z) {
    if (!z) return;
    (void)hipSetDevice(z->dev.c->device);
    (void)hipStreamSynchronize(z->dev.c->stream);
    delete z;
}

}  // extern "C"
