// kc_zstd_dstream_api.cpp — zstd.NewReader(r) / Decoder.Read / WriteTo on the device: the entry points kc_zstd_dstream_new / _feed /
// _reset / _free of include/kcgpu.h.  The state machine is kc_zdstream_host.h's; this file gives it the device: buffers of the
// stream's own, copies and the three kernels of kc_zstd_dstream.hip on the context's stream.
#include "kc_host.h"
#include "kc_zdstream_host.h"

namespace {

struct HipDevice : KcZsDevice {
    kc_ctx* c = nullptr;
    DevBuf buf[B_N];
    int reserve(int which, size_t bytes, void** p) override {
        const kc_status s = ensure(c, buf[which], bytes ? bytes : 1);
        *p = buf[which].p;
        return s;
    }
    int h2d(void* d, const void* h, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
        return KC_OK;
    }
    int d2h(void* h, const void* d, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream));
        return KC_OK;
    }
    int d2d(void* d, const void* s, size_t n) override {
        if (n) HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, c->stream));
        return KC_OK;
    }
    void entropy(const KcZsEntropyParams& P) override { kc_launch_zstd_dstream_entropy(P, c->stream); }
    void execute(const KcZsExecParams& P) override { kc_launch_zstd_dstream_execute(P, c->stream); }
    void hash(const KcZsHashParams& P) override { kc_launch_xxh64_stream(P, c->stream); }
    int sync() override {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        return KC_OK;
    }
    ~HipDevice() override {
        for (DevBuf& b : buf) if (b.p) (void)hipFree(b.p);
    }
};

}  // namespace

struct kc_zstd_dstream {
    HipDevice dev;
    KcZsStream s;
};

extern "C" {

kc_zstd_dstream* kc_zstd_dstream_new(kc_ctx* c, const kc_zstd_dopts* o) {  // NewReader / Reset: a fresh stream
    if (!c || !o) return nullptr;
    try {
        kc_zstd_dstream* z = new kc_zstd_dstream();
        z->dev.c = c;
        z->s.dev = &z->dev;
        z->s.o.max_memory = o->max_memory;
        z->s.o.max_window = o->max_window;
        z->s.o.ignore_checksum = o->ignore_checksum;
        z->s.o.blocks = (uint32_t)c->cfg.dstream_blocks;
        z->s.o.dicts = o->dicts;
        z->s.o.arena = o->arena;
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
