#pragma once
// kc_decdev_host.h — what the decoders' host sequences need of a device.  The six decoders (kc_zdec_host.h, kc_s2dec_host.h,
// kc_s2ranges_host.h, kc_flate_host.h, kc_zdstream_host.h, kc_s2rstream_host.h) keep their host side in headers written against
// this interface alone: the library gives them HipDevice (kc_decdev_hip.h), the CPU suite gives them plain memory
// (tools/hipemu/kcemu.cpp), so the host code the suite runs is the host code that ships.
//
// Copies, zero-fills and launches are ordered; sync() waits for all of them.  The source of an h2d and the target of a d2h stay
// untouched until the next sync().  The kernels are launched by their kc_launch_* wrappers on `stream`.
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "kc_kernels.h"

struct KcDecDevice {
    hipStream_t stream = nullptr;                                 // (null on the emulator)
    virtual int reserve(int which, size_t bytes, void** p) = 0;  // at least `bytes`; a buffer that grows loses its contents
    virtual int h2d(void* d, const void* h, size_t n) = 0;
    virtual int d2h(void* h, const void* d, size_t n) = 0;
    virtual int d2d(void* d, const void* s, size_t n) = 0;
    virtual int zero(void* d, size_t n) = 0;
    virtual int sync() = 0;
    virtual uint64_t budget() { return UINT64_MAX; }             // scratch one batch may ask for (reserve() may add 1/8 to each buffer)
    virtual int mark(int k) { (void)k; return 0; }               // a point in the stream's time, k = 0 .. 3
    virtual float span(int a, int b) { (void)a; (void)b; return 0; }  // ms from mark a to mark b, both behind a sync(); 0 where time is not kept
    virtual void lane_group(int lanes) { (void)lanes; }          // the launches that follow diverge in groups of `lanes` (the emulator must be told)
    virtual ~KcDecDevice() {}
};

// What a batch decoder's sequence reports besides its results.
struct KcDecTimes {
    float prep_ms = 0, match_ms = 0, other_ms = 0;  // plan passes / decode / checksum and compaction
    float emit_ms = 0;                              // the stateless writers' emit kernel (kc_stateless_host.h), reported as kc_timings::entropy_ms
    int batches = 0;                                // device batches the call was cut into
    uint64_t max_need = 0;                          // the largest single input's scratch, 1/8 allowance included: the least budget that refuses nothing
};

template <class T>
static inline int kc_dec_reserve(KcDecDevice* dev, int which, size_t count, T** p) {
    return dev->reserve(which, count * sizeof(T), (void**)p);
}
template <class T>
static inline int kc_dec_fetch(KcDecDevice* dev, std::vector<T>& h, const T* d, size_t count) {
    h.resize(count);
    return dev->d2h(h.data(), d, count * sizeof(T));
}
static inline void kc_dec_need(KcDecTimes& T, uint64_t scratch) {
    const uint64_t need = scratch + (scratch >> 3);
    if (need > T.max_need) T.max_need = need;
}
