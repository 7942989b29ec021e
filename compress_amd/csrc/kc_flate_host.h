#pragma once
// kc_flate_host.h — host side of flate.NewReader / flate.NewReaderDict / gzip.NewReader / zlib.NewReaderDict over a batch of independent inputs, written
// against KcDecDevice alone (kc_flate_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator over plain memory).
//
// One call: the sizing pass (kc_flate_inflate.hip) walks every input and yields its decoded size, its verdict short of the checksum
// and the bytes it read; the prefix sum of the sizes IS the output layout; the write pass decodes every input straight to its
// place, checks the gzip CRCs / the zlib Adler-32 and zero-fills what failed.  Nothing is staged and nothing is compacted, and no scratch grows with
// the inputs' bytes: the device form is one batch whatever the budget.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"
#include "kc_flate_dev.h"

enum { FL_IN_OFF, FL_SIZE, FL_STATUS, FL_CONSUMED, FL_MEMBERS, FL_OUT0, FL_WSTATUS, FL_DICT, FL_N };

struct KcFlOpts {
    uint32_t format = KCFL_FMT_FLATE;  // KCFL_FMT_*: raw DEFLATE, gzip or zlib
    int multistream = 1;            // gzip.Reader.Multistream
    const uint8_t* dict = nullptr;  // flate.NewReaderDict / zlib.NewReaderDict: its last dict_len <= 32 KiB (not read for gzip)
    uint32_t dict_len = 0;
    uint32_t dict_id = 1;           // zlib: adler32 of the WHOLE dictionary (adler32(nil) = 1), zlib/reader.go:164-165
};

// adler32.Checksum (RFC 1950, section 8.2), plain: the dictionary's id is computed once, on the host
static inline uint32_t kc_fl_adler32(const uint8_t* p, uint64_t n) {
    uint32_t s1 = 1, s2 = 0;
    while (n) {  // 5552 bytes of 0xFF are the most that 32-bit sums hold between two reductions
        const uint64_t k = n < 5552 ? n : 5552;
        for (uint64_t i = 0; i < k; i++) { s1 += p[i]; s2 += s1; }
        s1 %= 65521u; s2 %= 65521u;
        p += k; n -= k;
    }
    return s2 << 16 | s1;
}

// the sizing pass's results on the host, and the parameters both passes share (the arrays of the inputs last prepared)
struct KcFlPlan {
    KcFlateParams P;
    uint64_t* d_out0 = nullptr;
    std::vector<uint64_t> size, consumed;
    std::vector<uint32_t> status, members;
    void resize(uint32_t n) { size.assign(n, 0); consumed.assign(n, 0); status.assign(n, 0); members.assign(n, 0); }
};

// the device arrays of n inputs and the parameters both passes share
static inline int kc_fl_prepare(KcDecDevice* dev, const KcFlOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcFlPlan& H) {
    KcFlateParams& P = H.P;
    memset(&P, 0, sizeof(P));
    uint64_t* d_in_off = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, FL_IN_OFF, (size_t)n + 1, &d_in_off)) || (s = kc_dec_reserve(dev, FL_SIZE, n, &P.size)) ||
        (s = kc_dec_reserve(dev, FL_STATUS, n, &P.status)) || (s = kc_dec_reserve(dev, FL_CONSUMED, n, &P.consumed)) ||
        (s = kc_dec_reserve(dev, FL_MEMBERS, n, &P.members)) || (s = kc_dec_reserve(dev, FL_OUT0, n, &H.d_out0)) ||
        (s = kc_dec_reserve(dev, FL_WSTATUS, n, &P.wstatus)) || (s = dev->h2d(d_in_off, in_off, ((size_t)n + 1) * 8)))
        return s;
    P.src = d_src;
    P.in_off = d_in_off;
    P.n = n;
    P.gzip = o.format;
    P.multistream = o.multistream != 0;
    P.dict_id = o.dict_id;
    if (o.format != KCFL_FMT_GZIP && o.dict_len) {
        uint8_t* d_dict = nullptr;
        if ((s = kc_dec_reserve(dev, FL_DICT, o.dict_len, &d_dict)) || (s = dev->h2d(d_dict, o.dict, o.dict_len))) return s;
        P.dict = d_dict;
        P.dict_len = o.dict_len;
    }
    P.out0 = H.d_out0;
    return KC_OK;
}

// the sizing pass over the inputs last prepared; its results on the host (at H[at ...])
static inline int kc_fl_size_inputs(KcDecDevice* dev, KcFlPlan& H, uint32_t at, KcDecTimes& T) {
    const KcFlateParams& P = H.P;
    const uint32_t n = P.n;
    int s;
    if ((s = dev->mark(0))) return s;
    if (P.gzip == KCFL_FMT_ZLIB) kc_launch_zlib_size(P, dev->stream);
    else kc_launch_flate_size(P, dev->stream);
    if ((s = dev->mark(1)) || (s = dev->d2h(H.size.data() + at, P.size, (size_t)n * 8)) || (s = dev->d2h(H.status.data() + at, P.status, (size_t)n * 4)) ||
        (s = dev->d2h(H.consumed.data() + at, P.consumed, (size_t)n * 8)) || (s = dev->d2h(H.members.data() + at, P.members, (size_t)n * 4)) ||
        (s = dev->sync()))
        return s;
    T.prep_ms += dev->span(0, 1);
    return KC_OK;
}

// the write pass over the inputs last prepared, planned as H[at ...] says, input i at d_dst + out0[i]; the verdicts settle status /
// consumed: the write pass's for an input with members to write, else the sizing pass's
static inline int kc_fl_write_inputs(KcDecDevice* dev, const KcFlPlan& H, uint32_t at, const uint64_t* out0, uint8_t* d_dst, uint32_t* status,
                                     uint64_t* consumed, bool plan_on_device, KcDecTimes& T) {
    KcFlateParams P = H.P;
    const uint32_t n = P.n;
    int s;
    if (!plan_on_device &&  // the host forms re-group between the sweeps: the plan of THESE inputs goes up again
        ((s = dev->h2d(P.size, H.size.data() + at, (size_t)n * 8)) || (s = dev->h2d(P.status, H.status.data() + at, (size_t)n * 4)) ||
         (s = dev->h2d(P.members, H.members.data() + at, (size_t)n * 4))))
        return s;
    P.dst = d_dst;
    std::vector<uint32_t> wst(n);
    if ((s = dev->h2d(H.d_out0, out0, (size_t)n * 8)) || (s = dev->mark(1))) return s;
    if (P.gzip == KCFL_FMT_ZLIB) kc_launch_zlib_write(P, dev->stream);
    else kc_launch_flate_write(P, dev->stream);
    if ((s = dev->mark(2)) || (s = dev->d2h(wst.data(), P.wstatus, (size_t)n * 4)) || (s = dev->sync())) return s;
    T.match_ms += dev->span(1, 2);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = H.members[at + i] ? wst[i] : H.status[at + i];
        status[i] = v;
        if (consumed) consumed[i] = v ? 0 : H.consumed[at + i];
    }
    return KC_OK;
}

// bound != null: the sizing pass alone (d_dst, dst_cap and out_off are not read).  Returns KC_OK, KC_ERR_DST_TOO_SMALL (out_off
// holds the planned layout, nothing is written) or the device's error.
static inline int kc_fl_inflate(KcDecDevice* dev, const KcFlOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound, KcDecTimes& T) {
    if (!bound) out_off[0] = 0;
    if (n == 0) return KC_OK;
    KcFlPlan H;
    H.resize(n);
    int s;
    if ((s = kc_fl_prepare(dev, o, d_src, in_off, n, H)) || (s = kc_fl_size_inputs(dev, H, 0, T))) return s;
    if (bound) {
        for (uint32_t i = 0; i < n; i++) { bound[i] = H.size[i]; status[i] = H.status[i]; if (consumed) consumed[i] = H.consumed[i]; }
        return KC_OK;
    }
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.size[i];  // the planned layout
    if (out_off[n] > dst_cap) return KC_ERR_DST_TOO_SMALL;
    if ((s = kc_fl_write_inputs(dev, H, 0, out_off, d_dst, status, consumed, true, T))) return s;
    T.batches = 1;
    return KC_OK;
}
