#pragma once
// kc_zip_host.h — host side of zip.File.Open / io.ReadAll over a table of archive members, written against KcDecDevice alone
// (kc_zip_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator over plain memory).
//
// One call: the locate kernel reads every local header; from its results and the table the host makes the plan — which members get
// a range, and the prefix sum of the sizes the directory STATES is the layout — and the inflate, store and finish kernels decode
// every member once, straight to its place (kc_zip.hip).  There is no sizing pass: an archive that lies about its sizes costs the
// walk of the members that cannot stand, never memory.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"
#include "kc_zip_dev.h"

enum { ZP_MEM, ZP_BODY, ZP_BEND, ZP_LSTATUS, ZP_DSTATUS, ZP_KIND, ZP_OUT0, ZP_CHUNK0, ZP_CHUNK_MEM, ZP_VERDICT, ZP_CRC, ZP_CHUNK_CRC, ZP_STATUS, ZP_N };

#define KCZP_MAX_MEMBER ((uint64_t)1 << 30)  // bytes of one member, compressed or not, that this library serves

// The plan of member i from the table and the locate kernel's results: its kind, and for KCZP_NONE its verdict.  Rules 1 to 4 of
// include/kcgpu.h and the size rules that need no decoding.
static inline uint32_t kc_zp_plan_member(const kc_zip_member& m, uint32_t lstatus, uint64_t clipped, uint32_t* verdict) {
    *verdict = KCFL_OK;
    if (lstatus) { *verdict = lstatus; return KCZP_NONE; }                                        // reader.go:368-381
    if (m.is_dir) { if (m.uncompressed_size) *verdict = KCZP_FORMAT; return KCZP_NONE; }         // :252-267
    if (m.method != 0 && m.method != 8) { *verdict = KCZP_ALGORITHM; return KCZP_NONE; }         // :270-273
    if (m.compressed_size > KCZP_MAX_MEMBER || m.uncompressed_size > KCZP_MAX_MEMBER) { *verdict = KCZP_SIZE; return KCZP_NONE; }
    if (m.method == 0) {  // Store: the decompressor yields the clipped body (:331-340)
        if (clipped > m.uncompressed_size) { *verdict = KCZP_FORMAT; return KCZP_NONE; }
        if (clipped < m.uncompressed_size) { *verdict = KCFL_EOF; return KCZP_NONE; }
        return KCZP_STORE;
    }
    // a length of 258 bytes takes at least two bits: DEFLATE yields at most 1032 bytes per input byte
    return m.uncompressed_size > 1032 * clipped + 1032 ? KCZP_WALK : KCZP_INFLATE;
}

// bound: the layout and the verdicts that need no decoding alone (d_dst and dst_cap are not read).  Returns KC_OK,
// KC_ERR_DST_TOO_SMALL (out_off holds the planned layout, nothing is written), KC_ERR_UNSUPPORTED (more than 2^32 - 1 chunks) or
// the device's error.
static inline int kc_zp_read(KcDecDevice* dev, const uint8_t* d_src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* d_dst,
                             uint64_t dst_cap, uint64_t* out_off, uint32_t* status, bool bound, KcDecTimes& T) {
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    KcZipParams P;
    memset(&P, 0, sizeof(P));
    kc_zip_member* d_mem = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, ZP_MEM, n, &d_mem)) || (s = kc_dec_reserve(dev, ZP_BODY, n, &P.body)) || (s = kc_dec_reserve(dev, ZP_BEND, n, &P.body_end)) ||
        (s = kc_dec_reserve(dev, ZP_LSTATUS, n, &P.lstatus)) || (s = kc_dec_reserve(dev, ZP_DSTATUS, n, &P.dstatus)) ||
        (s = dev->h2d(d_mem, members, (size_t)n * sizeof(kc_zip_member))))
        return s;
    P.src = d_src; P.src_len = src_len; P.mem = d_mem; P.n = n;
    std::vector<uint64_t> body(n), bend(n), out0(n);
    std::vector<uint32_t> lst(n), kind(n), chunk0((size_t)n + 1, 0), chunk_mem;
    if ((s = dev->mark(0))) return s;
    kc_launch_zip_locate(P, dev->stream);
    if ((s = dev->mark(1)) || (s = dev->d2h(body.data(), P.body, (size_t)n * 8)) || (s = dev->d2h(bend.data(), P.body_end, (size_t)n * 8)) ||
        (s = dev->d2h(lst.data(), P.lstatus, (size_t)n * 4)) || (s = dev->sync()))
        return s;
    T.prep_ms += dev->span(0, 1);
    uint64_t chunks = 0;
    for (uint32_t i = 0; i < n; i++) {
        kind[i] = kc_zp_plan_member(members[i], lst[i], bend[i] - body[i], &status[i]);
        const bool range = kind[i] == KCZP_INFLATE || kind[i] == KCZP_STORE;
        out0[i] = out_off[i];
        out_off[i + 1] = out_off[i] + (range ? members[i].uncompressed_size : 0);
        if (kind[i] == KCZP_STORE) chunks += (members[i].uncompressed_size + KCZP_CHUNK - 1) / KCZP_CHUNK;
        chunk0[i + 1] = (uint32_t)chunks;
    }
    if (bound) return KC_OK;
    if (out_off[n] > dst_cap) return KC_ERR_DST_TOO_SMALL;
    if (chunks > 0xFFFFFFFFull) return KC_ERR_UNSUPPORTED;
    chunk_mem.resize((size_t)chunks + 1);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t c = chunk0[i]; c < chunk0[i + 1]; c++) chunk_mem[c] = i;
    uint32_t *d_kind = nullptr, *d_chunk0 = nullptr, *d_chunk_mem = nullptr;
    uint64_t* d_out0 = nullptr;
    if ((s = kc_dec_reserve(dev, ZP_KIND, n, &d_kind)) || (s = kc_dec_reserve(dev, ZP_OUT0, n, &d_out0)) ||
        (s = kc_dec_reserve(dev, ZP_CHUNK0, (size_t)n + 1, &d_chunk0)) || (s = kc_dec_reserve(dev, ZP_CHUNK_MEM, (size_t)chunks + 1, &d_chunk_mem)) ||
        (s = kc_dec_reserve(dev, ZP_VERDICT, n, &P.verdict)) || (s = kc_dec_reserve(dev, ZP_CRC, n, &P.crc)) ||
        (s = kc_dec_reserve(dev, ZP_CHUNK_CRC, (size_t)chunks + 1, &P.chunk_crc)) || (s = kc_dec_reserve(dev, ZP_STATUS, n, &P.status)) ||
        (s = dev->h2d(d_kind, kind.data(), (size_t)n * 4)) || (s = dev->h2d(d_out0, out0.data(), (size_t)n * 8)) ||
        (s = dev->h2d(d_chunk0, chunk0.data(), ((size_t)n + 1) * 4)) || (s = dev->h2d(d_chunk_mem, chunk_mem.data(), (size_t)chunks * 4)))
        return s;
    P.kind = d_kind; P.out0 = d_out0; P.chunk0 = d_chunk0; P.chunk_mem = d_chunk_mem; P.n_chunks = (uint32_t)chunks; P.dst = d_dst;
    std::vector<uint32_t> fin(n);
    if ((s = dev->mark(1))) return s;
    bool any_inflate = false, any_walk = false;
    for (uint32_t i = 0; i < n; i++) { any_inflate |= kind[i] == KCZP_INFLATE; any_walk |= kind[i] == KCZP_WALK; }
    if (any_inflate) kc_launch_zip_inflate(P, true, dev->stream);
    if (any_walk) kc_launch_zip_inflate(P, false, dev->stream);
    kc_launch_zip_store(P, dev->stream);
    if ((s = dev->mark(2))) return s;
    kc_launch_zip_finish(P, dev->stream);
    if ((s = dev->mark(3)) || (s = dev->d2h(fin.data(), P.status, (size_t)n * 4)) || (s = dev->sync())) return s;
    T.match_ms += dev->span(1, 2);
    T.other_ms += dev->span(2, 3);
    for (uint32_t i = 0; i < n; i++)
        if (kind[i] != KCZP_NONE) status[i] = fin[i];
    T.batches = 1;
    return KC_OK;
}
