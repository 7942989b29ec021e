#pragma once
// kc_s2dec_host.h — host side of s2.Reader / s2.Decode over a batch of independent inputs, written against KcDecDevice alone
// (kc_s2_dec_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator over plain memory).
//
// One call: the plan kernel's first pass sizes every input (kc_s2_plan.hip: data chunks, decoded bytes, first header-level error);
// the prefix sum of those sizes IS the output layout, because an S2 chunk's decoded length stands in its header; the second pass
// writes the chunk records with their final places in dst and the decode kernel decodes one chunk per wave straight to its place
// and checks its CRC (kc_s2_decode_all.hip).  The host then settles every input — the first failing chunk in stream order, else
// the plan's error — and zero-fills the range of every input that failed.  Nothing is staged and nothing is compacted.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"

enum { SD_IN_OFF, SD_NC, SD_BOUND, SD_STATUS, SD_CHUNK0, SD_OUT0, SD_CHUNKS, SD_CSTATUS, SD_N };

struct KcS2dMode {  // what one call decodes: framed streams under the reader's options, or bare blocks
    uint32_t max_block = 4u << 20;  // Reader.maxBlock (maxBlockSize)
    uint32_t max_buf = 0;           // MaxEncodedLen(max_block) + 4 (Reader.maxBufSize, s2/reader.go:42)
    int ignore_crc = 0, ignore_id = 0, blocks = 0;
};

// the plan's first pass: its parameters (the arrays on the device) and its results on the host
struct KcS2dPlan {
    KcS2PlanParams P;
    std::vector<uint32_t> nc, status;
    std::vector<uint64_t> bound;
    uint32_t* d_chunk0 = nullptr;
    uint64_t* d_out0 = nullptr;
};

// the plan's first pass over all inputs.  The inputs' offsets stay on the device.
static inline int kc_s2d_plan_inputs(KcDecDevice* dev, const KcS2dMode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcS2dPlan& H,
                                     KcDecTimes& T) {
    KcS2PlanParams& P = H.P;
    memset(&P, 0, sizeof(P));
    uint64_t* d_in_off = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, SD_IN_OFF, (size_t)n + 1, &d_in_off)) || (s = kc_dec_reserve(dev, SD_NC, n, &P.n_chunks)) ||
        (s = kc_dec_reserve(dev, SD_BOUND, n, &P.bound)) || (s = kc_dec_reserve(dev, SD_STATUS, n, &P.status)) ||
        (s = kc_dec_reserve(dev, SD_CHUNK0, n, &H.d_chunk0)) || (s = kc_dec_reserve(dev, SD_OUT0, n, &H.d_out0)) ||
        (s = dev->h2d(d_in_off, in_off, ((size_t)n + 1) * 8)))
        return s;
    P.src = d_src;
    P.in_off = d_in_off;
    P.n = n;
    P.max_block = m.max_block;
    P.max_buf = m.max_buf;
    P.ignore_id = m.ignore_id;
    P.blocks = m.blocks;
    if ((s = dev->mark(0))) return s;
    kc_launch_s2_plan(P, dev->stream);
    if ((s = dev->mark(1)) || (s = kc_dec_fetch(dev, H.nc, P.n_chunks, n)) || (s = kc_dec_fetch(dev, H.status, P.status, n)) ||
        (s = kc_dec_fetch(dev, H.bound, P.bound, n)) || (s = dev->sync()))
        return s;
    T.prep_ms += dev->span(0, 1);
    return KC_OK;
}

static const uint64_t kS2dPerChunk = sizeof(KcS2Chunk) + 4;  // device scratch one data chunk takes: its record and its verdict

// Returns KC_OK, KC_ERR_DST_TOO_SMALL (out_off holds the planned layout, nothing is written) or the device's error.
static inline int kc_s2d_decode(KcDecDevice* dev, const KcS2dMode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                uint64_t dst_cap, uint64_t* out_off, uint32_t* status, KcDecTimes& T) {
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    KcS2dPlan H;
    int s = kc_s2d_plan_inputs(dev, m, d_src, in_off, n, H, T);
    if (s != KC_OK) return s;
    const KcS2PlanParams& P = H.P;
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.bound[i];  // the planned layout
    if (out_off[n] > dst_cap) return KC_ERR_DST_TOO_SMALL;
    const uint64_t budget = dev->budget();
    std::vector<uint32_t> chunk0(n), cstatus;
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: inputs i0 .. i1 whose chunk records fit the budget (reserve() may over-allocate by 1/8) ----
        uint32_t i1 = i0, nc = 0;
        while (i1 < n) {
            const uint64_t all = ((uint64_t)nc + H.nc[i1]) * kS2dPerChunk;
            kc_dec_need(T, (uint64_t)H.nc[i1] * kS2dPerChunk);
            if (i1 > i0 && (all + (all >> 3) > budget || (uint64_t)nc + H.nc[i1] > 0x3FFFFFFFu)) break;
            chunk0[i1] = nc;
            nc += H.nc[i1];
            i1++;
        }
        const uint32_t nb = i1 - i0;
        if (nc) {
            KcS2PlanParams Q = P;  // second pass over this batch's inputs: the chunk records
            KcS2DecodeAllParams D;
            memset(&D, 0, sizeof(D));
            if ((s = kc_dec_reserve(dev, SD_CHUNKS, nc, &Q.chunks)) || (s = kc_dec_reserve(dev, SD_CSTATUS, nc, &D.status)) ||
                (s = dev->h2d(H.d_chunk0 + i0, chunk0.data() + i0, (size_t)nb * 4)) || (s = dev->h2d(H.d_out0 + i0, out_off + i0, (size_t)nb * 8)))
                return s;
            Q.in_off = P.in_off + i0;
            Q.n = nb;
            Q.chunk0 = H.d_chunk0 + i0;
            Q.out0 = H.d_out0 + i0;
            D.src = d_src;
            D.chunks = Q.chunks;
            D.n_chunks = nc;
            D.dst = d_dst;
            D.ignore_crc = m.ignore_crc;
            if ((s = dev->mark(0))) return s;
            kc_launch_s2_plan(Q, dev->stream);
            if ((s = dev->mark(1))) return s;
            kc_launch_s2_decode_all(D, dev->stream);
            if ((s = dev->mark(2)) || (s = kc_dec_fetch(dev, cstatus, (const uint32_t*)D.status, nc)) || (s = dev->sync())) return s;
            T.prep_ms += dev->span(0, 1);
            T.match_ms += dev->span(1, 2);
        }
        // ---- settle: the first failing chunk in stream order wins over the header-level error behind it (inside a chunk the
        // reference's order is DecodedLen, Snappy limit, max block — the plan — then decode, CRC — the kernel); a failed input's
        // planned range is zero-filled: no byte decoded from a corrupt stream stays in dst ----
        for (uint32_t i = i0; i < i1; i++) {
            uint32_t v = KCS2D_OK;
            for (uint32_t k = 0; k < H.nc[i] && !v; k++) v = cstatus[chunk0[i] + k];
            if (!v) v = H.status[i];
            status[i] = v;
            if (v && H.bound[i] && (s = dev->zero(d_dst + out_off[i], (size_t)H.bound[i]))) return s;
        }
        T.batches++;
        i0 = i1;
    }
    return dev->sync();
}
