#pragma once
// kc_deflate_host.h — host side of flate.NewWriter(w, HuffmanOnly) / gzip.NewWriterLevel(w, HuffmanOnly) over a batch of independent
// inputs, written against KcDecDevice alone (kc_deflate_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator
// over plain memory).
//
// One call: the inputs are cut into groups whose block records fit the scratch budget; plan and chain run per group and give every
// input's exact size; the prefix sum of the sizes IS the output layout (and DST_TOO_SMALL before anything is written); dst's range
// is zeroed, and emit runs per group (a call of more than one group plans each group a second time: the records are the scratch).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"
#include "kc_deflate_dev.h"

enum { DF_IN_OFF, DF_BLK0, DF_BLK_IN, DF_REC, DF_SIZE, DF_CRC, DF_OUT0, DF_EDGE, DF_N };

struct KcDfOpts {
    int level = -2;             // flate.HuffmanOnly, the one level served
    uint32_t end = KCDF_END_CLOSE;
    uint32_t block = 32768;     // compressor.init, flate/deflate.go:795-799: the window of this level ...
    uint32_t penalty = 10;      // ... and its logNewTablePenalty
    uint32_t gzip = 0;
};

// kc_flate_deflate_bound (include/kcgpu.h): per block its bytes and 176 (a stored block costs 5 and an owed EOB; a Huffman block is
// taken when bytes*8 + 40 exceeds its codes + the 560-bit header GUESS, while a real header may reach 17 + 19*3 + 258*7 = 1880 bits,
// and an owed EOB and its own add 30), 8 for the stream's end
static inline uint64_t kc_df_bound(uint64_t len, uint32_t block) {
    if (block == 0 || block > 65535) return 0;
    return len + 176 * ((len + block - 1) / block) + 8;
}
static inline uint32_t kc_df_records(uint64_t len, uint32_t block) { return len ? (uint32_t)((len + block - 1) / block) : 1u; }

struct KcDfPlan {
    KcDeflateParams P;
    std::vector<uint32_t> blk0, blk_in;
    std::vector<uint64_t> rel;
};

// plan and chain over the inputs i0 .. i1 (their sizes to size[i0 ...])
static inline int kc_df_plan_group(KcDecDevice* dev, const KcDfOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t i0, uint32_t i1,
                                   KcDfPlan& H, uint64_t* size, KcDecTimes& T) {
    const uint32_t n = i1 - i0;
    KcDeflateParams& P = H.P;
    memset(&P, 0, sizeof(P));
    H.blk0.assign((size_t)n + 1, 0);
    H.rel.resize((size_t)n + 1);
    H.blk_in.clear();
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t nb = kc_df_records(in_off[i0 + k + 1] - in_off[i0 + k], o.block);
        H.blk0[k + 1] = H.blk0[k] + nb;
        H.blk_in.insert(H.blk_in.end(), nb, k);
    }
    for (uint32_t k = 0; k <= n; k++) H.rel[k] = in_off[i0 + k] - in_off[i0];
    const uint32_t nblocks = H.blk0[n];
    uint64_t* d_in_off = nullptr;
    uint32_t *d_blk0 = nullptr, *d_blk_in = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, DF_IN_OFF, (size_t)n + 1, &d_in_off)) || (s = kc_dec_reserve(dev, DF_BLK0, (size_t)n + 1, &d_blk0)) ||
        (s = kc_dec_reserve(dev, DF_BLK_IN, nblocks, &d_blk_in)) || (s = kc_dec_reserve(dev, DF_REC, nblocks, &P.rec)) ||
        (s = kc_dec_reserve(dev, DF_SIZE, n, &P.size)) || (s = kc_dec_reserve(dev, DF_CRC, n, &P.crc)) ||
        (s = dev->h2d(d_in_off, H.rel.data(), ((size_t)n + 1) * 8)) || (s = dev->h2d(d_blk0, H.blk0.data(), ((size_t)n + 1) * 4)) ||
        (s = dev->h2d(d_blk_in, H.blk_in.data(), (size_t)nblocks * 4)))
        return s;
    P.src = d_src + in_off[i0];
    P.in_off = d_in_off; P.blk0 = d_blk0; P.blk_in = d_blk_in;
    P.n = n; P.nblocks = nblocks;
    P.gzip = o.gzip; P.end = o.end; P.block = o.block; P.penalty = o.penalty;
    if ((s = dev->mark(0))) return s;
    kc_launch_deflate_plan(P, dev->stream);
    if ((s = dev->mark(1))) return s;
    kc_launch_deflate_chain(P, dev->stream);
    if ((s = dev->mark(2)) || (s = dev->d2h(size + i0, P.size, (size_t)n * 8)) || (s = dev->sync())) return s;
    T.prep_ms += dev->span(0, 1);
    T.other_ms += dev->span(1, 2);
    return KC_OK;
}

// emit over the group last planned, input k of it at d_dst + out0[k]; dst's range [0, total) is zero but for what earlier groups wrote
static inline int kc_df_emit_group(KcDecDevice* dev, KcDfPlan& H, const uint64_t* out0, uint8_t* d_dst, uint64_t total, uint32_t* d_edge, KcDecTimes& T) {
    KcDeflateParams& P = H.P;
    uint64_t* d_out0 = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, DF_OUT0, P.n, &d_out0)) || (s = dev->h2d(d_out0, out0, (size_t)P.n * 8)) || (s = dev->mark(2))) return s;
    P.out0 = d_out0; P.dst = d_dst; P.total = total; P.edge = d_edge;
    kc_launch_deflate_emit(P, dev->stream);
    if ((s = dev->mark(3)) || (s = dev->sync())) return s;
    T.match_ms += dev->span(2, 3);
    return KC_OK;
}

// Returns KC_OK, KC_ERR_DST_TOO_SMALL (out_off holds the exact layout, nothing is written), KC_ERR_UNSUPPORTED (an input beyond
// KCDF_MAX_INPUT, or one whose records alone exceed the scratch budget) or the device's error.
static inline int kc_df_deflate(KcDecDevice* dev, const KcDfOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                uint64_t dst_cap, uint64_t* out_off, KcDecTimes& T) {
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    const uint64_t budget = dev->budget();
    const uint64_t per_input = 8 + 4 + 8 + 4 + 8;  // offsets, sizes, CRCs, places
    std::vector<uint32_t> cut(1, 0);  // the groups' first inputs
    uint64_t need = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = in_off[i + 1] - in_off[i];
        if (len > KCDF_MAX_INPUT) return KC_ERR_UNSUPPORTED;
        const uint64_t mine = (uint64_t)kc_df_records(len, o.block) * (sizeof(KcDfBlock) + 4) + per_input;
        kc_dec_need(T, mine + 64);
        if (mine + 64 + ((mine + 64) >> 3) > budget) return KC_ERR_UNSUPPORTED;
        if (need + mine + 64 + ((need + mine + 64) >> 3) > budget || (need + mine) / sizeof(KcDfBlock) > 0x7fffffffu) { cut.push_back(i); need = 0; }
        need += mine;
    }
    cut.push_back(n);
    const size_t groups = cut.size() - 1;
    KcDfPlan H;
    std::vector<uint64_t> size(n);
    int s;
    for (size_t g = 0; g < groups; g++)
        if ((s = kc_df_plan_group(dev, o, d_src, in_off, cut[g], cut[g + 1], H, size.data(), T))) return s;
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + size[i];
    const uint64_t total = out_off[n];
    if (total > dst_cap) return KC_ERR_DST_TOO_SMALL;
    uint32_t* d_edge = nullptr;
    if ((s = kc_dec_reserve(dev, DF_EDGE, 2, &d_edge)) || (s = dev->zero(d_edge, 8)) || (s = dev->zero(d_dst, (size_t)total))) return s;
    for (size_t g = 0; g < groups; g++) {
        if (groups > 1 && (s = kc_df_plan_group(dev, o, d_src, in_off, cut[g], cut[g + 1], H, size.data(), T))) return s;
        if ((s = kc_df_emit_group(dev, H, out_off + cut[g], d_dst, total, d_edge, T))) return s;
    }
    T.batches = (int)groups;
    return KC_OK;
}
