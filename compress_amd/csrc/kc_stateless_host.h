#pragma once
// kc_stateless_host.h — host side of flate.StatelessDeflate / gzip.NewWriterLevel(w, gzip.StatelessCompression) over a batch of
// independent inputs, written against KcDecDevice alone (kc_stateless_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the
// wave emulator over plain memory).
//
// One call: the inputs are cut into groups whose scratch fits the budget — per block a record, and a token word for every byte and
// one more (the large item: four times the input); with a dictionary 32 KiB per input for the dictionary and the first block side
// by side.  match, plan and chain run per group and give every input's exact size; the prefix sum of the sizes IS the output layout
// (and DST_TOO_SMALL before anything is written); dst's range is zeroed, and emit runs per group (a call of more than one group
// runs match, plan and chain a second time per group: records and tokens are the scratch).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"
#include "kc_stateless_dev.h"

enum { SL_IN_OFF, SL_BLK0, SL_BLK_IN, SL_REC, SL_TOK, SL_TOK0, SL_SIZE, SL_CRC, SL_OUT0, SL_EDGE, SL_COUNTS, SL_DICT, SL_COMB, SL_N };

struct KcSlOpts {
    uint32_t eof = 1;            // StatelessDeflate's eof
    uint32_t gzip = 0;           // Write + Close of gzip.Writer at StatelessCompression: eof and the dictionary do not apply
    uint32_t penalty = 0;        // logNewTablePenalty of bitWriterPool's writers
    std::vector<uint8_t> dict;   // at most KCSL_MAX_DICT bytes: the reference truncates to the last 8192 (:93-95)
};

// blocks of an input of len bytes behind a dictionary of dict_len <= 8192 bytes (stateless.go:106-116)
static inline uint64_t kc_sl_blocks(uint64_t len, uint32_t dict_len) {
    const uint64_t first = KCSL_MAX_BLOCK - dict_len;
    return len == 0 ? 0 : len <= first ? 1 : 1 + (len - first + KCSL_LATER - 1) / KCSL_LATER;
}
static inline uint32_t kc_sl_records(uint64_t len, uint32_t dict_len) { return len ? (uint32_t)kc_sl_blocks(len, dict_len) : 1u; }

// kc_flate_stateless_bound (include/kcgpu.h).  Per block its bytes and 176:
//  - a block without a match is stored: 5 bytes, and up to 15 bits of an EOB owed to the table before it;
//  - writeBlockDynamic writes a dynamic, a reused-table or a fixed block only where its exact size in bits is BELOW the stored size.
//    Under a table in force (:661-703) size is exact when reuse wins (reuseSize) and the ESTIMATE newSize when a new table wins;
//    fixed is taken there only with fixedSize + 7 < size < ssize, so it is exact and below stored either way, and a reused table
//    only with reuseSize < ssize; where the estimate won and neither return was taken, control falls to the new-table part
//    (:706-758), which compares the exact dynamicSize and fixedSize with ssize again before it writes.  So such a block costs less
//    than a stored one, plus the EOB owed in front of it;
//  - a Huffman-only block (more than 15/16 of its bytes left as tokens) is writeBlockHuff's: taken against the 560-bit GUESS of its
//    header while a real header may reach 1880 bits, the 176 bytes of kc_flate_deflate_bound (the doubled estimate at penalty 0 only
//    makes the stored choice more frequent).
// 8 for the end: the empty stored block of a non-eof call (5 bytes behind up to 7 bits of padding) or the ten-bit block of an eof call
// on nothing.  gzip adds 10 + 8 and the two bytes of Close's eof call.
static inline uint64_t kc_sl_bound(uint64_t len, uint64_t dict_len) {
    const uint32_t d = (uint32_t)(dict_len < KCSL_MAX_DICT ? dict_len : KCSL_MAX_DICT);
    return len + 176 * kc_sl_blocks(len, d) + 8;
}
#define KCSL_GZIP_EXTRA 20u

struct KcSlPlan {
    KcStatelessParams P;
    std::vector<uint32_t> blk0, blk_in;
    std::vector<uint64_t> rel, tok0;
};

// match, plan and chain over the inputs i0 .. i1 (their sizes to size[i0 ...])
static inline int kc_sl_plan_group(KcDecDevice* dev, const KcSlOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t i0, uint32_t i1,
                                   const uint8_t* d_dict, uint32_t* d_counts, KcSlPlan& H, uint64_t* size, KcDecTimes& T) {
    const uint32_t n = i1 - i0;
    const uint32_t dict_len = o.gzip ? 0u : (uint32_t)o.dict.size();
    KcStatelessParams& P = H.P;
    memset(&P, 0, sizeof(P));
    H.blk0.assign((size_t)n + 1, 0);
    H.rel.resize((size_t)n + 1);
    H.blk_in.clear();
    H.tok0.clear();
    uint64_t ntok = 0;
    const uint64_t first = KCSL_MAX_BLOCK - dict_len;
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t len = in_off[i0 + k + 1] - in_off[i0 + k];
        const uint32_t nb = kc_sl_records(len, dict_len);
        H.blk0[k + 1] = H.blk0[k] + nb;
        H.blk_in.insert(H.blk_in.end(), nb, k);
        for (uint32_t b = 0; b < nb; b++) {  // a block's tokens: at most one per byte, and one word to spare
            const uint64_t pos = b == 0 ? 0 : first + (uint64_t)(b - 1) * KCSL_LATER, most = b == 0 ? first : KCSL_LATER;
            H.tok0.push_back(ntok);
            ntok += (len - pos < most ? len - pos : most) + 1;
        }
    }
    for (uint32_t k = 0; k <= n; k++) H.rel[k] = in_off[i0 + k] - in_off[i0];
    const uint32_t nblocks = H.blk0[n];
    uint64_t *d_in_off = nullptr, *d_tok0 = nullptr;
    uint32_t *d_blk0 = nullptr, *d_blk_in = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, SL_IN_OFF, (size_t)n + 1, &d_in_off)) || (s = kc_dec_reserve(dev, SL_BLK0, (size_t)n + 1, &d_blk0)) ||
        (s = kc_dec_reserve(dev, SL_BLK_IN, nblocks, &d_blk_in)) || (s = kc_dec_reserve(dev, SL_REC, nblocks, &P.rec)) ||
        (s = kc_dec_reserve(dev, SL_TOK, (size_t)ntok, &P.tok)) || (s = kc_dec_reserve(dev, SL_TOK0, nblocks, &d_tok0)) ||
        (s = kc_dec_reserve(dev, SL_SIZE, n, &P.size)) || (s = kc_dec_reserve(dev, SL_CRC, n, &P.crc)) ||
        (dict_len && (s = kc_dec_reserve(dev, SL_COMB, (size_t)n * KCSL_COMB, &P.comb))) ||
        (s = dev->h2d(d_in_off, H.rel.data(), ((size_t)n + 1) * 8)) || (s = dev->h2d(d_blk0, H.blk0.data(), ((size_t)n + 1) * 4)) ||
        (s = dev->h2d(d_blk_in, H.blk_in.data(), (size_t)nblocks * 4)) || (s = dev->h2d(d_tok0, H.tok0.data(), (size_t)nblocks * 8)))
        return s;
    P.src = d_src + in_off[i0];
    P.in_off = d_in_off; P.blk0 = d_blk0; P.blk_in = d_blk_in; P.tok0 = d_tok0;
    P.n = n; P.nblocks = nblocks;
    P.gzip = o.gzip; P.eof = o.gzip ? 0u : o.eof; P.penalty = o.penalty;
    P.dict = d_dict; P.dict_len = dict_len;
    P.counts = d_counts;
    kc_launch_stateless_gather(P, dev->stream);  // (a dictionary call only; in the call's time, in no kernel's)
    if ((s = dev->mark(0))) return s;
    kc_launch_stateless_match(P, dev->stream);
    if ((s = dev->mark(1))) return s;
    kc_launch_stateless_plan(P, dev->stream);
    if ((s = dev->mark(2))) return s;
    kc_launch_stateless_chain(P, dev->stream);
    if ((s = dev->mark(3)) || (s = dev->d2h(size + i0, P.size, (size_t)n * 8)) || (s = dev->sync())) return s;
    T.match_ms += dev->span(0, 1);
    T.prep_ms += dev->span(1, 2);
    T.other_ms += dev->span(2, 3);
    return KC_OK;
}

// emit over the group last planned, input k of it at d_dst + out0[k]; dst's range [0, total) is zero but for what earlier groups wrote
static inline int kc_sl_emit_group(KcDecDevice* dev, KcSlPlan& H, const uint64_t* out0, uint8_t* d_dst, uint64_t total, uint32_t* d_edge, KcDecTimes& T) {
    KcStatelessParams& P = H.P;
    uint64_t* d_out0 = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, SL_OUT0, P.n, &d_out0)) || (s = dev->h2d(d_out0, out0, (size_t)P.n * 8)) || (s = dev->mark(0))) return s;
    P.out0 = d_out0; P.dst = d_dst; P.total = total; P.edge = d_edge;
    kc_launch_stateless_emit(P, dev->stream);
    if ((s = dev->mark(1)) || (s = dev->sync())) return s;
    T.emit_ms += dev->span(0, 1);
    return KC_OK;
}

// Returns KC_OK, KC_ERR_DST_TOO_SMALL (out_off holds the exact layout, nothing is written), KC_ERR_UNSUPPORTED (an input beyond
// KCDF_MAX_INPUT, or one whose scratch alone exceeds the budget) or the device's error.  counts: null, or KCSL_N_COUNTS decision
// counters of the call (a call of several groups decides every block twice and counts it once).  Times: match_ms the match finder,
// prep_ms plan and chain, other_ms emit.
static inline int kc_sl_deflate(KcDecDevice* dev, const KcSlOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                uint64_t dst_cap, uint64_t* out_off, KcDecTimes& T, uint32_t* counts = nullptr) {
    out_off[0] = 0;
    if (counts) memset(counts, 0, KCSL_N_COUNTS * 4);
    if (n == 0) return KC_OK;
    if (o.dict.size() > KCSL_MAX_DICT) return KC_ERR_BAD_ARG;
    const uint32_t dict_len = o.gzip ? 0u : (uint32_t)o.dict.size();
    const uint64_t budget = dev->budget();
    const uint64_t per_input = 8 + 4 + 8 + 4 + 8 + (dict_len ? KCSL_COMB : 0u);  // offsets, sizes, CRCs, places, the dictionary slot
    const uint64_t fixed = KCSL_MAX_DICT + KCSL_N_COUNTS * 4 + 64;
    std::vector<uint32_t> cut(1, 0);  // the groups' first inputs
    uint64_t need = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = in_off[i + 1] - in_off[i];
        if (len > KCDF_MAX_INPUT) return KC_ERR_UNSUPPORTED;
        const uint64_t nrec = kc_sl_records(len, dict_len);
        const uint64_t mine = nrec * (sizeof(KcSlBlock) + 4 + 8 + 4) + len * 4 + per_input;
        kc_dec_need(T, mine + fixed);
        if (mine + fixed + ((mine + fixed) >> 3) > budget) return KC_ERR_UNSUPPORTED;
        if (need + mine + fixed + ((need + mine + fixed) >> 3) > budget || (need + mine) / sizeof(KcSlBlock) > 0x7fffffffu) { cut.push_back(i); need = 0; }
        need += mine;
    }
    cut.push_back(n);
    const size_t groups = cut.size() - 1;
    uint8_t* d_dict = nullptr;
    uint32_t *d_counts = nullptr, *d_edge = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, SL_COUNTS, KCSL_N_COUNTS, &d_counts)) || (s = dev->zero(d_counts, KCSL_N_COUNTS * 4)) ||
        (s = kc_dec_reserve(dev, SL_DICT, (size_t)KCSL_MAX_DICT, &d_dict)) || (dict_len && (s = dev->h2d(d_dict, o.dict.data(), dict_len))))
        return s;
    KcSlPlan H;
    std::vector<uint64_t> size(n);
    for (size_t g = 0; g < groups; g++)
        if ((s = kc_sl_plan_group(dev, o, d_src, in_off, cut[g], cut[g + 1], d_dict, d_counts, H, size.data(), T))) return s;
    if (counts && ((s = dev->d2h(counts, d_counts, KCSL_N_COUNTS * 4)) || (s = dev->sync()))) return s;
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + size[i];
    const uint64_t total = out_off[n];
    if (total > dst_cap) return KC_ERR_DST_TOO_SMALL;
    if ((s = kc_dec_reserve(dev, SL_EDGE, 2, &d_edge)) || (s = dev->zero(d_edge, 8)) || (s = dev->zero(d_dst, (size_t)total))) return s;
    for (size_t g = 0; g < groups; g++) {
        if (groups > 1 && (s = kc_sl_plan_group(dev, o, d_src, in_off, cut[g], cut[g + 1], d_dict, d_counts, H, size.data(), T))) return s;
        if ((s = kc_sl_emit_group(dev, H, out_off + cut[g], d_dst, total, d_edge, T))) return s;
    }
    T.batches = (int)groups;
    return KC_OK;
}
