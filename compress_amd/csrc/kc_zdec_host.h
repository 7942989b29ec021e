#pragma once
// kc_zdec_host.h — host side of zstd.Decoder.DecodeAll over a batch of independent inputs, written against KcDecDevice alone
// (kc_zstd_dec_api.cpp runs it on the device, tools/hipemu/kcemu.cpp on the wave emulator over plain memory).
//
// One call: the plan kernel sizes every input (kc_zstd_plan.hip, first pass); the inputs are cut into batches whose staging fits the
// device's scratch budget; per batch the plan's second pass writes the frame records, the decode kernel decodes one frame per wave
// into its staging slot (kc_zstd_decode_all.hip), XXH64 of every decoded frame is taken, the host settles each input (first error in
// the reference's order, size limit, checksum) and kc_compact_kernel moves the frames of the inputs that stand into the dense
// output.  A failing input therefore never reaches dst at all.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"

enum { ZD_IN_OFF, ZD_NF, ZD_BOUND, ZD_SLOTB, ZD_EXACT, ZD_STATUS, ZD_FRAME0, ZD_SLOT0, ZD_FRAMES, ZD_STAGE, ZD_LITS, ZD_DICTS, ZD_ARENA,
       ZD_FSIZE, ZD_FSTATUS, ZD_FCRC, ZD_HASHOFF, ZD_HASH, ZD_COFF, ZD_CSIZE, ZD_N };  // ZD_COFF holds slot offsets then output offsets

// decoderOptions: what DecodeAll and the stream reader (kc_zdstream_host.h) both read
struct KcZdOpts {
    uint64_t max_memory = (uint64_t)64 << 30;   // decoderOptions.maxDecodedSize
    uint64_t max_window = (uint64_t)1 << 29;    // decoderOptions.maxWindowSize (MaxWindowSize)
    int ignore_checksum = 0;
    std::vector<KcZdDict> dicts;                // content_off = the dictionary's place in `arena`
    std::vector<uint8_t> arena;                 // the dictionaries' contents, each 16-byte aligned
};

// registers D with its content; -1: refused (dictMaxLength, or no memory)
static inline int kc_zd_add_dict(KcZdOpts& o, KcZdDict& D, const uint8_t* content, uint64_t len) {
    if (len > ((uint64_t)1 << 31)) return -1;  // dictMaxLength
    try {
        const size_t at = (o.arena.size() + 15) & ~(size_t)15;
        o.arena.resize(at + (size_t)len);
        if (len) memcpy(o.arena.data() + at, content, (size_t)len);
        D.content_off = at;
        D.content_len = (uint32_t)len;
        o.dicts.push_back(D);
    } catch (...) {
        return -1;
    }
    return 0;
}
// a raw dictionary (WithDecoderDictRaw, zstd/decoder_options.go:131-142)
static inline int kc_zd_add_dict_raw(KcZdOpts& o, uint32_t id, const uint8_t* content, uint64_t len) {
    KcZdDict D;
    memset(&D, 0, sizeof(D));
    D.id = id;
    D.rep[0] = 1; D.rep[1] = 4; D.rep[2] = 8;
    return kc_zd_add_dict(o, D, content, len);
}

// One input after the decode kernel, frame by frame in the order the reference meets them (zstd/decoder.go:342-408): the size limit
// against what the input has produced so far (exact only now, when an earlier frame carried no content size), the frame's own
// error, its checksum (hash[2 * f] = XXH64 of its decoded bytes), the running total.  Returns the input's status; *total = its
// decoded bytes when that is 0.
static inline uint32_t kc_zd_settle_input(const KcZdFrame* fr, const uint32_t* fstatus, const uint32_t* fsize, const uint32_t* crc_stored,
                                          const uint64_t* hash, uint32_t nf, uint64_t max_memory, bool ignore_checksum, uint64_t* total) {
    uint64_t produced = 0;
    for (uint32_t f = 0; f < nf; f++) {
        if (fr[f].fcs != KC_ZD_NO_SIZE && fr[f].fcs > max_memory - produced) return KCZD_SIZE;
        if (fstatus[f]) return fstatus[f];
        if (fr[f].checksum && !ignore_checksum && (uint32_t)hash[2 * (size_t)f] != crc_stored[f]) return KCZD_CRC;
        produced += fsize[f];
        if (produced > max_memory) return KCZD_SIZE;
    }
    *total = produced;
    return KCZD_OK;
}

// the plan's first pass: its parameters (the arrays on the device) and its results on the host
struct KcZdPlan {
    KcZdPlanParams P;
    std::vector<uint32_t> nf, exact, status;
    std::vector<uint64_t> bound, slotb;
    uint32_t* d_frame0 = nullptr;
    uint64_t* d_slot0 = nullptr;
    const uint8_t* d_arena = nullptr;
};

// the plan's first pass over all inputs.  The inputs' offsets and the dictionaries stay on the device.
static inline int kc_zd_plan_inputs(KcDecDevice* dev, const KcZdOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcZdPlan& H,
                                    KcDecTimes& T) {
    KcZdPlanParams& P = H.P;
    memset(&P, 0, sizeof(P));
    uint64_t* d_in_off = nullptr;
    int s;
    if ((s = kc_dec_reserve(dev, ZD_IN_OFF, (size_t)n + 1, &d_in_off)) || (s = kc_dec_reserve(dev, ZD_NF, n, &P.n_frames)) ||
        (s = kc_dec_reserve(dev, ZD_BOUND, n, &P.bound)) || (s = kc_dec_reserve(dev, ZD_SLOTB, n, &P.slot_bytes)) ||
        (s = kc_dec_reserve(dev, ZD_EXACT, n, &P.exact)) || (s = kc_dec_reserve(dev, ZD_STATUS, n, &P.status)) ||
        (s = kc_dec_reserve(dev, ZD_FRAME0, n, &H.d_frame0)) || (s = kc_dec_reserve(dev, ZD_SLOT0, n, &H.d_slot0)) ||
        (s = dev->h2d(d_in_off, in_off, ((size_t)n + 1) * 8)))
        return s;
    if (!o.dicts.empty()) {
        KcZdDict* d_dicts = nullptr;
        uint8_t* d_arena = nullptr;
        if ((s = kc_dec_reserve(dev, ZD_DICTS, o.dicts.size(), &d_dicts)) || (s = kc_dec_reserve(dev, ZD_ARENA, o.arena.size() + 16, &d_arena)) ||
            (s = dev->h2d(d_dicts, o.dicts.data(), o.dicts.size() * sizeof(KcZdDict))) || (s = dev->h2d(d_arena, o.arena.data(), o.arena.size())))
            return s;
        P.dicts = d_dicts;
        P.n_dicts = (uint32_t)o.dicts.size();
        H.d_arena = d_arena;
    }
    P.src = d_src;
    P.in_off = d_in_off;
    P.n = n;
    P.max_memory = o.max_memory;
    P.max_window = o.max_window;
    if ((s = dev->mark(0))) return s;
    kc_launch_zstd_plan(P, dev->stream);
    if ((s = dev->mark(1)) || (s = kc_dec_fetch(dev, H.nf, P.n_frames, n)) || (s = kc_dec_fetch(dev, H.exact, P.exact, n)) ||
        (s = kc_dec_fetch(dev, H.status, P.status, n)) || (s = kc_dec_fetch(dev, H.bound, P.bound, n)) ||
        (s = kc_dec_fetch(dev, H.slotb, P.slot_bytes, n)) || (s = dev->sync()))
        return s;
    T.prep_ms += dev->span(0, 1);
    return KC_OK;
}

// device scratch one frame takes besides its staging slot: literal scratch, its record and the per-frame result / compaction arrays
static const uint64_t kZdPerFrame = (uint64_t)KC_ZD_LIT_STRIDE + sizeof(KcZdFrame) + 4 * 4 + 8 * 5 + 64;

// Returns KC_OK, KC_ERR_DST_TOO_SMALL (the inputs settled so far are in dst) or the device's error.
static inline int kc_zd_decode_all(KcDecDevice* dev, const KcZdOpts& o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                   uint64_t dst_cap, uint64_t* out_off, uint32_t* status, KcDecTimes& T) {
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    KcZdPlan H;
    int s = kc_zd_plan_inputs(dev, o, d_src, in_off, n, H, T);
    if (s != KC_OK) return s;
    const KcZdPlanParams& P = H.P;
    const uint64_t budget = dev->budget();
    auto input_scratch = [&](uint32_t i) { return H.slotb[i] + (uint64_t)H.nf[i] * kZdPerFrame; };
    std::vector<uint32_t> frame0(n);
    std::vector<uint64_t> slot0(n);
    std::vector<KcZdFrame> fr;
    std::vector<uint32_t> fsize, fstatus, fcrc, csize;
    std::vector<uint64_t> hash, coff;
    uint64_t pos = 0;  // bytes of dst used
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: inputs i0 .. i1 whose staging and per-frame scratch fit the budget (reserve() may over-allocate by 1/8) ----
        uint32_t i1 = i0, nf = 0;
        uint64_t scratch = 0, slots = 0;
        while (i1 < n) {
            if (H.status[i1] == 0 && H.nf[i1]) {
                const uint64_t us = input_scratch(i1);
                kc_dec_need(T, us);
                if (us + (us >> 3) > budget) {  // cannot be decoded within the budget even alone: the second pass must skip it too
                    H.status[i1] = KCZD_SIZE;
                    if ((s = dev->h2d(P.status + i1, &H.status[i1], 4)) || (s = dev->sync())) return s;
                    i1++;
                    continue;
                }
                if (nf && ((scratch + us) + ((scratch + us) >> 3) > budget || (uint64_t)nf + H.nf[i1] > 0x3FFFFFFFu)) break;
                frame0[i1] = nf;
                slot0[i1] = slots;
                scratch += us;
                slots += H.slotb[i1];
                nf += H.nf[i1];
            }
            i1++;
        }
        const uint32_t nb = i1 - i0;
        std::vector<uint64_t> total(nb, 0);
        uint8_t* d_stage = nullptr;
        uint64_t* d_coff = nullptr;
        uint32_t* d_csize = nullptr;
        if (nf) {
            KcZdPlanParams Q = P;  // second pass over this batch's inputs: the frame records
            KcZdDecodeParams D;
            memset(&D, 0, sizeof(D));
            uint64_t* d_hash = nullptr;
            if ((s = kc_dec_reserve(dev, ZD_FRAMES, nf, &Q.frames)) || (s = kc_dec_reserve(dev, ZD_STAGE, (size_t)slots + 64, &d_stage)) ||
                (s = kc_dec_reserve(dev, ZD_LITS, (size_t)nf * KC_ZD_LIT_STRIDE, &D.lits)) || (s = kc_dec_reserve(dev, ZD_FSIZE, nf, &D.out_size)) ||
                (s = kc_dec_reserve(dev, ZD_FSTATUS, nf, &D.status)) || (s = kc_dec_reserve(dev, ZD_FCRC, nf, &D.crc_stored)) ||
                (s = kc_dec_reserve(dev, ZD_HASHOFF, (size_t)nf * 2 + 1, &D.hash_off)) || (s = kc_dec_reserve(dev, ZD_HASH, (size_t)nf * 2, &d_hash)) ||
                (s = kc_dec_reserve(dev, ZD_COFF, (size_t)nf * 2, &d_coff)) || (s = kc_dec_reserve(dev, ZD_CSIZE, nf, &d_csize)) ||
                (s = dev->h2d(H.d_frame0 + i0, frame0.data() + i0, (size_t)nb * 4)) || (s = dev->h2d(H.d_slot0 + i0, slot0.data() + i0, (size_t)nb * 8)))
                return s;
            Q.in_off = P.in_off + i0;
            Q.n = nb;
            Q.status = P.status + i0;
            Q.frame0 = H.d_frame0 + i0;
            Q.slot0 = H.d_slot0 + i0;
            D.src = d_src;
            D.frames = Q.frames;
            D.n_frames = nf;
            D.stage = d_stage;
            D.dicts = P.dicts;
            D.dict_arena = H.d_arena;
            D.max_memory = o.max_memory;
            if ((s = dev->mark(0))) return s;
            kc_launch_zstd_plan(Q, dev->stream);
            if ((s = dev->mark(1))) return s;
            kc_launch_zstd_decode_all(D, dev->stream);
            if ((s = dev->mark(2))) return s;
            // XXH64 of every decoded frame: the even "units" of hash_off (the odd ones are the unused rests of the slots)
            if (!o.ignore_checksum) {
                dev->lane_group(4);  // (one unit per quad; the quads' trip counts differ)
                kc_launch_xxh64(D.stage, D.hash_off, 2 * nf - 1, d_hash, dev->stream);
                dev->lane_group(64);
            }
            hash.assign((size_t)nf * 2, 0);
            coff.resize((size_t)nf * 2);
            csize.resize(nf);
            if ((s = dev->mark(3)) || (s = kc_dec_fetch(dev, fr, (const KcZdFrame*)Q.frames, nf)) || (s = kc_dec_fetch(dev, fsize, (const uint32_t*)D.out_size, nf)) ||
                (s = kc_dec_fetch(dev, fstatus, (const uint32_t*)D.status, nf)) || (s = kc_dec_fetch(dev, fcrc, (const uint32_t*)D.crc_stored, nf)) ||
                (!o.ignore_checksum && (s = dev->d2h(hash.data(), d_hash, ((size_t)nf * 2 - 1) * 8))) || (s = dev->sync()))
                return s;
            T.prep_ms += dev->span(0, 1);
            T.match_ms += dev->span(1, 2);
            T.other_ms += dev->span(2, 3);
        }
        // ---- settle the inputs; where their frames go ----
        uint64_t need = 0;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t i = i0 + k;
            if (H.status[i] == 0 && H.nf[i]) {
                const uint32_t f0 = frame0[i];
                H.status[i] = kc_zd_settle_input(fr.data() + f0, fstatus.data() + f0, fsize.data() + f0, fcrc.data() + f0, hash.data() + 2 * (size_t)f0,
                                                 H.nf[i], o.max_memory, o.ignore_checksum != 0, &total[k]);
                if (H.status[i]) total[k] = 0;
            }
            need += total[k];
        }
        if (pos + need > dst_cap) return KC_ERR_DST_TOO_SMALL;
        for (uint32_t f = 0; f < nf; f++) { coff[f] = fr[f].slot_off; coff[(size_t)nf + f] = 0; csize[f] = 0; }  // (a failed input's frames stay in their slots)
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t i = i0 + k;
            status[i] = H.status[i];
            if (H.status[i] == 0 && H.nf[i]) {
                uint64_t at = pos;
                for (uint32_t f = frame0[i]; f < frame0[i] + H.nf[i]; f++) { coff[(size_t)nf + f] = at; csize[f] = fsize[f]; at += fsize[f]; }
            }
            pos += total[k];
            out_off[i + 1] = pos;
        }
        if (nf && need) {
            if ((s = dev->h2d(d_coff, coff.data(), (size_t)nf * 2 * 8)) || (s = dev->h2d(d_csize, csize.data(), (size_t)nf * 4)) || (s = dev->mark(0))) return s;
            kc_launch_compact(d_stage, d_coff, d_csize, d_coff + nf, d_dst, nf, dev->stream);
            if ((s = dev->mark(1)) || (s = dev->sync())) return s;
            T.other_ms += dev->span(0, 1);
        }
        T.batches++;
        i0 = i1;
    }
    return KC_OK;
}
