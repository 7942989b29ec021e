#pragma once
// kc_zdstream_host.h — host logic of the zstd stream reader that needs no device of its own: the state machine behind
// kc_zstd_dstream_feed (kc_zstd_dstream_api.cpp; the wave emulator's wrapper tools/hipemu/kcemu.cpp runs the same machine over
// plain memory).  It follows the reference's stream decoder (zstd/decoder.go:486-567 nextBlockSync, :649-940 startStreamDecoder,
// framedec.go:65-278 reset, blockdec.go:122-212 the block header) and hands the device runs of whole blocks of one frame.
//
// The walk reads only fixed-position bytes of a block — its 3-byte header, the literals header, the sequence count and the modes
// byte; the last three by the functions the kernels read them with (kc_zblock_dev.h) —, sizes the block's literal and sequence slices exactly and names, for each of the four tables, where a block that repeats it
// finds it: the block itself, the earlier block of the launch that last defined it, or the stream's carried state.
//
// Verdicts where the stream form differs from DecodeAll's:
//   * a window above WithDecoderMaxWindow, or above WithDecoderMaxMemory, is KC_ZD_SIZE_EXCEEDED (decoder.go:500, :861-866:
//     ErrDecoderSizeExceeded), not KC_ZD_WINDOW_EXCEEDED.  (The reference's framedec.go:232 still names ErrWindowSizeExceeded for a
//     window descriptor above the maximum before decoder.go:500 gets to look; the class here is the one the stream decoder states.)
//   * WithDecoderMaxMemory bounds the window only, never what a stream returns in total;
//   * more bytes than Frame_Content_Size, or fewer at the last block (decoder.go:529-545, :794-801: ErrFrameSizeExceeded /
//     ErrFrameSizeMismatch), are KC_ZD_CORRUPT.
// Deviations: a stream frame has no 4 GiB limit (positions are 64-bit); the block that overruns Frame_Content_Size is not handed out
// in front of its error (the reference's asynchronous form hands it out).
// The dictionary: its content sits in front of the history buffer until the frame's output has slid out of it for the first time;
// from then on it is out of reach (the reference's streamed history is cut to the window likewise), so an offset that reaches into
// the dictionary once more than `window` + one launch of output lies in front of it is KC_ZD_CORRUPT.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_zdec_host.h"
#include "kc_zblock_dev.h"

// The stream's buffers on its device (kc_decdev_host.h).
enum { ZS_IN, ZS_RECS, ZS_LITS, ZS_SEQS, ZS_WTS, ZS_STAT, ZS_TAB, ZS_HASH, ZS_HIST0, ZS_HIST1, ZS_DICT, ZS_N };

struct KcZsOpts : KcZdOpts {
    uint32_t blocks = 512;               // blocks per launch (KC_OPT_DSTREAM_BLOCKS)
};

struct KcZsStream {
    enum { BETWEEN, SKIP, BLOCKS, CHECKSUM, FAILED, DONE };
    KcDecDevice* dev = nullptr;
    KcZsOpts o;
    int state = BETWEEN;
    uint32_t fail = 0;
    uint64_t skip_left = 0;
    // the frame
    uint64_t window = 0, fcs = KC_ZD_NO_SIZE, decoded = 0;
    bool checksum = false, fresh = false, dict_live = false;
    uint32_t dict = 0;                   // index + 1
    uint32_t dict_loaded = 0;            // the dictionary whose content B_DICT holds
    // the device state
    int cur = 0, sel = 0;
    uint64_t kept = 0, hist_cap[2] = {0, 0};
    void* hist[2] = {nullptr, nullptr};
    uint64_t digest = 0;
    // sources of copies in flight
    std::vector<KcZsBlock> recs;
    std::vector<uint32_t> stat;
    uint64_t result[2] = {0, 0};
    KcZsTables tab0;
    KcZsHash hash0;

    void reset() {
        state = BETWEEN; fail = 0; skip_left = 0; kept = 0; fresh = false; dict_live = false;
    }

    // ---- the frame header (framedec.go:65-278), consumed only when whole.  Returns the bytes it takes behind the magic, 0 when
    // more are needed, -1 with *cls on an error ----
    int frame_header(const uint8_t* p, uint64_t n, uint32_t* cls) {
        uint64_t pos = 0;
        if (n < 1) return 0;
        const uint32_t fhd = p[pos++];
        const bool single = ((fhd >> 5) & 1u) != 0u;
        if (fhd & 8u) { *cls = KCZD_CORRUPT; return -1; }  // reserved bit
        uint64_t w = 0;
        if (!single) {
            if (n - pos < 1) return 0;
            const uint32_t wd = p[pos++];
            const uint64_t base = (uint64_t)1 << (10 + (wd >> 3));
            w = base + (base / 8) * (wd & 7u);
        }
        uint32_t did = 0;
        const uint32_t dsz = (fhd & 3u) == 3u ? 4u : (fhd & 3u);
        if (n - pos < dsz) return 0;
        for (uint32_t k = 0; k < dsz; k++) did |= (uint32_t)p[pos + k] << (8 * k);
        pos += dsz;
        uint64_t f = KC_ZD_NO_SIZE;
        const uint32_t v = fhd >> 6;
        const uint32_t fsz = v == 0 ? (single ? 1u : 0u) : (1u << v);
        if (n - pos < fsz) return 0;
        if (fsz) {
            f = 0;
            for (uint32_t k = 0; k < fsz; k++) f |= (uint64_t)p[pos + k] << (8 * k);
            if (fsz == 2) f += 256;
            pos += fsz;
        }
        if (w > o.max_window || w > o.max_memory) { *cls = KCZD_SIZE; return -1; }
        if (w == 0 && single) {
            w = f > 1024 ? f : 1024;
            if (w > o.max_memory || w > o.max_window) { *cls = KCZD_SIZE; return -1; }
        }
        if (w < 1024) { *cls = KCZD_CORRUPT; return -1; }
        uint32_t dk = 0;
        for (uint32_t k = 0; k < (uint32_t)o.dicts.size(); k++) if (o.dicts[k].id == did) dk = k + 1;  // (a later registration replaces an earlier one)
        if (dk == 0 && did != 0) { *cls = KCZD_UNKNOWN_DICT; return -1; }
        window = w; fcs = f; decoded = 0; checksum = ((fhd >> 2) & 1u) != 0u; dict = dk;
        fresh = true;
        return (int)pos;
    }

    // ---- the fixed-position bytes of a compressed block, by the functions the kernel reads them with (kc_zblock_dev.h): the kernel
    // refuses a block whose record says otherwise ----
    void walk_compressed(const uint8_t* b, KcZsBlock& R) const {
        R.parsed = 0;
        ZdLitHdr h;
        if (zd_lit_header(b, (int)R.size, window, h)) return;
        const uint8_t* sp = b + h.hdr + h.comp;
        const int sn = (int)R.size - h.hdr - h.comp;
        int nseq = 0, sh = 0;
        if (zd_seq_count(sp, sn, nseq, sh)) return;
        if (nseq > 0 && sn - sh < 1) return;
        R.ltype = (uint32_t)h.ltype; R.regen = h.regen; R.comp = (uint32_t)h.comp; R.lhdr = (uint32_t)h.hdr; R.nseq = (uint32_t)nseq; R.shdr = (uint32_t)sh;
        R.modes = nseq ? sp[sh] : 0;
        R.parsed = 1;
    }

    void set_fail(uint32_t cls, uint32_t* status) { state = FAILED; fail = cls; *status = cls; }

    // One launch: blocks recs[0 .. count) of the current frame, whose bytes are in[0 .. in_len).  The bytes of the blocks in front of
    // the first failing one go to dst.  Returns a kc_status; *cls = the failing block's class (the stream is then failed).
    int launch(const uint8_t* in, uint64_t in_len, uint64_t need, bool has_last, uint8_t* dst, uint64_t* produced, uint32_t* cls) {
        const uint32_t count = (uint32_t)recs.size();
        int s;
        *cls = 0;
        // ---- the slices, the table sources, the last definers ----
        uint64_t lits = 0, seqs = 0, wts = 0;
        uint32_t last_def[4] = {KC_ZS_CARRIED, KC_ZS_CARRIED, KC_ZS_CARRIED, KC_ZS_CARRIED}, huf_wt = 0;
        for (uint32_t i = 0; i < count; i++) {
            KcZsBlock& R = recs[i];
            R.def = 0; R.wt_bytes = 0; R.wt_off = 0; R.lit_off = 0; R.seq_off = 0;
            for (int k = 0; k < 4; k++) R.src[k] = KC_ZS_CARRIED;
            if (R.type != 2 || !R.parsed) continue;
            if (R.ltype >= 2) { R.lit_off = lits; lits += R.regen; }
            if (R.ltype == 2) {
                R.src[KC_ZS_HUF] = KC_ZS_OWN;
                last_def[KC_ZS_HUF] = i;
                huf_wt = 0;
                const uint8_t* q = in + R.pos + R.lhdr;  // FSE-compressed weights: the table log is the description's first nibble
                if (R.comp >= 2 && q[0] > 0 && q[0] < 128 && (q[1] & 15u) + 5u > 7u) huf_wt = (4u << ((q[1] & 15u) + 5u)) + 4u;
                R.wt_bytes = huf_wt;
            } else if (R.ltype == 3) {
                R.src[KC_ZS_HUF] = last_def[KC_ZS_HUF];
                if (last_def[KC_ZS_HUF] != KC_ZS_CARRIED) R.wt_bytes = huf_wt;
            }
            if (R.wt_bytes) { R.wt_off = wts; wts += (R.wt_bytes + 3u) & ~3u; }
            if (R.nseq) {
                R.seq_off = seqs;
                seqs += 3 * (uint64_t)R.nseq;
                for (int kind = 0; kind < 3; kind++) {
                    if (zd_seq_mode(R.modes, kind) == 3) R.src[KC_ZS_LL + kind] = last_def[KC_ZS_LL + kind];
                    else { R.src[KC_ZS_LL + kind] = KC_ZS_OWN; last_def[KC_ZS_LL + kind] = i; }
                }
            }
        }
        uint32_t def_mask = 0;
        for (int k = 0; k < 4; k++) if (last_def[k] != KC_ZS_CARRIED) { recs[last_def[k]].def |= 1u << k; def_mask |= 1u << k; }
        // ---- device buffers ----
        void *d_in, *d_recs, *d_lits, *d_seqs, *d_wts, *d_stat, *d_tab, *d_hash, *d_dict = nullptr;
        if ((s = dev->reserve(ZS_IN, (size_t)in_len + 64, &d_in)) || (s = dev->reserve(ZS_RECS, (size_t)count * sizeof(KcZsBlock), &d_recs)) ||
            (s = dev->reserve(ZS_LITS, (size_t)lits + 64, &d_lits)) || (s = dev->reserve(ZS_SEQS, (size_t)seqs * 4 + 64, &d_seqs)) ||
            (s = dev->reserve(ZS_WTS, (size_t)wts + 64, &d_wts)) || (s = dev->reserve(ZS_STAT, 16 + (size_t)count * 12, &d_stat)) ||
            (s = dev->reserve(ZS_TAB, 2 * sizeof(KcZsTables), &d_tab)) || (s = dev->reserve(ZS_HASH, sizeof(KcZsHash), &d_hash)))
            return s;
        KcZsTables* tabs = (KcZsTables*)d_tab;
        if (fresh) {  // the frame's first launch: no tables, or the dictionary's; its offset history; a new checksum; an empty history
            fresh = false;
            kept = 0;
            dict_live = false;
            memset(&tab0, 0, sizeof(tab0));
            tab0.rep[0] = 1; tab0.rep[1] = 4; tab0.rep[2] = 8;
            if (dict) {
                const KcZdDict& D = o.dicts[dict - 1];
                for (int k = 0; k < 3; k++) tab0.rep[k] = D.rep[k];
                if (D.full) {  // the dictionary's tables are the "previous" tables of the first block (history.setDict)
                    memcpy(tab0.huf, D.huf, sizeof(D.huf));
                    memcpy(tab0.ll, D.ll, sizeof(D.ll));
                    memcpy(tab0.of, D.of, sizeof(D.of));
                    memcpy(tab0.ml, D.ml, sizeof(D.ml));
                    tab0.huf_log = D.huf_log; tab0.huf_ok = 1;
                    tab0.log[0] = D.ll_log; tab0.log[1] = D.of_log; tab0.log[2] = D.ml_log;
                    tab0.ok[0] = tab0.ok[1] = tab0.ok[2] = 1;
                }
                dict_live = D.content_len != 0;
                if (dict_live && dict_loaded != dict) {
                    dict_loaded = 0;
                    if ((s = dev->reserve(ZS_DICT, (size_t)D.content_len + 64, &d_dict)) ||
                        (s = dev->h2d(d_dict, o.arena.data() + D.content_off, D.content_len)))
                        return s;
                    dict_loaded = dict;
                }
            }
            memset(&hash0, 0, sizeof(hash0));
            hash0.v[0] = 11400714785074694791ULL + 14029467366897019727ULL;  // xxhash.go Reset: prime1 + prime2, prime2, 0, -prime1
            hash0.v[1] = 14029467366897019727ULL;
            hash0.v[3] = 0ULL - 11400714785074694791ULL;
            if ((s = dev->h2d(&tabs[cur], &tab0, sizeof(tab0))) || (s = dev->h2d(d_hash, &hash0, sizeof(hash0)))) return s;
        }
        if (dict_live) {
            if ((s = dev->reserve(ZS_DICT, (size_t)o.dicts[dict - 1].content_len + 64, &d_dict))) return s;
        }
        // ---- the history buffer: up to `window` bytes of what came before, then room for this launch ----
        if (kept + need > hist_cap[sel]) {
            const uint64_t keep = kept < window ? kept : window;
            const int other = sel ^ 1;
            const uint64_t want = (keep > window ? keep : window) + need;
            if (keep == 0 && hist_cap[sel] == 0) {  // (nothing to move)
                if ((s = dev->reserve(ZS_HIST0 + sel, (size_t)(need + 64), &hist[sel]))) return s;
                hist_cap[sel] = need;
            } else {
                // the slide goes into the second buffer: source and destination never overlap
                if (hist_cap[other] < keep + need) {
                    if ((s = dev->reserve(ZS_HIST0 + other, (size_t)(want + 64), &hist[other]))) return s;
                    hist_cap[other] = want;
                }
                if (keep && (s = dev->d2d(hist[other], (const uint8_t*)hist[sel] + (kept - keep), (size_t)keep))) return s;
                if (keep < kept) dict_live = false;  // the frame has slid: the dictionary is out of reach from here on
                sel = other;
                kept = keep;
            }
        }
        // ---- copies in, the three kernels, the verdicts out ----
        uint64_t* d_result = (uint64_t*)d_stat;
        uint32_t* d_est = (uint32_t*)((uint8_t*)d_stat + 16);
        uint32_t* d_xst = d_est + count;
        uint32_t* d_osz = d_xst + count;
        if ((s = dev->h2d(d_in, in, (size_t)in_len)) || (s = dev->h2d(d_recs, recs.data(), (size_t)count * sizeof(KcZsBlock)))) return s;
        KcZsEntropyParams E;
        memset(&E, 0, sizeof(E));
        E.in = (const uint8_t*)d_in; E.in_len = in_len; E.blocks = (const KcZsBlock*)d_recs; E.n_blocks = count; E.window = window;
        E.lits = (uint8_t*)d_lits; E.lits_len = lits; E.seqs = (uint32_t*)d_seqs; E.seqs_len = seqs; E.wts = (uint8_t*)d_wts;
        E.cur = &tabs[cur]; E.next = &tabs[cur ^ 1]; E.status = d_est;
        kc_launch_zstd_dstream_entropy(E, dev->stream);
        KcZsExecParams X;
        memset(&X, 0, sizeof(X));
        X.in = E.in; X.blocks = E.blocks; X.n_blocks = count; X.window = window; X.lits = E.lits; X.seqs = E.seqs; X.estatus = d_est;
        X.hist = (uint8_t*)hist[sel]; X.hist_pos = kept; X.hist_cap = hist_cap[sel];
        X.dict = dict_live ? (const uint8_t*)d_dict : nullptr;
        X.dict_len = dict_live ? o.dicts[dict - 1].content_len : 0;
        X.def_mask = def_mask; X.cur = E.cur; X.next = E.next; X.out_size = d_osz; X.status = d_xst; X.result = d_result;
        kc_launch_zstd_dstream_execute(X, dev->stream);
        const bool hashing = checksum && !o.ignore_checksum;
        if (hashing) {
            KcZsHashParams Hh;
            memset(&Hh, 0, sizeof(Hh));
            Hh.hist = X.hist; Hh.start = kept; Hh.result = d_result; Hh.h = (KcZsHash*)d_hash; Hh.final = has_last ? 1 : 0;
            kc_launch_xxh64_stream(Hh, dev->stream);
        }
        stat.assign((size_t)count * 2, 0);
        if ((s = dev->d2h(result, d_result, 16)) || (s = dev->d2h(stat.data(), d_xst, (size_t)count * 8))) return s;
        if (hashing && has_last && (s = dev->d2h(&digest, &((KcZsHash*)d_hash)->digest, 8))) return s;
        if ((s = dev->sync())) return s;
        // ---- what stands: the blocks in front of the first failure, held to the frame's content size ----
        uint32_t ok = (uint32_t)result[1];
        if (ok > count) ok = count;
        uint32_t verdict = ok < count ? stat[ok] : 0;
        if (ok < count && verdict == 0) verdict = KCZD_CORRUPT;
        uint64_t give = 0;
        for (uint32_t i = 0; i < ok; i++) {
            const uint64_t sz = stat[(size_t)count + i];
            if (fcs != KC_ZD_NO_SIZE && decoded + sz > fcs) { verdict = KCZD_CORRUPT; break; }                    // ErrFrameSizeExceeded
            if (has_last && i + 1 == count && fcs != KC_ZD_NO_SIZE && decoded + sz != fcs) { verdict = KCZD_CORRUPT; break; }  // ErrFrameSizeMismatch
            decoded += sz;
            give += sz;
        }
        if (give > need) return KC_ERR_INTERNAL;  // (the kernels hold every block to its bound)
        if (give) {
            if ((s = dev->d2h(dst, (const uint8_t*)hist[sel] + kept, (size_t)give)) || (s = dev->sync())) return s;
        }
        *produced = give;
        *cls = verdict;
        kept += give;
        cur ^= 1;
        return KC_OK;
    }

    // kc_zstd_dstream_feed
    int feed(const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed, uint64_t* produced, uint32_t* status) {
        uint64_t c = 0, p = 0;
        *consumed = 0; *produced = 0; *status = 0;
        if (state == FAILED) { *status = fail; return KC_OK; }
        int rc = KC_OK;
        for (;;) {
            const uint64_t avail = n - c;
            if (state == DONE || state == FAILED) break;
            if (state == BETWEEN) {
                if (avail == 0) { if (eof) state = DONE; break; }  // nothing more: a clean end (decoder.go:493, framedec.go reset on io.EOF)
                if (avail < 4) { if (eof) set_fail(KCZD_EOF, status); break; }
                const uint8_t* q = src + c;
                const uint32_t magic = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {  // skippable frame: its payload is counted down, never buffered
                    if (avail < 8) { if (eof) set_fail(KCZD_EOF, status); break; }
                    skip_left = (uint64_t)q[4] | ((uint64_t)q[5] << 8) | ((uint64_t)q[6] << 16) | ((uint64_t)q[7] << 24);
                    c += 8;
                    state = SKIP;
                    continue;
                }
                if (magic != 0xFD2FB528u) { set_fail(KCZD_MAGIC, status); break; }
                uint32_t cls = 0;
                const int h = frame_header(q + 4, avail - 4, &cls);
                if (h < 0) { set_fail(cls, status); break; }
                if (h == 0) { if (eof) set_fail(KCZD_EOF, status); break; }
                c += 4 + (uint64_t)h;
                state = BLOCKS;
                continue;
            }
            if (state == SKIP) {
                const uint64_t take = skip_left < avail ? skip_left : avail;
                c += take;
                skip_left -= take;
                if (skip_left == 0) { state = BETWEEN; continue; }
                if (eof) set_fail(KCZD_EOF, status);
                break;
            }
            if (state == CHECKSUM) {
                if (avail < 4) { if (eof) set_fail(KCZD_EOF, status); break; }
                const uint8_t* q = src + c;
                const uint32_t stored = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                c += 4;
                if (!o.ignore_checksum && stored != (uint32_t)digest) { set_fail(KCZD_CRC, status); break; }
                state = BETWEEN;
                continue;
            }
            // ---- BLOCKS: as many whole blocks as fit dst by their bound, at most the launch limit ----
            const uint64_t blockMax = window < (128u << 10) ? window : (uint64_t)(128u << 10);
            const uint64_t room = dst_cap - p;
            recs.clear();
            uint64_t at = c, need = 0;
            uint32_t pending = 0;
            bool more = false, has_last = false;
            while (recs.size() < o.blocks) {
                if (n - at < 3) { more = true; break; }
                const uint32_t bh = (uint32_t)src[at] | ((uint32_t)src[at + 1] << 8) | ((uint32_t)src[at + 2] << 16);
                const uint32_t type = (bh >> 1) & 3u, size = bh >> 3;
                if (type == 3) { pending = KCZD_CORRUPT; break; }
                uint64_t bound, have = size;
                if (type == 2) {
                    if (size > (128u << 10) || (uint64_t)size > window || size < 2) { pending = KCZD_CORRUPT; break; }
                    bound = blockMax;
                } else {
                    if (size > (128u << 10) || (uint64_t)size > window) { pending = KCZD_WINDOW; break; }
                    bound = size;
                    if (type == 1) have = 1;
                }
                if (n - at - 3 < have) { more = true; break; }
                if (bound > dst_cap) { rc = KC_ERR_DST_TOO_SMALL; break; }
                if (need + bound > room) break;  // (dst is full: the caller drains it)
                KcZsBlock R;
                memset(&R, 0, sizeof(R));
                R.pos = at + 3 - c; R.size = size; R.type = type;
                if (type == 2) walk_compressed(src + at + 3, R);
                recs.push_back(R);
                need += bound;
                at += 3 + have;
                if (bh & 1u) { has_last = true; break; }
            }
            if (recs.empty()) {
                if (rc != KC_OK) break;
                if (pending) set_fail(pending, status);
                else if (more && eof) set_fail(KCZD_EOF, status);
                break;  // (more input, or room in dst, is the caller's to bring)
            }
            rc = KC_OK;  // (a block too large for dst behind blocks that fit: the next call says so)
            uint64_t got = 0;
            uint32_t cls = 0;
            const int s = launch(src + c, at - c, need, has_last, dst + p, &got, &cls);
            if (s != KC_OK) { rc = s; state = FAILED; fail = KCZD_CORRUPT; break; }
            p += got;
            c = at;
            if (cls) { set_fail(cls, status); break; }
            if (has_last) state = checksum ? CHECKSUM : BETWEEN;
        }
        *consumed = c;
        *produced = p;
        return rc;
    }
};
