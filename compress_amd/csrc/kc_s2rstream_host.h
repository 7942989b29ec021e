#pragma once
// kc_s2rstream_host.h — host logic of the S2 stream reader that needs no device of its own: the state machine behind
// kc_s2_rstream_feed / _skip / _on_skippable (kc_s2_rstream_api.cpp; the wave emulator's wrapper tools/hipemu/kcemu.cpp runs the same
// machine over plain memory).  It follows the reference's sequential Reader: Read (s2/reader.go:249-405), readFull (:190-198),
// skippable and its callbacks (:200-246, ReaderSkippableCB :109), Skip (:674-842), Reset (:177).
//
// The chunk-header rules are kc_s2_walk_from's (kc_s2_plan_dev.h), in its partial form: the walk stops in front of the first chunk
// that is not whole instead of calling it corrupt, hands every skippable chunk over, and says where and in which reader state it
// stopped.  One window: the walk over what the caller holds, the bytes from the first body to decode to the end of the last one to
// the device, one launch of one wave per chunk (kc_s2_rstream.hip), the verdicts back, then the deliverable prefix straight from the
// device window to the caller's dst.  Windows follow each other synchronously.
//
// Skip: a data chunk that lies wholly inside the pending skip is passed by its header (and, for a compressed chunk, the uvarint);
// its body is counted down like a skippable chunk's payload — never staged, decoded or CRC-checked.  The chunk that holds the
// skip's end is decoded and checked whole; only its bytes behind the skip go to dst.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/kcgpu.h"
#include "kc_decdev_host.h"
#include "kc_s2_plan_dev.h"

// The stream's buffers on its device (kc_decdev_host.h).
enum { RS_IN, RS_RECS, RS_STAT, RS_OUT, RS_N };

struct KcS2rOpts {
    uint32_t max_block = 4u << 20;
    uint32_t max_buf = 0;     // MaxEncodedLen(max_block) + 4 (Reader.maxBufSize, s2/reader.go:42)
    int ignore_crc = 0, ignore_id = 0;
    uint32_t chunks = 4096;   // data chunks per launch (KC_OPT_S2_RSTREAM_CHUNKS)
};

struct KcS2rStream {
    enum { WALK, PAYLOAD, FAILED, DONE };
    KcDecDevice* dev = nullptr;
    KcS2rOpts o;
    int state = WALK;
    uint32_t fail = 0;
    int dev_fail = 0;                         // the kc_status of a copy or launch that failed: every later feed returns it
    bool readHeader = false, snappy = false;  // Reader.readHeader / Reader.snappyFrame at the first byte not yet consumed
    uint64_t skip_left = 0;                   // decoded bytes still to pass (Skip)
    uint64_t left = 0;                        // PAYLOAD: bytes of the current chunk still to count down
    uint32_t pay_id = 0;                      // PAYLOAD: the chunk's type when a callback takes its pieces, else 0
    kc_s2_skippable_fn cb[0x7e] = {nullptr};  // ids 0x80 .. 0xfd
    void* cb_user[0x7e] = {nullptr};
    // sources of copies in flight
    std::vector<KcS2WChunk> recs;
    std::vector<uint32_t> stat;

    void start() { readHeader = o.ignore_id != 0; snappy = false; }
    void reset() {  // Reader.Reset (:177): options and callbacks stay
        state = WALK; fail = 0; dev_fail = 0; skip_left = 0; left = 0; pay_id = 0;
        start();
    }
    int on_skippable(uint8_t id, kc_s2_skippable_fn fn, void* user) {  // ReaderSkippableCB (:109): 0x80 <= id <= 0xfd
        if (id < 0x80u || id > 0xfdu) return KC_ERR_BAD_ARG;
        cb[id - 0x80u] = fn;
        cb_user[id - 0x80u] = fn ? user : nullptr;
        return KC_OK;
    }
    void set_fail(uint32_t cls, uint32_t* status) { state = FAILED; fail = cls; *status = cls; }

    // One window: recs[0 .. count) whose bodies lie in in[0 .. in_len); `lo` bytes at the front of the first chunk belong to the skip.
    // The bytes of the chunks in front of the first failing one, less lo, go to dst.  Returns a kc_status; *cls = the failing chunk's
    // class.
    int launch(const uint8_t* in, uint64_t in_len, uint64_t out_len, uint64_t lo, uint8_t* dst, uint64_t* produced, uint32_t* cls) {
        const uint32_t count = (uint32_t)recs.size();
        void *d_in, *d_recs, *d_stat, *d_out;
        int s;
        *cls = 0;
        *produced = 0;
        if ((s = dev->reserve(RS_IN, (size_t)in_len, &d_in)) || (s = dev->reserve(RS_RECS, (size_t)count * sizeof(KcS2WChunk), &d_recs)) ||
            (s = dev->reserve(RS_STAT, (size_t)count * 4, &d_stat)) || (s = dev->reserve(RS_OUT, (size_t)out_len, &d_out)))  // (the kernel bounds every access exactly: no slack)
            return s;
        if ((s = dev->h2d(d_in, in, (size_t)in_len)) || (s = dev->h2d(d_recs, recs.data(), (size_t)count * sizeof(KcS2WChunk)))) return s;
        KcS2RstreamParams P;
        memset(&P, 0, sizeof(P));
        P.in = (const uint8_t*)d_in; P.in_len = in_len; P.chunks = (const KcS2WChunk*)d_recs; P.n_chunks = count; P.out = (uint8_t*)d_out;
        P.out_len = out_len; P.ignore_crc = o.ignore_crc; P.status = (uint32_t*)d_stat;
        kc_launch_s2_rstream(P, dev->stream);
        stat.assign(count, 0);
        if ((s = dev->d2h(stat.data(), d_stat, (size_t)count * 4)) || (s = dev->sync())) return s;
        uint64_t good = 0;  // decoded bytes in front of the first failing chunk
        for (uint32_t i = 0; i < count; i++) {
            if (stat[i]) { *cls = stat[i]; break; }
            good += recs[i].dlen;
        }
        if (good > out_len) return KC_ERR_INTERNAL;
        const uint64_t give = good > lo ? good - lo : 0;
        if (give) {
            if ((s = dev->d2h(dst, (const uint8_t*)d_out + lo, (size_t)give)) || (s = dev->sync())) return s;
        }
        *produced = give;
        return KC_OK;
    }

    // kc_s2_rstream_feed
    int feed(const uint8_t* src, uint64_t n, int eof, uint8_t* dst, uint64_t dst_cap, uint64_t* consumed, uint64_t* produced, uint32_t* status) {
        uint64_t c = 0, p = 0;
        *consumed = 0; *produced = 0; *status = 0;
        if (state == FAILED) {
            if (dev_fail) return dev_fail;  // the device failed, not the stream: no class is claimed for the input
            *status = fail;
            return KC_OK;
        }
        int rc = KC_OK;
        for (;;) {
            const uint64_t avail = n - c;
            if (state == DONE || state == FAILED) break;
            if (state == PAYLOAD) {  // a skippable chunk's payload, or the body of a data chunk inside the skip: counted down, never buffered
                const uint64_t take = left < avail ? left : avail;
                if (pay_id && take && cb[pay_id - 0x80u]) {  // (a callback removed while its chunk is in flight: a plain countdown)
                    if (cb[pay_id - 0x80u](cb_user[pay_id - 0x80u], (uint8_t)pay_id, src + c, take, left - take) != 0) {
                        c += take;
                        set_fail(KCS2D_CALLBACK, status);
                        break;
                    }
                }
                c += take;
                left -= take;
                if (left == 0) { state = WALK; pay_id = 0; continue; }
                if (eof) set_fail(KCS2D_CORRUPT, status);  // readFull (:190-198): the input ended inside a chunk
                break;
            }
            // ---- WALK ----
            if (avail == 0) {
                if (eof) {
                    if (skip_left) set_fail(KCS2D_UNEXPECTED_EOF, status);  // Skip at the input's end (:700-705)
                    else state = DONE;                                       // io.EOF from the 4-byte read: the clean end (:259-261)
                }
                break;
            }
            const uint64_t room = dst_cap - p, c0 = c;
            const bool rh0 = readHeader, sn0 = snappy;
            const uint64_t skip0 = skip_left;
            recs.clear();
            uint64_t need = 0, lo = 0, first_body = 0, over_at = 0, over_give = 0;
            bool over = false;
            auto more = [&](uint64_t) { return !over && recs.size() < o.chunks; };
            auto emit = [&](uint32_t, uint64_t body_off, uint32_t body_len, uint32_t kind, uint64_t, uint32_t dlen, uint32_t crc) {
                if (over) return;
                if (recs.empty() && skip_left > 0 && (uint64_t)dlen <= skip_left) {  // wholly inside the skip: passed by its header
                    skip_left -= dlen;
                    return;
                }
                const uint64_t cut = recs.empty() ? skip_left : 0;
                const uint64_t give = (uint64_t)dlen - cut;
                if (give > room - (need - lo)) {  // dst is full: the caller drains it
                    over = true; over_at = body_off - 8; over_give = give;
                    return;
                }
                if (recs.empty()) { lo = cut; skip_left = 0; first_body = body_off; }
                KcS2WChunk R;
                R.body_off = body_off - first_body; R.out_off = need; R.body_len = body_len; R.dlen = dlen; R.crc = crc; R.kind = kind;
                recs.push_back(R);
                need += dlen;
            };
            const KcS2Walk W = kc_s2_walk_from<true>(src, c, n, o.max_block, o.max_buf, readHeader, snappy, more, emit);
            const uint64_t at = over ? over_at : W.pos;
            readHeader = W.readHeader != 0; snappy = W.snappy != 0;  // (a data chunk changes neither: also right at over_at)
            if (!recs.empty()) {
                const KcS2WChunk& L = recs.back();
                uint64_t got = 0;
                uint32_t cls = 0;
                const int s = launch(src + first_body, L.body_off + L.body_len, need, lo, dst + p, &got, &cls);
                if (s != KC_OK) { rc = s; state = FAILED; dev_fail = s; break; }
                p += got;
                c = at;
                if (cls) { set_fail(cls, status); break; }
                continue;  // (what ended the walk is found again from here)
            }
            if (over) {
                if (p == 0 && over_give > dst_cap) {  // the next chunk to hand out can never fit: nothing of this walk is consumed
                    readHeader = rh0; snappy = sn0; skip_left = skip0;
                    // the refusal promises that nothing was consumed: a call that already counted a payload down reports that
                    // progress with KC_OK, and the next call, which starts here, refuses
                    if (c0 == 0) rc = KC_ERR_DST_TOO_SMALL;
                    break;
                }
                c = at;
                break;
            }
            c = at;
            if (W.status) { set_fail(W.status, status); break; }
            if (W.stopped == KC_S2W_SHORT) {  // more input is the caller's to bring
                if (eof) set_fail(KCS2D_CORRUPT, status);
                break;
            }
            if (W.stopped == KC_S2W_SHORT_DATA) {  // header (and uvarint) of a data chunk whose body is not whole
                if (skip_left > 0 && (uint64_t)W.dlen <= skip_left) {
                    skip_left -= W.dlen;
                    c += 4;
                    state = PAYLOAD; left = W.chunkLen; pay_id = 0;
                    continue;
                }
                if (eof) set_fail(KCS2D_CORRUPT, status);
                break;
            }
            if (W.stopped == KC_S2W_SKIPPABLE) {  // padding, index and other skippable chunks: the walk stands at the header
                const uint32_t id = W.type;
                const bool has_cb = id <= 0xfdu && cb[id - 0x80u] != nullptr;
                if (has_cb && p > 0) break;  // its callback runs once the bytes in front of it have been returned
                c += 4;
                state = PAYLOAD; left = W.chunkLen; pay_id = has_cb ? id : 0;
                if (has_cb && W.chunkLen == 0 && cb[id - 0x80u](cb_user[id - 0x80u], (uint8_t)id, src + c, 0, 0) != 0) { set_fail(KCS2D_CALLBACK, status); break; }
                continue;
            }
            // the walk reached the end of what the caller holds, at a chunk boundary
        }
        *consumed = c;
        *produced = p;
        return rc;
    }
};
