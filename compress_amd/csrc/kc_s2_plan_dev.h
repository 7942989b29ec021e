// kc_s2_plan_dev.h — the chunk walk of s2.Reader (s2/reader.go:259-404) over one input, written once for the device (one lane per
// input: kc_s2_plan.hip) and the host (the host-buffer entry points size their batches with it: kc_s2_dec_api.cpp).  It reads chunk
// headers, stream identifiers and the uvarint in front of a compressed chunk's tags; it never touches a chunk's payload.  Every read
// is checked against the input's end.
#pragma once
#include <stdint.h>
#include "kc_kernels.h"

#define KC_S2_MAX_CHUNK 0xFFFFFFu          // maxChunkSize (s2/s2.go:93)
#define KC_S2_MAX_SNAPPY_BLOCK 65536u      // maxSnappyBlockSize (s2/s2.go:99)

// decodedLen (s2/decode.go:36-47) of the block in [pos, end): a uvarint of at most 5 bytes whose value fits 32 bits
__host__ __device__ inline bool kc_s2_decoded_len(const uint8_t* in, uint64_t pos, uint64_t end, uint32_t* dlen, uint32_t* hdr) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 5; i++) {
        if (pos + i >= end) return false;  // binary.Uvarint: buffer too small
        const uint32_t b = in[pos + i];
        v |= (uint64_t)(b & 0x7fu) << (7 * i);
        if (b < 0x80u) {
            if (v > 0xffffffffull) return false;
            *dlen = (uint32_t)v;
            *hdr = i + 1;
            return true;
        }
    }
    return false;  // more than 5 bytes
}

struct KcS2Walk {
    uint32_t status;    // the first header-level error (KCS2D_*), 0: the walk reached the input's end at a chunk boundary
    uint32_t n_chunks;  // data chunks in front of it
    uint64_t total;     // their decoded bytes
    uint32_t stopped;   // kc_s2_walk_from: KC_S2W_MORE — more() ended the walk in front of the input's end; the partial form: KC_S2W_SHORT*, KC_S2W_SKIPPABLE
    // where the walk stands when it returns without an error, and the reader state there (the stream reader carries them from call to call)
    uint64_t pos;
    uint32_t readHeader, snappy;
    uint32_t type, chunkLen, dlen;  // KC_S2W_SHORT_DATA / KC_S2W_SKIPPABLE: the chunk at pos; dlen: a data chunk's decoded length
};
#define KC_S2W_MORE 1u        // more() said stop: nothing at or behind pos has been read
#define KC_S2W_SHORT 2u       // partial form: the chunk at pos is not whole and its header says nothing yet that could be acted on
#define KC_S2W_SHORT_DATA 3u  // partial form: a data chunk at pos whose body is not whole; its header checks passed and dlen is known
#define KC_S2W_SKIPPABLE 4u   // partial form: a padding, index or other skippable chunk at pos (header present), handed to the caller

// The walk from a given reader state: readHeader / snappy are Reader.readHeader / Reader.snappyFrame at `pos` (a chunk boundary).
// more(total) is asked before every chunk header is read: false ends the walk there with status 0 and W.stopped set — nothing at
// or behind `pos` has been read then (the ranged plan, kc_s2_ranges.hip).  emit(index, body_off, body_len, kind, out_rel, dlen, crc)
// is called for every data chunk in stream order.
// Partial (the stream reader, kc_s2rstream_host.h): [pos, end) is what a caller holds of a stream that may go on.  A chunk that is
// not whole is not corrupt: the walk stops in front of it (KC_S2W_SHORT; KC_S2W_SHORT_DATA when it is a data chunk whose header —
// for a compressed chunk also the uvarint — is there: every check that needs no body has then been made and W.dlen is set, which is
// all a pending Skip needs).  A skippable chunk is handed over whole or not (KC_S2W_SKIPPABLE): its payload is the caller's to count
// down.  emit is still called for whole data chunks only.
template <bool Partial = false, class More, class Emit>
__host__ __device__ inline KcS2Walk kc_s2_walk_from(const uint8_t* in, uint64_t pos, const uint64_t end, uint32_t max_block, uint32_t max_buf,
                                                    bool readHeader, bool snappy, More more, Emit emit) {
    KcS2Walk W;
    W.status = KCS2D_OK; W.n_chunks = 0; W.total = 0; W.stopped = 0; W.type = 0; W.chunkLen = 0; W.dlen = 0;
    uint64_t hpos = pos;  // (Partial: the header of the chunk in hand, where the walk steps back to)
    bool rh = readHeader;
    while (pos < end) {  // (nothing left: io.EOF from the 4-byte read, the clean end)
        if (!more(W.total)) { W.stopped = KC_S2W_MORE; break; }
        if (end - pos < 4) {
            if constexpr (Partial) W.stopped = KC_S2W_SHORT; else W.status = KCS2D_CORRUPT;
            break;
        }
        const uint32_t type = in[pos];
        const uint32_t chunkLen = (uint32_t)in[pos + 1] | ((uint32_t)in[pos + 2] << 8) | ((uint32_t)in[pos + 3] << 16);
        hpos = pos;
        rh = readHeader;
        pos += 4;
        if (!readHeader) {  // before the type switch: a leading padding chunk is corrupt too (reader.go:263-269)
            if (type != 0xffu) { W.status = KCS2D_CORRUPT; break; }
            readHeader = true;
        }
        if (type <= 0x01u) {
            if (chunkLen < 4 || chunkLen > max_buf) { W.status = KCS2D_CORRUPT; break; }
            if (end - pos < chunkLen) {
                if constexpr (Partial) {
                    uint32_t dl = chunkLen - 4, hdr = 0;
                    bool known = true;
                    if (type == 0x00u) {
                        if (end - pos < 4) known = false;
                        else if (!kc_s2_decoded_len(in, pos + 4, end, &dl, &hdr)) {
                            if (end - pos - 4 >= 5) { W.status = KCS2D_CORRUPT; break; }  // five bytes were there: not a matter of more input
                            known = false;
                        }
                    }
                    if (known && ((snappy && dl > KC_S2_MAX_SNAPPY_BLOCK) || dl > max_block)) { W.status = KCS2D_CORRUPT; break; }
                    W.stopped = known ? KC_S2W_SHORT_DATA : KC_S2W_SHORT;
                    W.type = type; W.chunkLen = chunkLen; W.dlen = dl;
                    pos = hpos; readHeader = rh;
                } else {
                    W.status = KCS2D_CORRUPT;
                }
                break;
            }
            const uint32_t crc = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16) | ((uint32_t)in[pos + 3] << 24);
            uint32_t dl = chunkLen - 4, hdr = 0;
            if (type == 0x00u && !kc_s2_decoded_len(in, pos + 4, pos + chunkLen, &dl, &hdr)) { W.status = KCS2D_CORRUPT; break; }
            if (snappy && dl > KC_S2_MAX_SNAPPY_BLOCK) { W.status = KCS2D_CORRUPT; break; }
            if (dl > max_block) { W.status = KCS2D_CORRUPT; break; }
            emit(W.n_chunks, pos + 4, chunkLen - 4, type == 0x01u ? KC_S2C_STORED : 0u, W.total, dl, crc);
            W.n_chunks++;
            W.total += dl;
            pos += chunkLen;
            continue;
        }
        if (type == 0xffu) {  // stream identifier: S2 or Snappy, also in the middle of an input (concatenated streams)
            if (chunkLen != 6) { W.status = KCS2D_CORRUPT; break; }
            if (end - pos < 6) {
                if constexpr (Partial) { W.stopped = KC_S2W_SHORT; pos = hpos; readHeader = rh; } else W.status = KCS2D_CORRUPT;
                break;
            }
            const uint8_t* m = in + pos;
            if (m[0] == 'S' && m[1] == '2' && m[2] == 's' && m[3] == 'T' && m[4] == 'w' && m[5] == 'O') snappy = false;
            else if (m[0] == 's' && m[1] == 'N' && m[2] == 'a' && m[3] == 'P' && m[4] == 'p' && m[5] == 'Y') snappy = true;
            else { W.status = KCS2D_CORRUPT; break; }
            pos += 6;
            continue;
        }
        if (type <= 0x7fu) { W.status = KCS2D_UNSUPPORTED; break; }  // reserved unskippable chunks
        if (chunkLen > KC_S2_MAX_CHUNK) { W.status = KCS2D_UNSUPPORTED; break; }
        if constexpr (Partial) {
            W.stopped = KC_S2W_SKIPPABLE; W.type = type; W.chunkLen = chunkLen;
            pos = hpos; readHeader = rh;
            break;
        }
        if (end - pos < chunkLen) { W.status = KCS2D_CORRUPT; break; }  // padding, index and other skippable chunks
        pos += chunkLen;
    }
    if constexpr (Partial) {
        if (W.status) { pos = hpos; readHeader = rh; }  // an error leaves the walk in front of the chunk that has it
    }
    W.pos = pos; W.readHeader = readHeader ? 1u : 0u; W.snappy = snappy ? 1u : 0u;
    return W;
}

// emit(index, body_off, body_len, kind, out_rel, dlen, crc) is called for every data chunk in stream order.
template <class Emit>
__host__ __device__ inline KcS2Walk kc_s2_walk(const uint8_t* in, uint64_t pos, const uint64_t end, uint32_t max_block, uint32_t max_buf, bool ignore_id,
                                               Emit emit) {
    return kc_s2_walk_from(in, pos, end, max_block, max_buf, ignore_id, false, [](uint64_t) { return true; }, emit);
}

// The reader's state behind the stream identifier at the front of the input [front, end): what a ranged read that starts in the
// middle of the input (at an index entry) starts from.  Without a valid identifier there the reader would have refused the input
// before it could seek (reader.go:263-269) unless it ignores identifiers.
__host__ __device__ inline uint32_t kc_s2_front_state(const uint8_t* in, uint64_t front, uint64_t end, bool ignore_id, bool* snappy) {
    *snappy = false;
    if (end >= front && end - front >= 10 && in[front] == 0xffu && in[front + 1] == 6 && in[front + 2] == 0 && in[front + 3] == 0) {
        const uint8_t* m = in + front + 4;
        if (m[0] == 'S' && m[1] == '2' && m[2] == 's' && m[3] == 'T' && m[4] == 'w' && m[5] == 'O') return KCS2D_OK;
        if (m[0] == 's' && m[1] == 'N' && m[2] == 'a' && m[3] == 'P' && m[4] == 'p' && m[5] == 'Y') { *snappy = true; return KCS2D_OK; }
    }
    return ignore_id ? KCS2D_OK : KCS2D_CORRUPT;
}

// One request of a ranged read: its walk.  The lane stands at `pos` (the stream's start, or the index entry Find gave) where `u`
// decoded bytes lie in front of it, and wants [off, off + len).  A chunk that ends at or before off while the reader is still
// skipping (its start lies in front of off) is passed by its header alone; every chunk from the one that holds off onwards is
// covered: cover(index, body_off, body_len, kind, a, dlen, crc) with `a` its decoded start in the stream.  The walk ends once the
// decoded position has reached off + len (for len 0: off) and reads nothing behind that point.
struct KcS2RangeWalk {
    uint32_t status;   // header-level error, KCS2D_EOF (the input ended inside the range) or KCS2D_UNEXPECTED_EOF (in front of it)
    uint32_t n_cover;  // covered chunks
    uint64_t got;      // min(len, decoded bytes available from off)
};
template <class Cover>
__host__ __device__ inline KcS2RangeWalk kc_s2_walk_range(const uint8_t* in, uint64_t pos, uint64_t end, uint32_t max_block, uint32_t max_buf,
                                                          bool readHeader, bool snappy, uint64_t u, uint64_t off, uint64_t len, Cover cover) {
    KcS2RangeWalk R;
    R.n_cover = 0;
    uint32_t n_cover = 0;
    auto more = [&](uint64_t total) { const uint64_t cur = u + total; return cur < off || cur - off < len; };
    auto emit = [&](uint32_t, uint64_t body_off, uint32_t body_len, uint32_t kind, uint64_t out_rel, uint32_t dlen, uint32_t crc) {
        const uint64_t a = u + out_rel;
        if (a < off && a + dlen <= off) return;  // Skip: "CRC is not checked on skipped blocks" (reader.go:671)
        cover(n_cover, body_off, body_len, kind, a, dlen, crc);
        n_cover++;
    };
    if (pos > end) pos = end;
    const KcS2Walk W = kc_s2_walk_from(in, pos, end, max_block, max_buf, readHeader, snappy, more, emit);
    const uint64_t cur = u + W.total;
    R.n_cover = n_cover;
    R.status = W.status;
    R.got = cur <= off ? 0 : (cur - off < len ? cur - off : len);
    if (!W.status && !W.stopped && more(W.total)) R.status = cur < off ? KCS2D_UNEXPECTED_EOF : KCS2D_EOF;  // Skip / ReadAt at the input's end
    return R;
}
