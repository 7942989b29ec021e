// kc_s2_dec_dev.h — the decoder of one S2 / Snappy data chunk by one wave, shared by the whole-input kernel (kc_s2_decode_all.hip)
// and the ranged one (kc_s2_ranges.hip): the tag-stream decoder, its literal and copy helpers and the CRC tail.
//
// Semantics: s2Decode (s2/decode_other.go:22-290) — literals in all five length forms, copy1 / copy2 / copy4, the repeat forms with
// their extended lengths, `offset <= 0 || d < offset || length > len(dst) - d`, both literal bounds, `d != dLen` at the end.  The
// input is untrusted: every read is checked against the chunk's end and every write against the dLen bytes at dst, and all checks
// of an operation come before any of its writes.
#pragma once
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_s2_dev.h"

struct __attribute__((packed)) s2d_u128u { uint32_t x, y, z, w; };
__device__ __forceinline__ void s2d_st128u(uint8_t* p, uint4 v) {  // unaligned 16-byte store
    s2d_u128u t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    *(s2d_u128u*)p = t;
}

// n bytes from a to d, the two ranges disjoint; all lanes call
__device__ __forceinline__ void s2d_copy8(uint8_t* d, const uint8_t* a, uint64_t n, int lane) {
    const uint64_t body = n & ~(uint64_t)7;
    for (uint64_t k = (uint64_t)lane * 8; k < body; k += 512) st64(d + k, ld64(a + k));
    for (uint64_t k = body + (uint64_t)lane; k < n; k += 64) d[k] = a[k];
}

// slicing-by-4 tables of CRC32C (Castagnoli, reflected 0x82F63B78); all lanes call
__device__ __forceinline__ void s2d_crc_tables(uint32_t (*crcT)[256], int lane) {
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
        crcT[0][i] = c;
    }
    KC_WAVE_SYNC();
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = crcT[0][i];
        for (int t = 1; t < 4; t++) { c = crcT[0][c & 0xFF] ^ (c >> 8); crcT[t][i] = c; }
    }
    KC_WAVE_SYNC();
}

// The chunk body src[0, n) decoded to dst[0, dLen) and, with want_crc, compared with the stored masked CRC32C; all lanes call and
// all return the same KCS2D_* verdict.  crcT must hold s2d_crc_tables when want_crc.
__device__ __forceinline__ uint32_t s2d_decode_chunk(const uint8_t* src, const uint32_t n, uint8_t* dst, const uint64_t dLen, const uint32_t kind,
                                                     const bool want_crc, const uint32_t stored_crc, uint32_t (*crcT)[256], uint32_t* crcM, uint32_t* crcP,
                                                     const int lane) {
    uint32_t err = KCS2D_OK;
    uint64_t d = 0;
    if (kind & KC_S2C_STORED) {  // uncompressed chunk: a wave-wide 16-byte copy
        if ((uint64_t)n != dLen) err = KCS2D_CORRUPT;  // (the plan took dlen from the chunk length)
        else {
            const uint32_t body = n & ~15u;
            for (uint32_t k = (uint32_t)lane * 16; k < body; k += 1024) s2d_st128u(dst + k, ld128u(src + k));
            for (uint32_t k = body + (uint32_t)lane; k < n; k += 64) dst[k] = src[k];
            d = n;
        }
    } else {
        uint32_t s = 0;
        {  // the uvarint in front of the tags (s2/decode.go:36-47); the plan read the same bytes
            uint64_t v = 0;
            bool ok = false;
            for (uint32_t i = 0; i < 5 && i < n; i++) {
                const uint32_t b = uniu((uint32_t)src[i]);
                v |= (uint64_t)(b & 0x7fu) << (7 * i);
                if (b < 0x80u) { ok = true; s = i + 1; break; }
            }
            if (!ok || v != dLen) err = KCS2D_CORRUPT;
        }
        uint64_t offset = 0;
        while (!err && s < n) {
            // up to 8 bytes at the tag, the same in every lane, zero behind the chunk's end
            const uint32_t avail = n - s;
            uint64_t tv;
            if (avail >= 8) tv = ld64(src + s);
            else {
                tv = 0;
                for (uint32_t k = 0; k < avail; k++) tv |= (uint64_t)src[s + k] << (8 * k);
            }
            const uint32_t t0 = uniu((uint32_t)tv), t1 = uniu((uint32_t)(tv >> 32));
            const uint32_t tag = t0 & 0xffu;
            uint64_t length;
            if ((tag & 3u) == 0) {  // literal
                uint32_t x = tag >> 2, tl;
                if (x < 60) tl = 1;
                else if (x == 60) { tl = 2; x = (t0 >> 8) & 0xffu; }
                else if (x == 61) { tl = 3; x = (t0 >> 8) & 0xffffu; }
                else if (x == 62) { tl = 4; x = t0 >> 8; }
                else { tl = 5; x = (t0 >> 8) | (t1 << 24); }
                if (tl > avail) { err = KCS2D_CORRUPT; break; }
                s += tl;
                length = (uint64_t)x + 1;
                if (length > dLen - d || length > (uint64_t)(n - s)) { err = KCS2D_CORRUPT; break; }
                s2d_copy8(dst + d, src + s, length, lane);
                d += length;
                s += (uint32_t)length;
                continue;
            }
            if ((tag & 3u) == 1) {  // copy1 / repeat (decode_other.go:72-97, 194-230)
                if (avail < 2) { err = KCS2D_CORRUPT; break; }
                const uint32_t toffset = ((tag & 0xe0u) << 3) | ((t0 >> 8) & 0xffu);
                uint32_t l = (tag >> 2) & 7u, tl = 2;
                if (toffset == 0) {
                    if (l == 5) { tl = 3; l = ((t0 >> 16) & 0xffu) + 4; }
                    else if (l == 6) { tl = 4; l = (t0 >> 16) + (1u << 8); }
                    else if (l == 7) { tl = 5; l = ((t0 >> 16) | ((t1 & 0xffu) << 16)) + (1u << 16); }
                    if (tl > avail) { err = KCS2D_CORRUPT; break; }
                } else {
                    offset = toffset;
                }
                s += tl;
                length = (uint64_t)l + 4;
            } else if ((tag & 3u) == 2) {
                if (avail < 3) { err = KCS2D_CORRUPT; break; }
                offset = (t0 >> 8) & 0xffffu;
                length = 1 + (uint64_t)(tag >> 2);
                s += 3;
            } else {
                if (avail < 5) { err = KCS2D_CORRUPT; break; }
                offset = (uint64_t)((t0 >> 8) | (t1 << 24));
                length = 1 + (uint64_t)(tag >> 2);
                s += 5;
            }
            if (offset == 0 || d < offset || length > dLen - d) { err = KCS2D_CORRUPT; break; }
            KC_WAVE_SYNC();  // what other lanes wrote so far is read back from here on
            uint8_t* o = dst + d;
            if (offset >= length) {
                s2d_copy8(o, o - offset, length, lane);
            } else if (length <= 64) {
                if ((uint32_t)lane < (uint32_t)length) o[lane] = (o - offset)[(uint32_t)lane % (uint32_t)offset];
            } else {
                // [o - offset, o + done) is periodic with period `offset` and `done` stays a multiple of it: copying its front
                // to o + done extends it without touching its source
                uint64_t done = 0;
                while (done < length) {
                    const uint64_t have = done + offset, left = length - done;
                    const uint64_t m = left < have ? left : have;
                    s2d_copy8(o + done, o - offset, m, lane);
                    done += m;
                    KC_WAVE_SYNC();
                }
            }
            d += length;
        }
    }
    if (!err && d != dLen) err = KCS2D_CORRUPT;
    if (!err && want_crc) {
        KC_WAVE_SYNC();
        const uint8_t* r = dst;
        auto rd32 = [&](int i) -> uint32_t { return ld32(r + i); };
        auto rdb = [&](int i) -> uint32_t { return r[i]; };
        const uint32_t cc = s2_crc32c_wave(rd32, rdb, (int)dLen, crcT, crcM, crcP, lane);
        if (((cc >> 15) | (cc << 17)) + 0xa282ead8u != stored_crc) err = KCS2D_CRC;
    }
    return err;
}
