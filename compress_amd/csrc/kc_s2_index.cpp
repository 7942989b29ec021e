// kc_s2_index.cpp — s2.Index on the host: Load, LoadStream, Find (s2/index.go:97-127, 238-413), the writer side add / reduce /
// appendTo (:57-87, 130-234) and IndexStream (:420-516).  Plain C++ with no device code.  The index bytes are untrusted: every read
// goes through a cursor that knows the buffer's end.
#include <string.h>
#include <new>
#include "../../include/kcgpu.h"
#include "kc_s2_index.h"

namespace {

const uint8_t kHeader[6] = {'s', '2', 'i', 'd', 'x', 0};   // S2IndexHeader
const uint8_t kTrailer[6] = {0, 'x', 'd', 'i', '2', 's'};  // S2IndexTrailer
const int64_t kMaxIndexEntries = 1 << 16, kMinIndexDist = 1 << 20;
const uint64_t kMaxChunkSize = 0xFFFFFF, kMaxBlockSize = 4u << 20;

struct Cur {  // b = b[n:] with its bounds
    const uint8_t* p;
    uint64_t left;
};

// binary.Varint (encoding/binary/varint.go:129-166): n > 0 bytes read; 0: buffer too small; < 0: overflow
int varint(const Cur& c, int64_t* v) {
    uint64_t x = 0;
    uint32_t s = 0;
    for (uint64_t i = 0; i < c.left; i++) {
        const uint8_t b = c.p[i];
        if (i == 10) return -(int)(i + 1);  // MaxVarintLen64: overflow
        if (b < 0x80) {
            if (i == 9 && b > 1) return -(int)(i + 1);
            x |= (uint64_t)b << s;
            int64_t r = (int64_t)(x >> 1);
            if (x & 1) r = ~r;
            *v = r;
            return (int)(i + 1);
        }
        x |= (uint64_t)(b & 0x7f) << s;
        s += 7;
    }
    return 0;
}

void put_varint(std::vector<uint8_t>& b, int64_t x) {  // binary.PutVarint
    uint64_t ux = (uint64_t)x << 1;
    if (x < 0) ux = ~ux;
    while (ux >= 0x80) { b.push_back((uint8_t)ux | 0x80); ux >>= 7; }
    b.push_back((uint8_t)ux);
}

// wrapping int64 arithmetic, as Go's (the offsets of a hostile index may overflow; the checks behind them decide)
int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

int load(kc_s2_index* i, const uint8_t* b0, uint64_t n, uint64_t* consumed) {
    Cur b{b0, n};
    auto ret = [&](int code) { if (consumed) *consumed = n - b.left; return code; };
    auto adv = [&](uint64_t k) { b.p += k; b.left -= k; };
    if (b.left <= 4 + 6 + 6) return ret(KC_S2I_UNEXPECTED_EOF);      // :239
    if (b.p[0] != 0x99) return ret(KC_S2I_CORRUPT);                  // :242 ChunkTypeIndex
    const uint64_t chunkLen = (uint64_t)b.p[1] | (uint64_t)b.p[2] << 8 | (uint64_t)b.p[3] << 16;
    adv(4);
    if (b.left < chunkLen) return ret(KC_S2I_UNEXPECTED_EOF);        // :249
    if (memcmp(b.p, kHeader, 6) != 0) return ret(KC_S2I_UNSUPPORTED);  // :252 (more than 6 bytes are left: :239)
    adv(6);
    int64_t v = 0;
    int k;
    if ((k = varint(b, &v)) <= 0 || v < 0) return ret(KC_S2I_CORRUPT);  // :258 total uncompressed
    i->total_uncompressed = v;
    adv((uint64_t)k);
    if ((k = varint(b, &v)) <= 0) return ret(KC_S2I_CORRUPT);        // :266 total compressed
    i->total_compressed = v;
    adv((uint64_t)k);
    if ((k = varint(b, &v)) <= 0) return ret(KC_S2I_CORRUPT);        // :274 estBlockUncomp
    if (v < 0) return ret(KC_S2I_CORRUPT);                           // :277
    i->est_block_uncomp = v;
    adv((uint64_t)k);
    if ((k = varint(b, &v)) <= 0) return ret(KC_S2I_CORRUPT);        // :285 entries
    if (v < 0 || v > kMaxIndexEntries) return ret(KC_S2I_CORRUPT);   // :288
    const size_t entries = (size_t)v;
    adv((uint64_t)k);
    i->c_off.resize(entries);
    i->u_off.resize(entries);
    if (b.left < 1) return ret(KC_S2I_UNEXPECTED_EOF);               // :299
    const uint8_t hasUncompressed = b.p[0];
    adv(1);
    if ((hasUncompressed & 1) != hasUncompressed) return ret(KC_S2I_CORRUPT);  // :304
    for (size_t idx = 0; idx < entries; idx++) {
        int64_t uOff = 0;
        if (hasUncompressed != 0) {
            if ((k = varint(b, &v)) <= 0) return ret(KC_S2I_CORRUPT);  // :313
            uOff = v;
            adv((uint64_t)k);
        }
        if (idx > 0) {
            const int64_t prev = i->u_off[idx - 1];
            uOff = wadd(uOff, wadd(prev, i->est_block_uncomp));
            if (uOff <= prev) return ret(KC_S2I_CORRUPT);            // :324
        }
        if (uOff < 0) return ret(KC_S2I_CORRUPT);                    // :328
        i->u_off[idx] = uOff;
    }
    int64_t cPredict = i->est_block_uncomp / 2;
    for (size_t idx = 0; idx < entries; idx++) {
        int64_t cOff = 0;
        if ((k = varint(b, &v)) <= 0) return ret(KC_S2I_CORRUPT);    // :340
        cOff = v;
        adv((uint64_t)k);
        if (idx > 0) {
            const int64_t cPredictNew = wadd(cPredict, cOff / 2);
            const int64_t prev = i->c_off[idx - 1];
            cOff = wadd(cOff, wadd(prev, cPredict));
            if (cOff <= prev) return ret(KC_S2I_CORRUPT);            // :353
            cPredict = cPredictNew;
        }
        if (cOff < 0) return ret(KC_S2I_CORRUPT);                    // :358
        i->c_off[idx] = cOff;
    }
    if (b.left < 4 + 6) return ret(KC_S2I_UNEXPECTED_EOF);           // :363
    adv(4);
    if (memcmp(b.p, kTrailer, 6) != 0) return ret(KC_S2I_CORRUPT);   // :370
    adv(6);
    return ret(KC_S2I_OK);
}

// ---- the writer side, for IndexStream: add (:57-87), reduce (:130-152), appendTo (:154-234) ----
struct Builder {
    int64_t total_u = 0, total_c = 0, est = 0;  // (a zero Index: IndexStream starts from `var i Index`)
    std::vector<int64_t> c, u;

    bool add(int64_t comp, int64_t unc) {
        if (!u.empty()) {
            const size_t last = u.size() - 1;
            if (u[last] == unc) { c[last] = comp; return true; }
            if (u[last] > unc || c[last] > comp) return false;
            if (u[last] + kMinIndexDist > unc) return true;
        }
        c.push_back(comp);
        u.push_back(unc);
        return true;
    }
    void reduce() {
        if ((int64_t)u.size() < kMaxIndexEntries && est >= kMinIndexDist) return;
        int64_t removeN = ((int64_t)u.size() + 1) / kMaxIndexEntries;
        while (est * (removeN + 1) < kMinIndexDist && (int64_t)u.size() / (removeN + 1) > 1000) removeN++;
        size_t j = 0;
        for (size_t idx = 0; idx < u.size(); idx += (size_t)removeN + 1, j++) { c[j] = c[idx]; u[j] = u[idx]; }
        c.resize(j);
        u.resize(j);
        est += est * removeN;
    }
    std::vector<uint8_t> append_to(int64_t uncompTotal, int64_t compTotal) {
        reduce();
        std::vector<uint8_t> b = {0x99, 0, 0, 0};
        b.insert(b.end(), kHeader, kHeader + 6);
        put_varint(b, uncompTotal);
        put_varint(b, compTotal);
        put_varint(b, est);
        put_varint(b, (int64_t)u.size());
        uint8_t hasUncompressed = 0;
        for (size_t idx = 0; idx < u.size(); idx++) {
            if (idx == 0 ? u[0] != 0 : u[idx] != u[idx - 1] + est) { hasUncompressed = 1; break; }
        }
        b.push_back(hasUncompressed);
        if (hasUncompressed)
            for (size_t idx = 0; idx < u.size(); idx++) put_varint(b, idx ? u[idx] - (u[idx - 1] + est) : u[idx]);
        int64_t cPredict = est / 2;
        for (size_t idx = 0; idx < c.size(); idx++) {
            int64_t cOff = c[idx];
            if (idx > 0) {
                cOff -= c[idx - 1] + cPredict;
                cPredict += cOff / 2;
            }
            put_varint(b, cOff);
        }
        const uint32_t sz = (uint32_t)(b.size() + 4 + 6);
        for (int k = 0; k < 4; k++) b.push_back((uint8_t)(sz >> (8 * k)));
        b.insert(b.end(), kTrailer, kTrailer + 6);
        const size_t chunkLen = b.size() - 4;
        b[1] = (uint8_t)chunkLen; b[2] = (uint8_t)(chunkLen >> 8); b[3] = (uint8_t)(chunkLen >> 16);
        return b;
    }
};

// IndexStream's loop (:424-515): KC_S2I_OK with the index in `out`, or the class of its error
uint32_t index_stream(const uint8_t* src, uint64_t n, std::vector<uint8_t>& out) {
    Builder i;
    bool readHeader = false;
    uint64_t pos = 0;
    for (;;) {
        if (pos == n) { out = i.append_to(i.total_u, i.total_c); return KC_S2I_OK; }  // io.EOF from the 4-byte read
        if (n - pos < 4) return KC_S2I_UNEXPECTED_EOF;                // io.ReadFull's own error, returned as it is (:430)
        const int64_t startChunk = i.total_c;
        i.total_c += 4;
        const uint8_t chunkType = src[pos];
        if (!readHeader) {
            if (chunkType != 0xff) return KC_S2I_CORRUPT;             // :439
            readHeader = true;
        }
        const uint64_t chunkLen = (uint64_t)src[pos + 1] | (uint64_t)src[pos + 2] << 8 | (uint64_t)src[pos + 3] << 16;
        pos += 4;
        if (chunkLen < 4) return KC_S2I_CORRUPT;                      // :444, for every chunk type
        i.total_c += (int64_t)chunkLen;
        if (n - pos < chunkLen) return KC_S2I_UNEXPECTED_EOF;         // :451
        const uint8_t* buf = src + pos;
        pos += chunkLen;
        if (chunkType == 0x00) {
            // DecodedLen(buf[4:]) (s2/decode.go:29-47): a uvarint of at most 5 bytes... binary.Uvarint reads up to 10; n <= 0 or a value
            // above 32 bits is ErrCorrupt
            uint64_t v = 0;
            bool ok = false;
            for (uint64_t k = 0; k < 10 && 4 + k < chunkLen; k++) {
                const uint8_t b = buf[4 + k];
                if (k == 9 && b > 1) break;
                v |= (uint64_t)(b & 0x7f) << (7 * k);
                if (b < 0x80) { ok = true; break; }
            }
            if (!ok || v > 0xffffffffull) return KC_S2I_CORRUPT;      // :460
            if (v > kMaxBlockSize) return KC_S2I_CORRUPT;             // :463
            if (i.est == 0) i.est = (int64_t)v;
            if (!i.add(startChunk, i.total_u)) return KC_S2I_CORRUPT;  // (an internal error of add: cannot happen on ascending totals)
            i.total_u += (int64_t)v;
            continue;
        }
        if (chunkType == 0x01) {
            const uint64_t n2 = chunkLen - 4;
            if (n2 > kMaxBlockSize) return KC_S2I_CORRUPT;            // :478
            if (i.est == 0) i.est = (int64_t)n2;
            if (!i.add(startChunk, i.total_u)) return KC_S2I_CORRUPT;
            i.total_u += (int64_t)n2;
            continue;
        }
        if (chunkType == 0xff) {
            if (chunkLen != 6) return KC_S2I_CORRUPT;                 // :493
            if (memcmp(buf, "S2sTwO", 6) != 0 && memcmp(buf, "sNaPpY", 6) != 0) return KC_S2I_CORRUPT;  // :499
            continue;
        }
        if (chunkType <= 0x7f) return KC_S2I_UNSUPPORTED;             // :508
        if (chunkLen > kMaxChunkSize) return KC_S2I_UNSUPPORTED;      // :511 (a 24-bit length never is)
    }
}

}  // namespace

extern "C" {

kc_s2_index* kc_s2_index_new(void) { return new (std::nothrow) kc_s2_index(); }
void kc_s2_index_free(kc_s2_index* ix) { delete ix; }

int kc_s2_index_load(kc_s2_index* ix, const uint8_t* b, uint64_t n, uint64_t* consumed) {
    if (consumed) *consumed = 0;
    if (!ix || (n && !b)) return KC_S2I_CORRUPT;
    try { return load(ix, b, n, consumed); } catch (...) { return KC_S2I_CORRUPT; }
}

int kc_s2_index_load_stream(kc_s2_index* ix, const uint8_t* stream, uint64_t n) {
    if (!ix || (n && !stream)) return KC_S2I_CORRUPT;
    if (n < 10) return KC_S2I_UNEXPECTED_EOF;                         // rs.Seek(-10, io.SeekEnd) fails (:383)
    const uint8_t* tmp = stream + n - 10;
    if (memcmp(tmp + 4, kTrailer, 6) != 0) return KC_S2I_UNSUPPORTED;  // :393
    const uint64_t sz = (uint64_t)tmp[0] | (uint64_t)tmp[1] << 8 | (uint64_t)tmp[2] << 16 | (uint64_t)tmp[3] << 24;
    if (sz > kMaxChunkSize + 4) return KC_S2I_CORRUPT;                // :397
    if (sz > n) return KC_S2I_UNEXPECTED_EOF;                         // rs.Seek(-sz, io.SeekEnd) fails (:400)
    try { return load(ix, stream + n - sz, sz, nullptr); } catch (...) { return KC_S2I_CORRUPT; }
}

int kc_s2_index_find(const kc_s2_index* ix, int64_t offset, int64_t* c_off, int64_t* u_off) {
    if (c_off) *c_off = 0;
    if (u_off) *u_off = 0;
    if (!ix || !c_off || !u_off) return KC_S2I_CORRUPT;
    if (ix->total_uncompressed < 0) return KC_S2I_CORRUPT;            // :98
    if (offset < 0) {
        offset = ix->total_uncompressed + offset;
        if (offset < 0) return KC_S2I_UNEXPECTED_EOF;                 // :104
    }
    if (offset > ix->total_uncompressed) return KC_S2I_UNEXPECTED_EOF;  // :108
    // the last entry whose uncompressed offset is <= offset, else (0, 0) — or the first entry when there are more than 200 (:110-118)
    size_t lo = 0, hi = ix->u_off.size();
    while (lo < hi) {  // sort.Search: the first entry with u > offset
        const size_t mid = lo + (hi - lo) / 2;
        if (ix->u_off[mid] > offset) hi = mid; else lo = mid + 1;
    }
    if (lo == 0 && ix->u_off.size() > 200) lo = 1;
    if (lo > 0) { *c_off = ix->c_off[lo - 1]; *u_off = ix->u_off[lo - 1]; }
    return KC_S2I_OK;
}

int64_t kc_s2_index_total_uncompressed(const kc_s2_index* ix) { return ix ? ix->total_uncompressed : -1; }
int64_t kc_s2_index_total_compressed(const kc_s2_index* ix) { return ix ? ix->total_compressed : -1; }
int64_t kc_s2_index_est_block_uncompressed(const kc_s2_index* ix) { return ix ? ix->est_block_uncomp : 0; }

uint32_t kc_s2_index_entries(const kc_s2_index* ix, int64_t* c_off, int64_t* u_off, uint32_t cap) {
    if (!ix) return 0;
    const uint32_t n = (uint32_t)ix->u_off.size();
    for (uint32_t k = 0; k < n && k < cap; k++) {
        if (c_off) c_off[k] = ix->c_off[k];
        if (u_off) u_off[k] = ix->u_off[k];
    }
    return n;
}

kc_status kc_s2_index_stream(const uint8_t* src, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t* status) {
    if (!out_len || !status || (n && !src) || (cap && !out)) return KC_ERR_BAD_ARG;
    *out_len = 0;
    try {
        std::vector<uint8_t> b;
        *status = index_stream(src, n, b);
        if (*status) return KC_OK;
        *out_len = b.size();
        if (b.size() > cap) return KC_ERR_DST_TOO_SMALL;
        memcpy(out, b.data(), b.size());
        return KC_OK;
    } catch (...) { return KC_ERR_INTERNAL; }
}

}  // extern "C"
