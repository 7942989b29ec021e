// kc_zdec_dev.h — device functions shared by the zstd decoders: the verifier (kc_zstd_decode.hip) and the product path
// (kc_zstd_decode_all.hip): FSE decoding cells, the backward / forward bit readers, FSE_Table_Description parsing, table
// construction, the predefined distributions and the code tables of literal lengths, match lengths and offsets.
#pragma once
#include "kc_dev.h"

namespace {

struct ZdSym { uint16_t base; uint8_t sym; uint8_t nb; };  // FSE decoding cell: newState base, symbol, bits to read

struct ZdShared {
    uint16_t huf[1 << 11];  // symbol << 8 | nBits, index = next tableLog bits
    ZdSym ll[1 << 9], of[1 << 9], ml[1 << 9];  // the reference reads a table log of up to 9 for all three (zstd/fse_decoder.go tablelogAbsoluteMax)
    ZdSym wt[1 << 7];       // FSE table of the Huffman weights, up to table log 7 (a larger one goes to the frame's literal scratch)
    uint8_t weights[256];
    int16_t norm[64];
    uint16_t next[64];
    uint32_t seqLL[64], seqML[64], seqOF[64];
    int iv[16];
};
enum { V_ERR = 0, V_HUFLOG, V_LLLOG, V_OFLOG, V_MLLOG, V_LLOK, V_OFOK, V_MLOK, V_HUFOK, V_NBATCH };

__device__ __forceinline__ int zd_hibit(uint32_t v) { return 31 - __builtin_clz(v); }

// backward bit reader (zstd/bitreader.go) over global memory: `pos` = unread bits
struct ZdRBits {
    const uint8_t* p;
    long pos;
    __device__ bool init(const uint8_t* d, int n) {
        if (n <= 0 || d[n - 1] == 0) return false;
        p = d;
        pos = (long)n * 8 - (8 - zd_hibit(d[n - 1]));
        return true;
    }
    __device__ uint32_t peek(int nb) const {  // next nb (<= 24) bits, most significant first, zeros below bit 0
        if (nb == 0) return 0;
        const long lo = pos - nb;  // lowest bit index wanted (may be negative)
        uint64_t w = 0;
        const long b0 = (lo < 0 ? 0 : lo) >> 3;
        for (int k = 0; k < 5; k++) {
            const long bi = b0 + k;
            if (bi * 8 < pos) w |= (uint64_t)p[bi] << (8 * k);
        }
        if (lo >= 0) return (uint32_t)((w >> (lo & 7)) & ((1u << nb) - 1u));
        const int have = (int)pos;  // fewer than nb bits left: they are the high part, zeros fill the rest
        if (have <= 0) return 0;
        return (uint32_t)((w & ((1ull << have) - 1ull)) << (nb - have)) & ((1u << nb) - 1u);
    }
    __device__ uint32_t read(int nb) { const uint32_t v = peek(nb); pos -= nb; return v; }
};

// forward bit cursor for FSE table descriptions (zero padded past the end)
struct ZdFBits {
    const uint8_t* p;
    int n;
    int bit;
    __device__ uint32_t peek(int nb) const {
        uint64_t v = 0;
        const int b0 = bit >> 3;
        for (int k = 0; k < 5; k++) if (b0 + k < n) v |= (uint64_t)p[b0 + k] << (8 * k);
        return (uint32_t)((v >> (bit & 7)) & ((1ull << nb) - 1ull));
    }
    __device__ uint32_t take(int nb) { const uint32_t v = peek(nb); bit += nb; return v; }
};

// FSE_Table_Description -> norm[] (fse_decoder.go:52-184).  Returns bytes consumed, 0 on error.  Lane 0 only.
__device__ int zd_read_ncount(const uint8_t* p, int n, int maxSym, int maxLog, int16_t* norm, int* nSym, int* tableLog) {
    if (n < 1) return 0;
    ZdFBits b{p, n, 0};
    const int tl = (int)b.take(4) + 5;
    if (tl > maxLog) return 0;
    int remaining = 1 << tl, sym = 0;
    while (remaining > 0 && sym <= maxSym) {
        const int maxv = remaining + 1;
        const int bits = zd_hibit((uint32_t)maxv) + 1;
        const int lowThreshold = (1 << bits) - 1 - maxv;
        int v = (int)b.peek(bits - 1);
        if (v < lowThreshold) b.bit += bits - 1;
        else { v = (int)b.take(bits); if (v >= (1 << (bits - 1))) v -= lowThreshold; }
        const int prob = v - 1;
        if (prob > 32767) return 0;  // (table log 15, one symbol with every cell: no stream can follow such a table)
        norm[sym++] = (int16_t)prob;
        remaining -= prob < 0 ? 1 : prob;
        if (prob == 0) {
            for (;;) {
                const int rep = (int)b.take(2);
                for (int k = 0; k < rep && sym <= maxSym; k++) norm[sym++] = 0;
                if (rep != 3) break;
                if (b.bit > n * 8) return 0;
            }
        }
        if (b.bit > n * 8) return 0;
    }
    if (remaining != 0 || sym <= 1) return 0;
    *nSym = sym;
    *tableLog = tl;
    return (b.bit + 7) >> 3;
}

// fse_decoder.go buildDtable: norm -> decoding cells.  Lane 0 only.
__device__ bool zd_build_fse(const int16_t* norm, int nSym, int tl, ZdSym* dt, uint16_t* next) {
    const int size = 1 << tl;
    int high = size - 1;
    for (int s = 0; s < nSym; s++) {
        if (norm[s] == -1) { dt[high--].sym = (uint8_t)s; next[s] = 1; }
        else next[s] = (uint16_t)norm[s];
    }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nSym; s++)
        for (int k = 0; k < norm[s]; k++) {
            dt[pos].sym = (uint8_t)s;
            do { pos = (pos + step) & mask; } while (pos > high);
        }
    if (pos != 0) return false;
    for (int u = 0; u < size; u++) {
        const uint16_t nx = next[dt[u].sym]++;
        if (nx == 0) return false;
        const int nb = tl - zd_hibit(nx);
        dt[u].nb = (uint8_t)nb;
        dt[u].base = (uint16_t)((nx << nb) - size);
    }
    return true;
}

__constant__ int16_t kLLNorm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ int16_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__constant__ int16_t kMLNorm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                    1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ uint32_t kLLBase[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
                                     1024, 2048, 4096, 8192, 16384, 32768, 65536};
__constant__ uint32_t kMLBase[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                                     33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};

// One sequence table according to its mode (blockdec.go:560-640).  Lane 0 only.  Returns bytes consumed (>= 0) or -1.
__device__ int zd_seq_table(int mode, int kind, const uint8_t* p, int n, ZdShared& S) {
    ZdSym* dt = kind == 0 ? S.ll : (kind == 1 ? S.of : S.ml);
    const int maxSym = kind == 0 ? 35 : (kind == 1 ? 30 : 52);  // maxOffsetLengthSymbol = 30 (zstd/fse_predefined.go:45)
    const int maxLog = 9;
    if (mode == 0) {
        const int16_t* src = kind == 0 ? kLLNorm : (kind == 1 ? kOFNorm : kMLNorm);
        const int ns = kind == 0 ? 36 : (kind == 1 ? 29 : 53);
        const int tl = kind == 1 ? 5 : 6;
        for (int i = 0; i < ns; i++) S.norm[i] = src[i];
        if (!zd_build_fse(S.norm, ns, tl, dt, S.next)) return -1;
        S.iv[V_LLLOG + kind] = tl;
        S.iv[V_LLOK + kind] = 1;
        return 0;
    }
    if (mode == 1) {
        if (n < 1 || p[0] > maxSym) return -1;
        dt[0].sym = p[0]; dt[0].nb = 0; dt[0].base = 0;
        S.iv[V_LLLOG + kind] = 0;
        S.iv[V_LLOK + kind] = 1;
        return 1;
    }
    if (mode == 2) {
        int ns = 0, tl = 0;
        const int used = zd_read_ncount(p, n, maxSym, maxLog, S.norm, &ns, &tl);
        if (used == 0 || used > n) return -1;
        if (!zd_build_fse(S.norm, ns, tl, dt, S.next)) return -1;
        S.iv[V_LLLOG + kind] = tl;
        S.iv[V_LLOK + kind] = 1;
        return used;
    }
    return S.iv[V_LLOK + kind] ? 0 : -1;  // repeat
}

// FSE-compressed Huffman weights (huff0/decompress.go:57-70 -> fse.Decompress).  Lane 0.  Returns count or -1.
// The reference's fse package takes a table log of up to 15 and any of 256 symbols here (fse/decompress.go readNCount), whatever the
// weights turn out to be.  The counts live in S.huf, which the new code is about to replace; a table of log 8 or more lives in
// `scratch` (the frame's literal scratch, free until this block's literals are decoded), and is refused if that cannot hold it.
__device__ int zd_fse_weights(const uint8_t* p, int n, ZdShared& S, uint8_t* out, uint8_t* scratch, uint32_t scratchBytes) {
    int ns = 0, tl = 0;
    int16_t* norm = (int16_t*)S.huf;
    uint16_t* next = S.huf + 256;
    const int hdr = zd_read_ncount(p, n, 255, 15, norm, &ns, &tl);
    if (hdr == 0 || hdr >= n) return -1;
    ZdSym* dt = S.wt;  // the sequence tables must survive: a later block may use them in repeat mode
    if (tl > 7) {
        const uint32_t skip = (uint32_t)(4 - ((uintptr_t)scratch & 3)) & 3;
        if (scratchBytes < skip || ((size_t)sizeof(ZdSym) << tl) > (size_t)(scratchBytes - skip)) return -1;
        dt = (ZdSym*)(scratch + skip);
    }
    if (!zd_build_fse(norm, ns, tl, dt, next)) return -1;
    ZdRBits br;
    if (!br.init(p + hdr, n - hdr)) return -1;
    uint32_t s1 = br.read(tl), s2 = br.read(tl);
    if (br.pos < 0) return -1;
    int w = 0;
    for (;;) {
        if (w + 2 > 255) return -1;
        out[w++] = dt[s1].sym;
        s1 = dt[s1].base + br.read(dt[s1].nb);
        if (br.pos < 0) { out[w++] = dt[s2].sym; break; }
        if (w + 2 > 255) return -1;
        out[w++] = dt[s2].sym;
        s2 = dt[s2].base + br.read(dt[s2].nb);
        if (br.pos < 0) { out[w++] = dt[s1].sym; break; }
    }
    return w;
}

}  // namespace
