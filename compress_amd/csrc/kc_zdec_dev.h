// kc_zdec_dev.h — the zstd block parser of the device, written once for the three decoders: the verifier (kc_zstd_decode.hip),
// DecodeAll (kc_zstd_decode_all.hip) and the stream reader (kc_zstd_dstream.hip).  FSE decoding cells, the backward / forward bit
// readers, FSE_Table_Description parsing, table construction, the predefined distributions and the code tables of literal lengths,
// match lengths and offsets; and on top of them the sections of a compressed block as blockdec.go:275-650 walks them: the literals
// header and the sequence count (kc_zblock_dev.h, shared with the host), the Huffman tree description, the 1X / 4X streams, the three
// sequence tables, the sequence loop for a group of 64 and the offset history.  The functions return 0 or an error class (a length or
// -1 where they consume bytes); what a failure is called, where the output goes and where repeated tables come from is the caller's.
#pragma once
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zblock_dev.h"

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

// The FSE_Table_Description of sequence table `kind` (0 literal lengths, 1 offsets, 2 match lengths) -> S.norm.  The reference's table
// reader wants four readable bytes in front of it (fse_decoder.go:57).  Lane 0 only.  Returns bytes consumed or -1.
__device__ __forceinline__ int zd_seq_ncount(int kind, const uint8_t* p, int n, ZdShared& S, int* nSym, int* tableLog) {
    const int maxSym = kind == 0 ? 35 : (kind == 1 ? 30 : 52);  // maxOffsetLengthSymbol = 30 (zstd/fse_predefined.go:45)
    if (n < 4) return -1;
    const int used = zd_read_ncount(p, n, maxSym, 9, S.norm, nSym, tableLog);
    return used == 0 || used > n ? -1 : used;
}

// The bytes a sequence table's description takes, without building the table.  Lane 0 only.  Returns bytes (>= 0) or -1.
__device__ __forceinline__ int zd_seq_table_skip(int mode, int kind, const uint8_t* p, int n, ZdShared& S) {
    int ns = 0, tl = 0;
    if (mode == 1) return n < 1 ? -1 : 1;
    return mode == 2 ? zd_seq_ncount(kind, p, n, S, &ns, &tl) : 0;
}

// One sequence table according to its mode (blockdec.go:556-640).  Lane 0 only.  Returns bytes consumed (>= 0) or -1.
__device__ int zd_seq_table(int mode, int kind, const uint8_t* p, int n, ZdShared& S) {
    ZdSym* dt = kind == 0 ? S.ll : (kind == 1 ? S.of : S.ml);
    const int maxSym = kind == 0 ? 35 : (kind == 1 ? 30 : 52);
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
        const int used = zd_seq_ncount(kind, p, n, S, &ns, &tl);
        if (used < 0) return -1;
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

// The three sequence tables of a block according to the modes byte at sp[0] (blockdec.go:556-622): lane 0 builds them, the whole wave
// learns the bytes they took (the modes byte included), or -1.  A table in Repeat_Mode must be in S already (S.iv[V_LLOK + kind]).
__device__ __forceinline__ int zd_seq_tables(const uint8_t* sp, int sn, ZdShared& S, int lane) {
    if (lane == 0) {
        int q2 = sn < 1 || (sp[0] & 3) ? -1 : 1;
        for (int kind = 0; kind < 3 && q2 > 0; kind++) {
            const int r = zd_seq_table(zd_seq_mode(sp[0], kind), kind, sp + q2, sn - q2, S);
            q2 = r < 0 ? -1 : q2 + r;
        }
        S.iv[V_NBATCH] = q2;
    }
    KC_WAVE_SYNC();
    const int used = S.iv[V_NBATCH];
    KC_EMU_SYNC();
    return used;
}

// Huffman_Tree_Description at q (left bytes) -> S.huf, S.iv[V_HUFLOG], S.iv[V_HUFOK] (huff0/decompress.go:29-168): weights on lane 0,
// table fill on all lanes.  Whole wave.  scratch: where a weight table of log 8 or more lives meanwhile (zd_fse_weights).  Returns
// the bytes the description took, or -1.
__device__ __forceinline__ int zd_huf_table(const uint8_t* q, int left, ZdShared& S, int lane, uint8_t* scratch, uint32_t scratchBytes) {
    if (lane == 0) {
        int e2 = 0, used = 0, nw = 0;
        const int hb = left > 0 ? q[0] : 0;
        if (left < 2) e2 = 1;
        else if (hb >= 128) {
            nw = hb - 127;
            used = 1 + (nw + 1) / 2;
            if (used > left) e2 = 1;
            else for (int k = 0; k < nw; k++) S.weights[k] = (k & 1) ? (q[1 + (k >> 1)] & 15) : (q[1 + (k >> 1)] >> 4);
        } else {
            used = 1 + hb;
            if (hb == 0 || used > left) e2 = 1;
            else { nw = zd_fse_weights(q + 1, hb, S, S.weights, scratch, scratchBytes); if (nw <= 0) e2 = 1; }
        }
        int tableLog = 0;
        if (!e2) {
            uint32_t total = 0, rank1 = 0;
            for (int k = 0; k < nw; k++) { if (S.weights[k] > 11) e2 = 1; total += (1u << (S.weights[k] & 15)) >> 1; rank1 += S.weights[k] == 1; }
            if (!e2 && total == 0) e2 = 1;
            if (!e2) {
                tableLog = zd_hibit(total) + 1;
                const uint32_t rest = (1u << tableLog) - total;
                if (tableLog > 11 || rest == 0 || (rest & (rest - 1)) != 0) e2 = 1;
                else {
                    const int lastW = zd_hibit(rest) + 1;
                    rank1 += lastW == 1;
                    if (rank1 < 2 || (rank1 & 1)) e2 = 1;  // "min elt size, even check failed"
                    S.weights[nw++] = (uint8_t)lastW;
                    for (int k = nw; k < 256; k++) S.weights[k] = 0;
                }
            }
        }
        S.iv[V_HUFLOG] = tableLog;
        S.iv[V_HUFOK] = e2 ? 0 : 1;
        S.iv[V_NBATCH] = e2 ? -1 : used;
    }
    KC_WAVE_SYNC();
    const int used = S.iv[V_NBATCH], tableLog = S.iv[V_HUFLOG];
    KC_EMU_SYNC();
    if (used < 0) return -1;
    // start of each symbol's cell range: cells are ordered by (weight asc, symbol asc)
    for (int s0 = 0; s0 < 256; s0 += 64) {
        const int sy = s0 + lane;
        const int w = S.weights[sy];
        if (w) {
            uint32_t start = 0;
            for (int t = 0; t < 256; t++) {
                const int wt = S.weights[t];
                if (wt && (wt < w || (wt == w && t < sy))) start += (1u << wt) >> 1;
            }
            const uint32_t len = (1u << w) >> 1;
            const uint16_t e = (uint16_t)((sy << 8) | (tableLog + 1 - w));
            for (uint32_t k = 0; k < len; k++) S.huf[start + k] = e;
        }
    }
    KC_WAVE_SYNC();
    return used;
}

// The Huffman streams of a literals section at q (left bytes), one (Decompress1X) or four behind their jump table (Decompress4X), one
// lane each, `regen` symbols into lits.  Whole wave.  Returns 0 or the error class.
__device__ __forceinline__ int zd_huf_streams(const uint8_t* q, int left, bool four, uint32_t regen, const ZdShared& S, int lane, uint8_t* lits) {
    const int hlog = S.iv[V_HUFLOG];
    int sOff = 0, sLen = left, oOff = 0, oLen = (int)regen;  // this lane's stream and where its symbols go
    int nstreams = 1;
    if (four) {
        if (left < 10) return KCZD_CORRUPT;  // the jump table and a byte per stream (decompress_generic.go:19)
        const int s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8), s3 = q[4] | (q[5] << 8);
        if (6 + s1 + s2 + s3 > left) return KCZD_CORRUPT;
        const int seg = ((int)regen + 3) / 4;
        if (seg * 3 > (int)regen) return KCZD_CORRUPT;
        const int k = lane & 3;
        sOff = 6 + (k > 0 ? s1 : 0) + (k > 1 ? s2 : 0) + (k > 2 ? s3 : 0);
        sLen = k == 0 ? s1 : (k == 1 ? s2 : (k == 2 ? s3 : left - sOff));
        oOff = k * seg;
        oLen = k < 3 ? seg : (int)regen - 3 * seg;
        nstreams = 4;
    }
    int serr = 0;
    if (lane < nstreams) {
        ZdRBits br;
        if (!br.init(q + sOff, sLen)) serr = 1;
        else {
            uint8_t* o = lits + oOff;
            for (int i = 0; i < oLen; i++) {
                const uint16_t e = S.huf[br.peek(hlog)];
                o[i] = (uint8_t)(e >> 8);
                br.pos -= (e & 0xFF);
            }
            if (br.pos != 0) serr = 1;
        }
    }
    if (ballot64(serr != 0)) return KCZD_CORRUPT;
    KC_WAVE_SYNC();
    return 0;
}

// The offset history (seqdec.go:262-300): the offset an offset value stands for, and the three repeat offsets behind it.  ofVal 1 .. 3
// is a repeat code (shifted by one when the sequence has no literals), 4 and up the offset ofVal - 3.  Returns 0, with 0 at the head of
// the history, where a repeat code resolves to no offset at all: the reference forces that to 1; the caller forces or refuses.
__device__ __forceinline__ uint32_t zd_rep_offset(uint32_t ofVal, uint32_t llen, uint32_t& rep0, uint32_t& rep1, uint32_t& rep2) {
    if (ofVal > 3) { rep2 = rep1; rep1 = rep0; rep0 = ofVal - 3; return rep0; }
    const uint32_t idx = ofVal + (llen == 0 ? 1u : 0u);  // 1: repeat 1, 2: repeat 2, 3: repeat 3, 4: repeat 1 minus one byte
    if (idx == 1) return rep0;
    const uint32_t off = idx == 4 ? rep0 - 1 : (idx == 2 ? rep1 : rep2);
    if (idx != 2) rep2 = rep1;
    rep1 = rep0;
    rep0 = off;
    return off;
}

// The sequence bitstream of a block between two groups: lane 0's reader and FSE states.
struct ZdSeqDec {
    ZdRBits br;
    uint32_t llS, ofS, mlS;
};
// Opens the bitstream at sp (sn bytes) and reads the three initial states.  Whole wave.  Returns 0, KCZD_CORRUPT or, where the reader
// ran dry, KCZD_EOF.
__device__ __forceinline__ int zd_seq_open(ZdSeqDec& q, const uint8_t* sp, int sn, const ZdShared& S, int lane) {
    q.br.p = nullptr; q.br.pos = 0;
    q.llS = q.ofS = q.mlS = 0;
    int e = 0;
    if (lane == 0) {
        if (!q.br.init(sp, sn)) e = KCZD_CORRUPT;
        else {
            q.llS = q.br.read(S.iv[V_LLLOG]); q.ofS = q.br.read(S.iv[V_OFLOG]); q.mlS = q.br.read(S.iv[V_MLLOG]);
            if (q.br.pos < 0) e = KCZD_EOF;  // (io.ErrUnexpectedEOF)
        }
    }
    return uni(e);
}
// Sequences s0 .. s0 + cnt (cnt <= 64) of the block's nSeq on lane 0 (seqdec.go:221-434): symbols against their limits, extra bits,
// next states; (litLen, matchLen, offset) of sequence s0 + i are left in S.seqLL / seqML / seqOF[i] for the whole wave.  What an offset
// value becomes is the caller's: offset(ofVal, litLen, off) sets `off` or returns false to refuse the sequence.  Whole wave.  Returns 0,
// KCZD_EOF where the reader ran dry, else KCZD_CORRUPT (the last group: "extra bits on block").
template <class Offset>
__device__ __forceinline__ int zd_seq_group(ZdSeqDec& q, ZdShared& S, int lane, int s0, int cnt, int nSeq, Offset offset) {
    if (lane == 0) {
        int e2 = 0;
        for (int i = 0; i < cnt; i++) {
            const ZdSym cl = S.ll[q.llS], co = S.of[q.ofS], cm = S.ml[q.mlS];
            if (cl.sym > 35 || cm.sym > 52 || co.sym > 30) { e2 = KCZD_CORRUPT; break; }
            uint32_t ofVal;
            if (co.sym <= 24) ofVal = (1u << co.sym) + q.br.read(co.sym);
            else { const uint32_t hi = q.br.read(co.sym - 16); const uint32_t lo = q.br.read(16); ofVal = (1u << co.sym) + ((hi << 16) | lo); }
            const uint32_t mlen = kMLBase[cm.sym] + q.br.read(kMLBits[cm.sym]);
            const uint32_t llen = kLLBase[cl.sym] + q.br.read(kLLBits[cl.sym]);
            uint32_t off;
            if (!offset(ofVal, llen, off)) { e2 = KCZD_CORRUPT; break; }
            if (s0 + i + 1 < nSeq) {
                q.llS = cl.base + q.br.read(cl.nb);
                q.mlS = cm.base + q.br.read(cm.nb);
                q.ofS = co.base + q.br.read(co.nb);
            }
            if (q.br.pos < 0) { e2 = KCZD_EOF; break; }
            S.seqLL[i] = llen; S.seqML[i] = mlen; S.seqOF[i] = off;
        }
        if (!e2 && s0 + cnt >= nSeq && q.br.pos != 0) e2 = KCZD_CORRUPT;  // "extra bits on block"
        S.iv[V_ERR] = e2;
    }
    KC_WAVE_SYNC();
    const int e2 = S.iv[V_ERR];
    KC_EMU_SYNC();
    return e2;
}

// FSE cells between LDS and the layout a dictionary or a stream's carried state keeps them in.  Whole wave.
__device__ __forceinline__ void zd_cells_in(ZdSym* dst, const KcZdCell* src, int n, int lane) {
    for (int k = lane; k < n; k += 64) { const KcZdCell a = src[k]; dst[k].base = a.base; dst[k].sym = a.sym; dst[k].nb = a.nb; }
}
__device__ __forceinline__ void zd_cells_out(KcZdCell* dst, const ZdSym* src, int n, int lane) {
    for (int k = lane; k < n; k += 64) { KcZdCell a; a.base = src[k].base; a.sym = src[k].sym; a.nb = src[k].nb; dst[k] = a; }
}

}  // namespace
