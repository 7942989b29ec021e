// kc_stateless_dev.h — flate.StatelessDeflate on the device: what the kernels of kc_flate_stateless.hip share.
//
// Semantics: StatelessDeflate (flate/stateless.go:76-162) and statelessEnc (:176-325); tokens.AddMatchLong, AddEOB, EstimatedBits and
// mFastLog2 (flate/token.go:284-309, :311-315, :225-260, :212-220); writeBlockDynamic (flate/huffman_bit_writer.go:620-765) with
// canReuse (:163-190), indexTokens (:784-815), extraBitSize / fixedSize / storedSize / dynamicSize / dynamicReuseSize / headerSize
// (:350-419), writeFixedHeader (:531-547) and writeTokens (:824-975); writeBlockHuff and what it calls as kc_deflate_dev.h restates them;
// gzip's Write and Close at StatelessCompression (gzip/gzip.go:230-231, :278-279).
//
// THE PENALTY IS 0.  StatelessDeflate takes its bit writer from bitWriterPool: newHuffmanBitWriter(nil) and reset, which leave
// logNewTablePenalty at its zero value — not the 10 compressor.init gives HuffmanOnly.  So newSize>>0 DOUBLES the estimate of a new
// table in writeBlockDynamic (:665), and estBits += estBits>>0 doubles it in writeBlockHuff (:1042).  A quirk, and the bytes depend on it.
//
// In the reference itself every block is found independently: the input is cut at fixed places (the first block 32767 - len(dict)
// bytes, every later one 24575 behind 8192 bytes of history that are the input's own), and each block gets a fresh 8192-entry table.
// What spans blocks is the bit writer's state: lastHeader, lastHuffMan, the table in force, the owed EOB, the bit position.  So the
// work is cut by BLOCK: match (one wave per block: statelessEnc, tokens to scratch, the three histograms into the record), plan (one
// wave per block: everything about a block that does not depend on the blocks before it), chain (one wave per input: the reference's
// decisions in order) and emit (one wave per block: bits at the position the chain gave).
#pragma once
#include "kc_deflate_dev.h"

#define KCSL_MAX_BLOCK 32767u   // maxStatelessBlock
#define KCSL_MAX_DICT 8192u     // maxStatelessDict
#define KCSL_LATER (KCSL_MAX_BLOCK - KCSL_MAX_DICT)
#define KCSL_PREDEF 250u        // maxPredefinedTokens
#define KCSL_MATCH 0x40000000u  // matchType; a match token is matchType | length-3 << 22 | offset code << 16 | offset-1 (token.go:15-26)
#define KCSL_COMB 32768u        // a dictionary call: the slot of dictionary + first block per input
// a block's class (stateless.go:134-145)
#define KCSL_C_NONE 0u     // the record of an empty input
#define KCSL_C_STORED 1u   // dst.n == 0
#define KCSL_C_HUFF 2u     // dst.n > len - len>>4: writeBlockHuff
#define KCSL_C_DYN 3u      // writeBlockDynamic
// how the chain has a block written
#define KCSL_W_NONE 0u
#define KCSL_W_STORED 1u
#define KCSL_W_FIXED 2u    // its tokens under the fixed tables
#define KCSL_W_TOKENS 3u   // its tokens under rec[table]
#define KCSL_W_BYTES 4u    // its bytes as literals under rec[table]
#define KCSL_F_OWED 1u     // an EOB of rec[prev_table] comes first
#define KCSL_F_EOB 2u      // the block ends with the EOB of its table
#define KCSL_F_LAST 4u     // the stream's end follows
#define KCSL_F_HEADER 8u   // the dynamic header of the block's own table comes first
#define KCSL_F_FINAL 16u   // the header carries the final bit (isEof)
// the decision counters of tests/stateless_model.py, then those of writeBlockHuff (tests/deflate_model.py)
enum { KCSL_N_STORED_NO_MATCH, KCSL_N_HUFFMAN_ONLY, KCSL_N_DYN_FIRST, KCSL_N_DYN_REUSE, KCSL_N_DYN_NEW_OWED, KCSL_N_DYN_FIXED, KCSL_N_DYN_STORED,
       KCSL_N_CANNOT_REUSE, KCSL_N_H_QUICK, KCSL_N_H_EST, KCSL_N_H_FIRST, KCSL_N_H_REUSE, KCSL_N_H_NEW_OWED, KCSL_N_H_NOT_REUSABLE, KCSL_N_COUNTS = 16 };

// hist: literalFreq's layout, then offsetFreq: [0, 256) litHist, [256] EOB, [257 + c] length code c (extraHist[c + 1]), [288 + c] offset
// code c.  A KCSL_C_HUFF block has the histogram of its BYTES in [0, 256) from the plan on.
struct KcSlBlock {
    // match
    uint16_t hist[320];
    uint32_t ntok;           // dst.n
    // plan
    uint32_t cls;
    uint16_t code[288];      // the block's own tables: canonical codes, bit-reversed
    uint8_t len[288];
    uint16_t ocode[32];
    uint8_t olen[32];
    uint8_t codegen[320];    // generateCodegen's sequence, extras in line, n_codegen bytes
    uint16_t cgcode[20];
    uint8_t cglen[20];
    uint32_t n_codegen, ncg, hdr_bits, num_lit, num_off;
    uint32_t self_bits;      // every code of the block under its own tables, one EOB included (no extra bits)
    uint32_t extra_bits, fixed_bits, est_bits;  // extraBitSize, fixedSize(extraBits), tokens.EstimatedBits
    uint32_t quick;          // writeBlockHuff's quick check says stored
    // chain
    uint32_t how, flags;
    uint32_t table, prev_table;  // records: the tables the codes come from; the table an owed EOB comes from
    uint64_t start_bit;      // in the input's DEFLATE stream, of the first bit this block writes (an owed EOB included)
};

struct KcStatelessParams {
    const uint8_t* src;
    const uint64_t* in_off;   // n + 1
    uint32_t n;
    uint32_t gzip, eof;       // gzip: Write + Close, header and trailer around; eof: StatelessDeflate's argument (gzip: 0)
    uint32_t penalty;         // logNewTablePenalty: 0
    uint32_t dict_len;        // <= 8192
    const uint8_t* dict;      // dict_len bytes
    uint8_t* comb;            // dict_len != 0: n slots of KCSL_COMB bytes, the dictionary and the first block's bytes of every input
    const uint32_t* blk0;     // n + 1: the first record of every input; every input has at least one record
    const uint32_t* blk_in;   // nblocks: the input of every record
    uint32_t nblocks;
    KcSlBlock* rec;
    uint32_t* tok;            // the tokens of every block, len + 1 words each ...
    const uint64_t* tok0;     // ... nblocks: where a block's begin
    uint64_t* size;           // chain: the exact bytes of every input's output
    uint32_t* crc;            // chain, gzip: CRC-32 of every input
    uint32_t* counts;         // chain: KCSL_N_COUNTS decision counters, added to
    // emit
    const uint64_t* out0;     // where input i's output starts in dst
    uint8_t* dst;             // zeroed over [0, total)
    uint64_t total;
    uint32_t* edge;           // [2], zeroed (DfSink)
};
void kc_launch_stateless_gather(const KcStatelessParams& P, hipStream_t st);
void kc_launch_stateless_match(const KcStatelessParams& P, hipStream_t st);
void kc_launch_stateless_plan(const KcStatelessParams& P, hipStream_t st);
void kc_launch_stateless_chain(const KcStatelessParams& P, hipStream_t st);
void kc_launch_stateless_emit(const KcStatelessParams& P, hipStream_t st);

// the bytes of record r: `n` bytes at `pos` of input `input` (stateless.go:106-116)
struct SlSpan { uint64_t begin; uint32_t input, idx, nblk, pos, n; };
__device__ __forceinline__ SlSpan sl_span(const KcStatelessParams& P, const uint32_t r) {
    SlSpan s;
    s.input = P.blk_in[r];
    s.idx = r - P.blk0[s.input];
    s.nblk = P.blk0[s.input + 1] - P.blk0[s.input];
    s.begin = P.in_off[s.input];
    const uint64_t len = P.in_off[s.input + 1] - s.begin;
    const uint32_t first = KCSL_MAX_BLOCK - P.dict_len;
    s.pos = s.idx == 0 ? 0u : first + (s.idx - 1) * KCSL_LATER;
    const uint32_t most = s.idx == 0 ? first : KCSL_LATER;
    s.n = (uint32_t)(len - s.pos < most ? len - s.pos : most);
    return s;
}

__device__ __forceinline__ uint32_t sl_hash(const uint32_t u) { return (u * 0x1e35a7bdu) >> (32 - 13); }  // hashSL
// lengthCode(length - 3) (token.go:30-57) and offsetCode(offset - 1) (:89-126, :365-379) in closed form; their extra bits
// (huffman_bit_writer.go:44-68).  The extra VALUE is the low `extra bits` bits of the argument: every base is a multiple of 2^extra.
__device__ __forceinline__ uint32_t sl_length_code(const uint32_t xl) {
    if (xl < 8) return xl;
    if (xl == 255) return 28;
    const uint32_t e = 29u - (uint32_t)__builtin_clz(xl);  // bits.Len32(xl) - 3
    return 4 + 4 * e + ((xl >> e) & 3u);
}
__device__ __forceinline__ uint32_t sl_length_extra(const uint32_t lc) { return lc < 8 || lc == 28 ? 0u : (lc - 4) >> 2; }
__device__ __forceinline__ uint32_t sl_offset_code(const uint32_t off) {
    if (off < 4) return off;
    const uint32_t h = 31u - (uint32_t)__builtin_clz(off);
    return 2 * h + ((off >> (h - 1)) & 1u);
}
__device__ __forceinline__ uint32_t sl_offset_extra(const uint32_t oc) { return oc < 4 ? 0u : (oc >> 1) - 1; }

// fixedLiteralEncoding / fixedOffsetEncoding (huffman_code.go:80-121): the length and the bit-reversed code of symbol k
__device__ __forceinline__ uint32_t sl_fixed_lit(const uint32_t k) {  // code | len << 16
    uint32_t code, len;
    if (k < 144) { code = 0x30 + k; len = 8; }
    else if (k < 256) { code = 0x190 + (k - 144); len = 9; }
    else if (k < 280) { code = k - 256; len = 7; }
    else { code = 0xC0 + (k - 280); len = 8; }
    return df_reverse(code, len) | len << 16;
}
__device__ __forceinline__ uint32_t sl_fixed_off(const uint32_t k) { return df_reverse(k, 5) | 5u << 16; }

// generateCodegen (huffman_bit_writer.go:269-348) over lens[0, nlit) and olens[0, noff); ONE lane.  Returns the sequence's bytes (at
// most nlit + noff: the output is never longer than the input); cgfreq[19] are its frequencies.
__device__ __forceinline__ uint32_t sl_codegen(const uint8_t* lens, const int nlit, const uint8_t* olens, const int noff, uint8_t* out, uint32_t* cgfreq) {
    for (int k = 0; k < 19; k++) cgfreq[k] = 0;
    auto at = [&](int k) -> uint32_t { return k < nlit ? lens[k] : k < nlit + noff ? olens[k - nlit] : 255u; };
    uint32_t size = at(0), o = 0;
    int count = 1;
    for (int in = 1; size != 255u; in++) {
        const uint32_t next = at(in);
        if (next == size) { count++; continue; }
        if (size != 0) {
            out[o++] = (uint8_t)size; cgfreq[size]++; count--;
            while (count >= 3) {
                const int k = count < 6 ? count : 6;
                out[o++] = 16; out[o++] = (uint8_t)(k - 3); cgfreq[16]++; count -= k;
            }
        } else {
            while (count >= 11) {
                const int k = count < 138 ? count : 138;
                out[o++] = 18; out[o++] = (uint8_t)(k - 11); cgfreq[18]++; count -= k;
            }
            if (count >= 3) { out[o++] = 17; out[o++] = (uint8_t)(count - 3); cgfreq[17]++; count = 0; }
        }
        count--;
        for (; count >= 0; count--) { out[o++] = (uint8_t)size; cgfreq[size]++; }
        size = next;
        count = 1;
    }
    return o;
}

// mFastLog2 (token.go:212-220) and tokens.EstimatedBits (:225-260; nFilled is 0 on this path) on ONE lane, in the order of the
// reference's loops.  The value to reproduce is the reference's default amd64 build: unfused IEEE single precision, a correctly
// rounded division, truncated by int().  So no contraction here: the pragma holds for the device compiler, which fuses by default;
// the host compiler of the emulator build fuses nothing at its baseline target.
__device__ __forceinline__ float sl_fast_log2(const float val) {
#pragma clang fp contract(off)
    int32_t ux;
    __builtin_memcpy(&ux, &val, 4);
    float log2 = (float)(((ux >> 23) & 255) - 128);
    ux &= -0x7f800001;
    ux += 127 << 23;
    float uval;
    __builtin_memcpy(&uval, &ux, 4);
    float t = -0.34484843f * uval;
    t = t + 2.02466578f;
    t = t * uval;
    t = t - 0.67487759f;
    log2 = log2 + t;
    return log2;
}
__device__ __forceinline__ float sl_shannon_term(const uint32_t v, const float inv) {
#pragma clang fp contract(off)
    const float n = (float)v;
    float b = -sl_fast_log2(n * inv);
    // atLeastOne (huffman_code.go:374-382) also clamps at 15.  Not restated: EstimatedBits is only asked where a block goes to
    // writeBlockDynamic, i.e. with at most 30 720 tokens (15/16 of 32 767) and an EOB, so n * inv >= 1 / 30 721 and b <= 14.91.
    if (b < 1.0f) b = 1.0f;
    const float p = b * n;
    return p;
}
// freq: KcSlBlock::hist's layout; total: t.n, an EOB token included where the block is written with sync
__device__ __forceinline__ uint32_t sl_estimated_bits(const uint32_t* freq, const uint32_t total) {
#pragma clang fp contract(off)
    float shannon = 0.0f;
    uint32_t bits = 0, n_matches = 0;
    if (total > 0) {
        const float inv = 1.0f / (float)total;
        for (int k = 0; k < 256; k++) {
            const uint32_t v = freq[k];
            if (v) { const float p = sl_shannon_term(v, inv); shannon = shannon + p; }
        }
        shannon = shannon + 15.0f;
        for (uint32_t c = 0; c < 29; c++) {
            const uint32_t v = freq[257 + c];
            if (v) {
                const float p = sl_shannon_term(v, inv);
                shannon = shannon + p;
                bits += sl_length_extra(c) * v;
                n_matches += v;
            }
        }
    }
    if (n_matches > 0) {
        const float inv = 1.0f / (float)n_matches;
        for (uint32_t c = 0; c < 30; c++) {
            const uint32_t v = freq[288 + c];
            if (v) {
                const float p = sl_shannon_term(v, inv);
                shannon = shannon + p;
                bits += sl_offset_extra(c) * v;
            }
        }
    }
    return (uint32_t)(int32_t)shannon + bits;
}
