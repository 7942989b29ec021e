// kc_deflate_dev.h — the block writer of flate.HuffmanOnly on the device: what the three kernels of kc_flate_deflate.hip share.
//
// Semantics: writeBlockHuff (flate/huffman_bit_writer.go:987-1174) with generateCodegen (:269-348), codegens / headerSize (:350-368),
// writeDynamicHeader (:458-497), writeStoredHeader (:502-529) and flush (:192-218); huffmanEncoder.generate, bitCounts and
// assignEncodingAndSize (flate/huffman_code.go:339-371, :183-309, :313-333); the stream rules of compressor.write / storeHuff /
// close / syncFlush (flate/deflate.go:755-770, :701-708, :865-880, :772-785); gzip's default header and trailer (gzip/gzip.go).
//
// A block of HuffmanOnly has no history.  What one block needs of the blocks before it is three numbers: lastHeader, which block's
// table is in force, and the bit position.  So the work is cut by BLOCK: the plan kernel gives every block its histogram, its quick
// check, its own candidate table and that table's header (one wave per block, any input); the chain kernel walks each input's
// blocks in order and takes the reference's decisions (one wave per input); the emit kernel writes every block's bits at the
// position the chain gave it (one wave per block).  The per-block record KcDfBlock is the only scratch.
#pragma once
#include "kc_dev.h"
#include "kc_s2_dev.h"
#include "kc_wave.h"

#define KCDF_END_CLOSE 0u  // compressor.close: the ten-bit fixed block ends the stream
#define KCDF_END_FLUSH 1u  // compressor.syncFlush: an empty stored block, the stream stays open
// a block's decision (the counters of tests/deflate_model.py)
#define KCDF_NONE 0u        // the record of an empty input: only the stream's end
#define KCDF_QUICK 1u       // stored by the quick check
#define KCDF_EST 2u         // stored by the estimate
#define KCDF_FIRST 3u       // a new table, nothing owed
#define KCDF_REUSE 4u       // the table in force goes on
#define KCDF_NEW_OWED 5u    // EOB of the table in force, then a new table
#define KCDF_F_OWED 1u      // flags: an EOB of prev_table comes first
#define KCDF_F_SYNC 2u      //        the block ends with its EOB
#define KCDF_F_LAST 4u      //        the stream's end follows
#define KCDF_F_NOT_REUSABLE 8u  //    canReuseBits said MaxInt32
#define KCDF_MAX_INPUT ((uint64_t)1 << 30)  // bytes per input this library serves
#define KCDF_GUESS_HEADER_BITS 560

struct KcDfBlock {
    // plan
    uint16_t hist[256];
    uint16_t code[258];     // the block's own table: canonical codes, bit-reversed; [256] EOB
    uint8_t len[260];
    uint8_t codegen[264];   // generateCodegen's sequence, extras in line, n_codegen bytes
    uint16_t cgcode[20];    // the code-length code
    uint8_t cglen[20];
    uint32_t n_codegen, ncg, hdr_bits;
    uint32_t self_bits;     // tmpLitEncoding.canReuseBits(literalFreq[:257]): the block's codes under its own table, EOB included
    uint32_t quick;         // the quick check says stored
    // chain
    uint32_t decision, flags;
    uint32_t table, prev_table;  // records: the table the codes come from; the table an owed EOB comes from
    uint64_t start_bit;     // in the input's DEFLATE stream, of the first bit this block writes (an owed EOB included)
};

struct KcDeflateParams {
    const uint8_t* src;
    const uint64_t* in_off;   // n + 1
    uint32_t n;
    uint32_t gzip, end;       // gzip: header and trailer around; KCDF_END_*
    uint32_t block, penalty;  // the two values compressor.init fixes per level (32768, 10 for HuffmanOnly); block 1 .. 65535
    const uint32_t* blk0;     // n + 1: the first record of every input; every input has at least one record
    const uint32_t* blk_in;   // nblocks: the input of every record
    uint32_t nblocks;
    KcDfBlock* rec;
    uint64_t* size;           // chain: the exact bytes of every input's output
    uint32_t* crc;            // chain, gzip: CRC-32 of every input
    // emit
    const uint64_t* out0;     // where input i's output starts in dst
    uint8_t* dst;             // zeroed over [0, total)
    uint64_t total;
    uint32_t* edge;           // [2], zeroed: what is ORed into the words that hold dst's first and last byte without lying in it
};
void kc_launch_deflate_plan(const KcDeflateParams& P, hipStream_t st);
void kc_launch_deflate_chain(const KcDeflateParams& P, hipStream_t st);
void kc_launch_deflate_emit(const KcDeflateParams& P, hipStream_t st);

__device__ __forceinline__ uint32_t df_reverse(uint32_t code, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; k++) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// what generate needs besides its inputs; one wave.  Sized for the largest alphabet generate is called on: the 286 literal / length
// symbols of kc_flate_stateless.hip (the HuffmanOnly kernels use 257 of them).
struct DfGenLds {
    uint16_t rank[292];
    uint16_t lit[292], frq[292];  // the nodes in order of (freq, literal), maxNode behind them
    int32_t lv[17][4];            // levelInfo: lastFreq, nextCharFreq, nextPairFreq, needed (level is the index)
    int32_t leaf[16][16];         // leafCounts
    int32_t bit_count[16];
    uint32_t next_code[16];
};
#define DF_MAXI32 0x7fffffff

// bitCounts (huffman_code.go:183-309), statement by statement, on ONE lane over LDS; the list has n >= 3 nodes
__device__ __forceinline__ void df_bit_counts(DfGenLds& G, const int32_t n, int32_t maxBits) {
    enum { LAST, NCHAR, NPAIR, NEED };
    G.lit[n] = 0xFFFF; G.frq[n] = 0xFFFF;  // maxNode
    if (maxBits > n - 1) maxBits = n - 1;
    for (int a = 0; a < 17; a++) for (int b = 0; b < 4; b++) G.lv[a][b] = 0;
    for (int a = 0; a < 16; a++) for (int b = 0; b < 16; b++) G.leaf[a][b] = 0;
    const int32_t l2f = G.frq[2], l1f = G.frq[1], l0f = (int32_t)G.frq[0] + (int32_t)G.frq[1];
    for (int32_t level = 1; level <= maxBits; level++) {
        G.lv[level][LAST] = l1f; G.lv[level][NCHAR] = l2f; G.lv[level][NPAIR] = l0f; G.lv[level][NEED] = 0;
        G.leaf[level][level] = 2;
        if (level == 1) G.lv[level][NPAIR] = DF_MAXI32;
    }
    G.lv[maxBits][NEED] = 2 * n - 4;
    int32_t level = maxBits;
    while (level < 16) {  // (ends by the break below: every round takes one of the 2n - 4 items the top level needs, or leaves a level for good)
        int32_t* l = G.lv[level];
        if (l[NPAIR] == DF_MAXI32 && l[NCHAR] == DF_MAXI32) {
            l[NEED] = 0;
            G.lv[level + 1][NPAIR] = DF_MAXI32;
            level++;
            continue;
        }
        const int32_t prevFreq = l[LAST];
        if (l[NCHAR] < l[NPAIR]) {
            const int32_t k = G.leaf[level][level] + 1;
            l[LAST] = l[NCHAR];
            G.leaf[level][level] = k;
            l[NCHAR] = G.lit[k] < 0xFFFF ? (int32_t)G.frq[k] : DF_MAXI32;
        } else {
            l[LAST] = l[NPAIR];
            for (int32_t j = 0; j < 16; j++) if (j != level) G.leaf[level][j] = G.leaf[level - 1][j];
            G.lv[level - 1][NEED] = 2;
        }
        if (--l[NEED] == 0) {
            if (level == maxBits) break;
            G.lv[level + 1][NPAIR] = prevFreq + l[LAST];
            level++;
        } else {
            while (G.lv[level - 1][NEED] > 0) level--;
        }
    }
    for (int b = 0; b < 16; b++) G.bit_count[b] = 0;
    int32_t bits = 1;
    for (int32_t lvl = maxBits; lvl > 0; lvl--) { G.bit_count[bits] = G.leaf[maxBits][lvl] - G.leaf[maxBits][lvl - 1]; bits++; }
}

// huffmanEncoder.generate (huffman_code.go:339-371) over freq[0, nsym) in LDS: lens / codes (bit-reversed) of every symbol.  All
// lanes call; freq must be visible (KC_WAVE_SYNC before), lens / codes are visible on return.  The sort by (freq, literal) is a rank
// sort: the key is a total order, so any sort gives the reference's list.
__device__ __forceinline__ void df_generate(const uint32_t* freq, const int nsym, const int maxBits, DfGenLds& G, uint8_t* lens, uint16_t* codes,
                                            const int lane) {
    uint32_t mine = 0;
    for (int s = lane; s < nsym; s += 64) {
        const uint32_t f = freq[s];
        if (!f) { lens[s] = 0; codes[s] = 0; continue; }
        const uint32_t key = f << 9 | (uint32_t)s;
        uint32_t r = 0;
        for (int t = 0; t < nsym; t++) {
            const uint32_t g = freq[t];
            r += g && (g << 9 | (uint32_t)t) < key;
        }
        G.rank[s] = (uint16_t)r;
        G.lit[r] = (uint16_t)s;
        G.frq[r] = (uint16_t)f;
        mine++;
    }
    const int count = (int)wave_reduce_sum(mine);
    KC_WAVE_SYNC();
    if (count <= 2) {  // everything has one bit, codes in literal order
        if (lane == 0) { for (int b = 0; b < 16; b++) G.bit_count[b] = 0; G.bit_count[1] = count; }
    } else if (lane == 0) {
        df_bit_counts(G, count, maxBits);
    }
    KC_WAVE_SYNC();
    for (int s = lane; s < nsym; s += 64) {  // assignEncodingAndSize: the last bit_count[1] nodes get one bit, the bit_count[2] before them two ...
        if (!freq[s]) continue;
        const int pos = count - 1 - (int)G.rank[s];
        int nb = 1, cum = G.bit_count[1];
        while (pos >= cum && nb < 15) { nb++; cum += G.bit_count[nb]; }
        lens[s] = (uint8_t)nb;
    }
    KC_WAVE_SYNC();
    if (lane == 0) {  // ... and within one length the codes go up in literal order: the canonical code of RFC 1951, 3.2.2
        uint32_t code = 0;
        G.next_code[0] = 0;
        for (int nb = 1; nb < 16; nb++) { code = (code + (uint32_t)G.bit_count[nb - 1]) << 1; G.next_code[nb] = code; }
        for (int s = 0; s < nsym; s++) {
            const uint32_t nb = lens[s];
            if (nb) codes[s] = (uint16_t)df_reverse(G.next_code[nb]++, nb);
        }
    }
    KC_WAVE_SYNC();
}

// generateCodegen (huffman_bit_writer.go:269-348) over lens[0, 257) and the one offset code of length 1 (huffOffset); ONE lane.
// Returns the sequence's bytes; cgfreq[19] are its frequencies.
__device__ __forceinline__ uint32_t df_codegen(const uint8_t* lens, uint8_t* out, uint32_t* cgfreq) {
    for (int k = 0; k < 19; k++) cgfreq[k] = 0;
    auto at = [&](int k) -> uint32_t { return k < 257 ? lens[k] : k == 257 ? 1u : 255u; };
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
__device__ static const uint8_t DF_CODEGEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Bits into dst, least significant first, from any bit position.  dst is zero where nothing was written yet, and words are shared
// between the lanes, the waves and the inputs that meet in them: the first and the last word a sink touches are ORed in (vector
// atomicOr); a word in between belongs to this sink alone and is stored.  The two words that hold dst's first / last bytes without
// lying inside dst are never touched: their bits collect in edge[] and kc_deflate_edges_kernel stores the bytes.
struct DfSink {
    uint32_t* W;        // dst's address rounded down to a word
    uint64_t w;         // the word being filled
    uint64_t acc;
    uint32_t nb;        // bits of acc that are placed (those below the start are zero: another sink's)
    bool live, first;
    uint64_t elo, ehi;  // the edge words' indices (UINT64_MAX: none)
    uint32_t* edge;
};
__device__ __forceinline__ void df_word_or(const DfSink& S, const uint64_t w, const uint32_t v) {
    if (!S.live || !v) return;
    if (w == S.elo) atomicOr(&S.edge[0], v);
    else if (w == S.ehi) atomicOr(&S.edge[1], v);
    else atomicOr(&S.W[w], v);
}
__device__ __forceinline__ void df_seek(DfSink& S, const uint64_t bit) {
    S.w = bit >> 5; S.nb = (uint32_t)(bit & 31); S.acc = 0; S.first = true;
}
__device__ __forceinline__ uint64_t df_tell(const DfSink& S) { return (S.w << 5) + S.nb; }
__device__ __forceinline__ void df_put(DfSink& S, const uint32_t v, const uint32_t n) {  // n <= 32, v < 2^n
    S.acc |= (uint64_t)v << S.nb;
    S.nb += n;
    if (S.nb >= 32) {
        const uint32_t word = (uint32_t)S.acc;
        if (S.first) df_word_or(S, S.w, word);
        else if (S.live) S.W[S.w] = word;
        S.first = false;
        S.acc >>= 32; S.nb -= 32; S.w++;
    }
}
__device__ __forceinline__ void df_pad_to_byte(DfSink& S) { df_put(S, 0, (8 - (S.nb & 7)) & 7); }
__device__ __forceinline__ void df_close(DfSink& S) {  // what is left goes out; the sink stands at the same bit
    if (S.nb) df_word_or(S, S.w, (uint32_t)S.acc);
    S.acc = 0; S.first = true;  // (its bits are out: a sink used on starts like a fresh one here)
}
