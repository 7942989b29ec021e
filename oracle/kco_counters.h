// oracle/kco_counters.h — TEST INFRASTRUCTURE ONLY (CPU oracle; see kco_common.h).
// Decision counters of the entropy stage: one fixed array of relaxed atomic counters indexed by an enum, a table of names and
// one C entry (kco_debug_counters, kco_api.cpp) that dumps "name\tcount" lines.  A counter sits where the oracle takes a branch
// of huff0 / fse / blockenc.go whose outcome depends on a histogram and is invisible in the frame header; tests use them to know
// that their inputs reach the branch (tests/test_entropy_decisions.py).  No strings, maps or locks on the encode path: an
// increment is one relaxed fetch_add, placed per block or per symbol of a table, never in a per-input-byte loop.
//
// A name is "<reference file>:<line the oracle cites for the function> <function>: <decision>".  The three sequence coders share
// zstd/fse_encoder.go; their counters carry the coder (ll / of / ml) in front.
#pragma once
#include <atomic>
#include <cstdint>

namespace kco {
namespace ctr {

#define KCO_FSE_CODER_COUNTERS(X, C, c)                                                                  \
    X(C##_TABLELOG_5, c " zstd/fse_encoder.go:429 optimalTableLog: tableLog 5")                         \
    X(C##_TABLELOG_6, c " zstd/fse_encoder.go:429 optimalTableLog: tableLog 6")                         \
    X(C##_TABLELOG_7, c " zstd/fse_encoder.go:429 optimalTableLog: tableLog 7")                         \
    X(C##_TABLELOG_8, c " zstd/fse_encoder.go:429 optimalTableLog: tableLog 8")                         \
    X(C##_USE_RLE, c " zstd/fse_encoder.go:259 normalizeCount: useRLE")                                 \
    X(C##_LOWPROB, c " zstd/fse_encoder.go:259 normalizeCount: -1 (low-probability) symbol")            \
    X(C##_ROUND_UP, c " zstd/fse_encoder.go:259 normalizeCount: small proba rounded up")                \
    X(C##_NC2, c " zstd/fse_encoder.go:334 normalizeCount2: entered")                                   \
    X(C##_NC2_SECOND_PASS, c " zstd/fse_encoder.go:334 normalizeCount2: second lowOne pass")            \
    X(C##_NC2_ALL_SMALL, c " zstd/fse_encoder.go:334 normalizeCount2: all small exit")                  \
    X(C##_NC2_ROUND_ROBIN, c " zstd/fse_encoder.go:334 normalizeCount2: total == 0 round robin")        \
    X(C##_NC2_PROPORTIONAL, c " zstd/fse_encoder.go:334 normalizeCount2: proportional exit")            \
    X(C##_WC_ZERO_RUN_24, c " zstd/fse_encoder.go:488 writeCount: zero run >= 24")                      \
    X(C##_WC_ZERO_RUN_3, c " zstd/fse_encoder.go:488 writeCount: zero run >= 3")                        \
    X(C##_WC_CNT_GE_THRESHOLD, c " zstd/fse_encoder.go:488 writeCount: cnt >= threshold")               \
    X(C##_WC_SHRINK_TWICE, c " zstd/fse_encoder.go:488 writeCount: nbBits shrinks more than once after one symbol")

#define KCO_COUNTERS(X)                                                                                   \
    X(HUF_USE_RLE, "huff0/compress.go:43 compress: ErrUseRLE")                                            \
    X(HUF_INCOMPRESSIBLE_MAXCOUNT, "huff0/compress.go:43 compress: incompressible by maxCount")           \
    X(HUF_REUSE_TAKEN, "huff0/compress.go:43 compress: reuse taken")                                      \
    X(HUF_REUSE_POSSIBLE_NEW_TABLE, "huff0/compress.go:43 compress: reuse possible, new table built")     \
    X(HUF_REUSE_GE_WANTSIZE, "huff0/compress.go:43 compress: reuse taken, then >= wantSize")              \
    X(HUF_NEW_GE_WANTSIZE, "huff0/compress.go:43 compress: new table, then >= wantSize")                  \
    X(HUF_1X, "huff0/compress.go:229 compress1X")                                                         \
    X(HUF_4X, "huff0/compress.go:269 compress4X")                                                         \
    X(HUF_4X_STREAM_TOO_LONG, "huff0/compress.go:269 compress4X: stream above 65535 bytes")               \
    X(HUF_TABLELOG_1, "huff0/compress.go:457 buildCTable: actualTableLog 1")                              \
    X(HUF_TABLELOG_2, "huff0/compress.go:457 buildCTable: actualTableLog 2")                              \
    X(HUF_TABLELOG_3, "huff0/compress.go:457 buildCTable: actualTableLog 3")                              \
    X(HUF_TABLELOG_4, "huff0/compress.go:457 buildCTable: actualTableLog 4")                              \
    X(HUF_TABLELOG_5, "huff0/compress.go:457 buildCTable: actualTableLog 5")                              \
    X(HUF_TABLELOG_6, "huff0/compress.go:457 buildCTable: actualTableLog 6")                              \
    X(HUF_TABLELOG_7, "huff0/compress.go:457 buildCTable: actualTableLog 7")                              \
    X(HUF_TABLELOG_8, "huff0/compress.go:457 buildCTable: actualTableLog 8")                              \
    X(HUF_TABLELOG_9, "huff0/compress.go:457 buildCTable: actualTableLog 9")                              \
    X(HUF_TABLELOG_10, "huff0/compress.go:457 buildCTable: actualTableLog 10")                            \
    X(HUF_TABLELOG_11, "huff0/compress.go:457 buildCTable: actualTableLog 11")                            \
    X(SMH_MAXNBBITS_5, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 5")                        \
    X(SMH_MAXNBBITS_6, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 6")                        \
    X(SMH_MAXNBBITS_7, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 7")                        \
    X(SMH_MAXNBBITS_8, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 8")                        \
    X(SMH_MAXNBBITS_9, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 9")                        \
    X(SMH_MAXNBBITS_10, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 10")                      \
    X(SMH_MAXNBBITS_11, "huff0/compress.go:609 setMaxHeight: entered, maxNbBits 11")                      \
    X(SMH_EXCESS_1, "huff0/compress.go:609 setMaxHeight: excess depth 1")                                 \
    X(SMH_EXCESS_2, "huff0/compress.go:609 setMaxHeight: excess depth 2")                                 \
    X(SMH_EXCESS_3, "huff0/compress.go:609 setMaxHeight: excess depth 3")                                 \
    X(SMH_EXCESS_4UP, "huff0/compress.go:609 setMaxHeight: excess depth >= 4")                            \
    X(SMH_COST_POSITIVE, "huff0/compress.go:609 setMaxHeight: totalCost > 0 loop")                        \
    X(SMH_BREAK_LOW_EMPTY, "huff0/compress.go:609 setMaxHeight: inner for, break on lowPos == noSymbol")  \
    X(SMH_BREAK_HIGH_LE_LOW, "huff0/compress.go:609 setMaxHeight: inner for, break on highTotal <= lowTotal") \
    X(SMH_SKIP_EMPTY_RANKS, "huff0/compress.go:609 setMaxHeight: upward skip over empty ranks")           \
    X(SMH_SEED_LOWER_RANK, "huff0/compress.go:609 setMaxHeight: lower rank seeded (rankLast[n-1] == noSymbol)") \
    X(SMH_RANK_LAST_IS_0, "huff0/compress.go:609 setMaxHeight: the rank's last position is 0")            \
    X(SMH_RANK_EMPTIED, "huff0/compress.go:609 setMaxHeight: rank emptied by the nBits mismatch")         \
    X(SMH_COST_NEGATIVE, "huff0/compress.go:609 setMaxHeight: totalCost < 0 loop")                        \
    X(SMH_REPAY_RANK1_UNSET, "huff0/compress.go:609 setMaxHeight: repay, rankLast[1] == noSymbol")        \
    X(SMH_REPAY_RANK1_SET, "huff0/compress.go:609 setMaxHeight: repay, rankLast[1] set")                  \
    X(HWT_MAXSYM_LT_2, "huff0/huff0.go:180 cTable.write: maxSym < 2")                                     \
    X(HWT_FSE_USED, "huff0/huff0.go:180 cTable.write: FSE of the weights used")                           \
    X(HWT_FSE_NOT_SMALLER, "huff0/huff0.go:180 cTable.write: FSE succeeded but was not smaller")          \
    X(HWT_FSE_USE_RLE, "huff0/huff0.go:180 cTable.write: FSE returned ErrUseRLE")                         \
    X(HWT_FSE_INCOMPRESSIBLE_MAXCOUNT, "huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by maxCount (fse/compress.go:18)") \
    X(HWT_FSE_INCOMPRESSIBLE_SIZE, "huff0/huff0.go:180 cTable.write: FSE ErrIncompressible by output size (fse/compress.go:18)") \
    X(HWT_RAW_EVEN, "huff0/huff0.go:180 cTable.write: raw 4-bit weights, even maxSym")                    \
    X(HWT_RAW_ODD, "huff0/huff0.go:180 cTable.write: raw 4-bit weights, odd maxSym")                      \
    X(HWT_OVER_128_SYMBOLS, "huff0/huff0.go:180 cTable.write: more than 128 symbols, ErrIncompressible")  \
    X(FSEB_NC2, "fse/compress.go:557 normalizeCount2: entered")                                           \
    X(FSEB_NC2_SECOND_PASS, "fse/compress.go:557 normalizeCount2: second lowOne pass")                    \
    X(FSEB_NC2_ALL_SMALL, "fse/compress.go:557 normalizeCount2: all small exit")                          \
    X(FSEB_NC2_ROUND_ROBIN, "fse/compress.go:557 normalizeCount2: total == 0 round robin")                \
    X(FSEB_NC2_PROPORTIONAL, "fse/compress.go:557 normalizeCount2: proportional exit")                    \
    X(BLK_LITS_16_NONE, "zstd/blockenc.go:337,481 literals: 16 literals, no entropy coder")               \
    X(BLK_LITS_17_1X, "zstd/blockenc.go:337,481 literals: 17 literals, 1X")                               \
    X(BLK_LITS_1023_1X, "zstd/blockenc.go:337,481 literals: 1023 literals, 1X")                           \
    X(BLK_LITS_1024_4X, "zstd/blockenc.go:337,481 literals: 1024 literals, 4X")                           \
    X(ENCLITS_LT_8, "zstd/blockenc.go:337 encodeLits: n < 8")                                             \
    X(ENCLITS_LT_32_NO_DICT, "zstd/blockenc.go:337 encodeLits: n < 32 without a dictionary table")        \
    X(ENCLITS_NOT_SMALLER, "zstd/blockenc.go:337 encodeLits: compressed no smaller than raw with both headers") \
    X(ENCODE_NOT_SMALLER, "zstd/blockenc.go:481 encode: compressed no smaller than raw with both headers") \
    X(LH_RAW_1, "zstd/blockenc.go:150 literalsHeader.setSize: raw, 1 byte")                               \
    X(LH_RAW_2, "zstd/blockenc.go:150 literalsHeader.setSize: raw, 2 bytes")                              \
    X(LH_RAW_3, "zstd/blockenc.go:150 literalsHeader.setSize: raw, 3 bytes")                              \
    X(LH_RLE_1, "zstd/blockenc.go:150 literalsHeader.setSize: RLE, 1 byte")                               \
    X(LH_RLE_2, "zstd/blockenc.go:150 literalsHeader.setSize: RLE, 2 bytes")                              \
    X(LH_RLE_3, "zstd/blockenc.go:150 literalsHeader.setSize: RLE, 3 bytes")                              \
    X(LH_COMP_3, "zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 3 bytes")                     \
    X(LH_COMP_4, "zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 4 bytes")                     \
    X(LH_COMP_5, "zstd/blockenc.go:178 literalsHeader.setSizes: compressed, 5 bytes")                     \
    X(ENCODE_SAVED_LT_16, "zstd/blockenc.go:481 encode: saved < 16")                                      \
    X(ENCODE_SINGLE_SEQ_RLE, "zstd/blockenc.go:481 encode: single-sequence RLE block")                    \
    KCO_FSE_CODER_COUNTERS(X, LL, "ll")                                                                   \
    KCO_FSE_CODER_COUNTERS(X, OF, "of")                                                                   \
    KCO_FSE_CODER_COUNTERS(X, ML, "ml")                                                                   \
    X(GC_LL_MAX_LT_16, "zstd/blockenc.go:831 genCodes: highest LL code < 16")                             \
    X(GC_LL_MAX_16_24, "zstd/blockenc.go:831 genCodes: highest LL code 16..24")                           \
    X(GC_LL_MAX_GE_25, "zstd/blockenc.go:831 genCodes: highest LL code >= 25")                            \
    X(GC_LL_MAX_TOP, "zstd/blockenc.go:831 genCodes: highest LL code 35 (top)")                           \
    X(GC_ML_MAX_LT_32, "zstd/blockenc.go:831 genCodes: highest ML code < 32")                             \
    X(GC_ML_MAX_32_42, "zstd/blockenc.go:831 genCodes: highest ML code 32..42")                           \
    X(GC_ML_MAX_GE_43, "zstd/blockenc.go:831 genCodes: highest ML code >= 43")                            \
    X(GC_ML_MAX_TOP, "zstd/blockenc.go:831 genCodes: highest ML code 52 (top)")                           \
    X(GC_OF_MAX_LT_8, "zstd/blockenc.go:831 genCodes: highest OF code < 8")                               \
    X(GC_OF_MAX_8_15, "zstd/blockenc.go:831 genCodes: highest OF code 8..15")                             \
    X(GC_OF_MAX_GE_16, "zstd/blockenc.go:831 genCodes: highest OF code >= 16")                            \
    X(GC_OF_MAX_TOP, "zstd/blockenc.go:831 genCodes: highest OF code 30 (top)")                           \
    X(GC_NSEQ_127, "zstd/blockenc.go:481 encode: nSeq exactly 127")                                       \
    X(GC_NSEQ_128, "zstd/blockenc.go:481 encode: nSeq exactly 128")

enum Id {
#define X(id, name) id,
    KCO_COUNTERS(X)
#undef X
    COUNT
};

// per-coder counters: base of the coder's group + offset within the group
enum Coder { LL = LL_TABLELOG_5, OF = OF_TABLELOG_5, ML = ML_TABLELOG_5, NONE = -1 };
enum CoderOff {
    TABLELOG_5 = 0, USE_RLE = 4, LOWPROB, ROUND_UP, NC2, NC2_SECOND_PASS, NC2_ALL_SMALL, NC2_ROUND_ROBIN, NC2_PROPORTIONAL,
    WC_ZERO_RUN_24, WC_ZERO_RUN_3, WC_CNT_GE_THRESHOLD, WC_SHRINK_TWICE
};

// CoderOff restates the order of KCO_FSE_CODER_COUNTERS, and the three groups are laid out alike
static_assert(LL + TABLELOG_5 + 3 == LL_TABLELOG_8 && LL + USE_RLE == LL_USE_RLE && LL + LOWPROB == LL_LOWPROB && LL + ROUND_UP == LL_ROUND_UP &&
              LL + NC2 == LL_NC2 && LL + NC2_SECOND_PASS == LL_NC2_SECOND_PASS && LL + NC2_ALL_SMALL == LL_NC2_ALL_SMALL &&
              LL + NC2_ROUND_ROBIN == LL_NC2_ROUND_ROBIN && LL + NC2_PROPORTIONAL == LL_NC2_PROPORTIONAL &&
              LL + WC_ZERO_RUN_24 == LL_WC_ZERO_RUN_24 && LL + WC_ZERO_RUN_3 == LL_WC_ZERO_RUN_3 &&
              LL + WC_CNT_GE_THRESHOLD == LL_WC_CNT_GE_THRESHOLD && LL + WC_SHRINK_TWICE == LL_WC_SHRINK_TWICE, "CoderOff out of step with the macro");
static_assert(OF + WC_SHRINK_TWICE == OF_WC_SHRINK_TWICE && ML + WC_SHRINK_TWICE == ML_WC_SHRINK_TWICE && (int)OF - (int)LL == (int)ML - (int)OF,
              "the three coders' groups differ");

inline std::atomic<uint64_t> g_table[COUNT];
inline std::atomic<uint64_t>* table() { return g_table; }
inline const char* const* names() {
    static const char* const n[COUNT] = {
#define X(id, name) name,
        KCO_COUNTERS(X)
#undef X
    };
    return n;
}
static inline void hit(int id) { table()[id].fetch_add(1, std::memory_order_relaxed); }
// a counter of a sequence coder; coder == NONE (an encoder that is none of a block's three) counts nothing
static inline void hitc(int coder, int off) { if (coder >= 0) hit(coder + off); }

}  // namespace ctr
}  // namespace kco
