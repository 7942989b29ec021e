// kc_zexec_dev.h — device code shared by the zstd decoders that execute sequences in groups of 64: DecodeAll (kc_zstd_decode_all.hip)
// and the stream reader (kc_zstd_dstream.hip): what a frame sees behind it, a block's literals, and the group executor.  (The block
// parser in front of it is kc_zdec_dev.h, which the verifier shares; the verifier executes its sequences one after the other.)
#pragma once
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zdec_dev.h"

namespace {

#define ZA_SHORT 32u  // copies up to this many bytes are made by the sequence's own lane, longer ones by the whole wave

// what the frame sees behind it: the dictionary's content (if any) in front of its own output
struct ZaHist {
    uint8_t* out;
    const uint8_t* dict;
    uint32_t dict_len;
    __device__ __forceinline__ uint8_t at(int64_t q) const { return q < 0 ? dict[(int64_t)dict_len + q] : out[q]; }
};

// The literals of one block: a run of one byte value (rle >= 0) or bytes at L
struct ZaLits {
    const uint8_t* L;
    int rle;
    __device__ __forceinline__ uint8_t at(uint32_t k) const { return rle >= 0 ? (uint8_t)rle : L[k]; }
};

// Executes `cnt` decoded sequences (S.seqLL / seqML / seqOF, one per lane) at output position d, literal position lp.
//   * every lane gets the output position of its sequence by a wave prefix sum over ll + ml;
//   * all literal runs, and every match whose source ends in front of the group's first output byte, are copied at once — short
//     ones by their own lane, long ones by the whole wave;
//   * the remaining matches follow in order, each by the whole wave.
// All checks come first: a group that fails writes nothing.  Returns 0 or the error class; d and lp advance on success.
__device__ int za_execute_group(ZdShared& S, int cnt, int lane, const ZaHist& H, const ZaLits& LT, uint64_t& d, uint32_t& lp, uint32_t regen,
                                uint64_t cap, uint64_t blockStart, uint64_t blockMax, uint64_t window, int capClass) {
    const uint32_t myLL = lane < cnt ? S.seqLL[lane] : 0u, myML = lane < cnt ? S.seqML[lane] : 0u, myOF = lane < cnt ? S.seqOF[lane] : 1u;
    KC_EMU_SYNC();  // (lane 0 refills the three arrays for the next group)
    const uint32_t tot = myLL + myML;
    const uint32_t incT = wave_incl_scan(tot, lane), incL = wave_incl_scan(myLL, lane);
    const uint32_t gTot = rdlane32(incT, 63), gLit = rdlane32(incL, 63);
    const uint64_t o0 = d + (incT - tot);      // my literals go here
    const uint64_t m0 = o0 + myLL;             // my match goes here
    const uint32_t l0 = lp + (incL - myLL);    // my first literal
    int bad = 0;
    if ((uint64_t)lp + gLit > (uint64_t)regen) bad = KCZD_CORRUPT;                       // "unexpected literal count"
    else if ((d - blockStart) + gTot > blockMax) bad = KCZD_CORRUPT;                     // "output bigger than max block size"
    else if (d + gTot > cap) bad = capClass;
    // "match offset bigger than current history": beyond the frame's output plus the dictionary, or beyond the window while still
    // inside the output (an offset that reaches into the dictionary is not held to the window: seqdec.go:345-364)
    const bool offBad = lane < cnt && ((uint64_t)myOF > m0 + H.dict_len || ((uint64_t)myOF > window && (uint64_t)myOF <= m0));
    if (ballot64(offBad)) bad = bad ? bad : KCZD_CORRUPT;
    if (bad) return bad;
    const int64_t src0 = (int64_t)m0 - (int64_t)myOF;  // my match's source (negative: in the dictionary)
    const bool indep = lane < cnt && src0 + (int64_t)myML <= (int64_t)d;
    if (lane < cnt) {
        if (myLL <= ZA_SHORT) for (uint32_t k = 0; k < myLL; k++) H.out[o0 + k] = LT.at(l0 + k);
        if (indep && myML <= ZA_SHORT) for (uint32_t k = 0; k < myML; k++) H.out[m0 + k] = H.at(src0 + k);
    }
    for (uint64_t m = ballot64(lane < cnt && myLL > ZA_SHORT); m; m &= m - 1) {
        const int s = ctz64(m);
        const uint32_t n = rdlane32(myLL, s), src = rdlane32(l0, s);
        const uint64_t dst = rdlane64(o0, s);
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) H.out[dst + k] = LT.at(src + k);
    }
    for (uint64_t m = ballot64(indep && myML > ZA_SHORT); m; m &= m - 1) {
        const int s = ctz64(m);
        const uint32_t n = rdlane32(myML, s);
        const uint64_t dst = rdlane64(m0, s);
        const int64_t src = (int64_t)rdlane64((uint64_t)src0, s);
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) H.out[dst + k] = H.at(src + k);
    }
    KC_WAVE_SYNC();
    for (uint64_t m = ballot64(lane < cnt && !indep && myML > 0); m; m &= m - 1) {
        const int s = ctz64(m);
        const uint32_t n = rdlane32(myML, s), off = rdlane32(myOF, s);
        const uint64_t dst = rdlane64(m0, s);
        const int64_t src = (int64_t)dst - (int64_t)off;
        // an overlapping match repeats its first `off` bytes, which lie in front of it
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) H.out[dst + k] = H.at(src + (off >= n ? k : k % off));
        KC_WAVE_SYNC();
    }
    d += gTot;
    lp += gLit;
    return 0;
}

}  // namespace
