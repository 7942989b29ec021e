#pragma once
// kc_zdec_host.h — host logic of zstd.Decoder.DecodeAll that needs no device: what becomes of an input once its frames have been
// decoded (kc_zstd_dec_api.cpp; the wave emulator's wrapper tools/hipemu/kcemu.cpp runs the same kernels and settles them the same way).
#include <stdint.h>
#include "kc_kernels.h"

// One input after the decode kernel, frame by frame in the order the reference meets them (zstd/decoder.go:342-408): the size limit
// against what the input has produced so far (exact only now, when an earlier frame carried no content size), the frame's own
// error, its checksum (hash[2 * f] = XXH64 of its decoded bytes), the running total.  Returns the input's status; *total = its
// decoded bytes when that is 0.
static inline uint32_t kc_zd_settle_input(const KcZdFrame* fr, const uint32_t* fstatus, const uint32_t* fsize, const uint32_t* crc_stored,
                                          const uint64_t* hash, uint32_t nf, uint64_t max_memory, bool ignore_checksum, uint64_t* total) {
    uint64_t produced = 0;
    for (uint32_t f = 0; f < nf; f++) {
        if (fr[f].fcs != KC_ZD_NO_SIZE && fr[f].fcs > max_memory - produced) return KCZD_SIZE;
        if (fstatus[f]) return fstatus[f];
        if (fr[f].checksum && !ignore_checksum && (uint32_t)hash[2 * (size_t)f] != crc_stored[f]) return KCZD_CRC;
        produced += fsize[f];
        if (produced > max_memory) return KCZD_SIZE;
    }
    *total = produced;
    return KCZD_OK;
}
