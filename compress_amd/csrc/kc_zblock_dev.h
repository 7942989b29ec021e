// kc_zblock_dev.h — the fixed-position fields of a zstd compressed block (blockdec.go:275-345, :505-555), written once for the device
// (the three decoders, through kc_zdec_dev.h) and the host (the stream reader's walk, kc_zdstream_host.h, which sizes a block's slices
// from them; the entropy kernel refuses a block whose record says otherwise).  They read the block's bytes and nothing else.
#pragma once
#include <stdint.h>
#include "kc_kernels.h"

#define ZA_MAX_BLOCK (128u << 10)  // maxCompressedBlockSize: what a block holds and regenerates at most

// The literals header.  comp: the bytes of the literals section behind the header (a raw run: regen, an RLE run: 1).
struct ZdLitHdr {
    int ltype, hdr, comp;
    uint32_t regen;
    bool four;
};
// Reads it from the block b of bn >= 1 bytes.  Returns 0 or the error class (KCZD_*).
__host__ __device__ __attribute__((always_inline)) inline int zd_lit_header(const uint8_t* b, int bn, uint64_t window, ZdLitHdr& h) {
    h.ltype = b[0] & 3;
    const int sf = (b[0] >> 2) & 3;
    const int need = h.ltype < 2 ? ((sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3)) : (sf < 2 ? 3 : (sf == 2 ? 4 : 5));
    if (need > bn) return KCZD_CORRUPT;
    uint64_t v = 0;
    for (int k = 0; k < need; k++) v |= (uint64_t)b[k] << (8 * k);
    h.hdr = need;
    h.four = false;
    if (h.ltype < 2) {
        h.regen = (uint32_t)(v >> ((sf & 1) == 0 ? 3 : 4));
        if (h.regen > ZA_MAX_BLOCK || (uint64_t)h.regen > window) return KCZD_WINDOW;
        h.comp = h.ltype == 0 ? (int)h.regen : 1;
    } else {
        const int bits = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
        h.regen = (uint32_t)(v >> 4) & ((1u << bits) - 1u);
        h.comp = (int)((uint32_t)(v >> (4 + bits)) & ((1u << bits) - 1u));
        h.four = sf != 0;
        if (h.regen > ZA_MAX_BLOCK || (uint64_t)h.regen > window) return KCZD_WINDOW;
    }
    if ((uint64_t)h.hdr + (uint64_t)h.comp > (uint64_t)bn) return KCZD_CORRUPT;
    return 0;
}

// The sequences header behind the literals section: the count and the bytes it takes.  Returns 0 or the error class.
__host__ __device__ __attribute__((always_inline)) inline int zd_seq_count(const uint8_t* sp, int sn, int& nSeq, int& sh) {
    if (sn < 1) return KCZD_CORRUPT;
    nSeq = sp[0];
    sh = 1;
    if (nSeq >= 128) {
        if (nSeq < 255) { if (sn < 2) return KCZD_CORRUPT; nSeq = ((nSeq - 128) << 8) + sp[1]; sh = 2; }
        else { if (sn < 3) return KCZD_CORRUPT; nSeq = sp[1] + (sp[2] << 8) + 0x7F00; sh = 3; }
    }
    return 0;
}

// The compression mode of table `kind` (0 literal lengths, 1 offsets, 2 match lengths) in the modes byte behind the count
__host__ __device__ __attribute__((always_inline)) inline int zd_seq_mode(uint32_t modes, int kind) { return (int)((modes >> (6 - 2 * kind)) & 3u); }
