// kc_zstd_decode.hip — zstd frame decoder on the device: the verifier half of SURVEY.md §8f N1 for zstd
// (zstd/framedec.go:65-330 -> blockdec.go:227-690 -> seqdec_generic.go:16,161, fse_decoder.go, huff0/decompress.go).
// One wave per frame, whose decoded length is given.  The compressed-block parser is the shared one (kc_zdec_dev.h: serial format
// parsing on lane 0 with the tables in LDS, Huffman streams on one lane per stream); what is the verifier's own is the frame header,
// the given length as the bound of every write, a repeat offset that resolves to 0 refused instead of forced to 1, and the in-order
// copy loop: literal and match copies use all 64 lanes, one sequence after the other.  Raw-content dictionaries are supported as
// history; dictionary entropy tables are not (status 8 / 12).  Not a throughput kernel: it exists so that a device-resident encode
// can be verified (decode + XXH64 compare) without leaving the GPU.
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_zdec_dev.h"

__global__ __launch_bounds__(64) void kc_zstd_decode_kernel(KcZstdDecParams P) {
    __shared__ ZdShared S;
    const int lane = (int)threadIdx.x;
    const uint32_t u = blockIdx.x;
    if (u >= P.n_units) return;
    const uint8_t* __restrict__ in = P.enc + P.enc_off[u];
    const int n = (int)(P.enc_off[u + 1] - P.enc_off[u]);
    uint8_t* __restrict__ out = P.dst + P.dst_off[u];
    const uint64_t want = P.dst_off[u + 1] - P.dst_off[u];
    uint8_t* __restrict__ lits = P.lits + (size_t)u * P.lit_stride;
    if (lane < 16) S.iv[lane] = 0;
    KC_WAVE_SYNC();
    int err = 0;
    int p = 0;
    bool checksum = false;
    // ---- frame header (framedec.go:65-200), identical on all lanes ----
    if (n == 0) {  // nothing was emitted for an empty unit (WithZeroFrames(false))
        if (lane == 0) { P.status[u] = want == 0 ? 0u : 2u; P.crc_stored[u] = 0xFFFFFFFFu; P.has_crc[u] = 0u; }
        return;
    }
    if (n < 6 || ld32(in) != 0xFD2FB528u) err = 1;
    uint64_t fcs = 0, window = 0;
    int fcsSize = 0;
    if (!err) {
        const uint8_t fhd = in[4];
        p = 5;
        const bool single = (fhd >> 5) & 1;
        checksum = (fhd >> 2) & 1;
        if (fhd & 8) err = 1;
        if (!single) {  // Window_Descriptor (n >= 6: in[5] is there)
            const uint32_t wd = in[p++];
            const uint64_t base = (uint64_t)1 << (10 + (wd >> 3));
            window = base + (base / 8) * (wd & 7u);
            if (window > ((uint64_t)1 << 29)) err = 1;  // above the reference decoder's maximum (ErrWindowSizeExceeded)
        }
        const int dsz = (fhd & 3) == 3 ? 4 : (fhd & 3);
        if (dsz && P.dict == nullptr) err = 20;  // a dictionary frame needs the dictionary content (raw content only: no entropy tables)
        p += dsz;
        fcsSize = (fhd >> 6) == 0 ? (single ? 1 : 0) : (1 << (fhd >> 6));
        if (p + fcsSize > n) err = 1;
        else {
            for (int k = 0; k < fcsSize; k++) fcs |= (uint64_t)in[p + k] << (8 * k);
            if (fcsSize == 2) fcs += 256;
            p += fcsSize;
        }
        if (single) window = fcs > 1024 ? fcs : 1024;
        if (!err && fcsSize > 0 && fcs != want) err = 2;
    }
    uint64_t d = 0;  // bytes produced
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;
    bool last = false;
    while (!err && !last) {
        if (p + 3 > n) { err = 3; break; }
        const uint32_t bh = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
        p += 3;
        last = bh & 1;
        const int type = (bh >> 1) & 3;
        const int size = (int)(bh >> 3);
        if (type == 0) {  // raw
            if (p + size > n || d + (uint64_t)size > want) { err = 4; break; }
            for (int k = lane; k < size; k += 64) out[d + k] = in[p + k];
            d += (uint64_t)size; p += size;
            continue;
        }
        if (type == 1) {  // RLE
            if (p + 1 > n || d + (uint64_t)size > want) { err = 4; break; }
            const uint8_t v = in[p];
            for (int k = lane; k < size; k += 64) out[d + k] = v;
            d += (uint64_t)size; p += 1;
            continue;
        }
        if (type == 3 || p + size > n || size > (128 << 10)) { err = 5; break; }
        // ================= compressed block =================
        const uint8_t* b = in + p;
        const int bn = size;
        p += size;
        // ---- literals section (blockdec.go:275-460) ----
        if (bn < 2) { err = 6; break; }  // ErrBlockTooSmall (blockdec.go:233): nothing below is read past the block
        ZdLitHdr h;
        if (zd_lit_header(b, bn, window, h) || h.regen > P.lit_stride) { err = 6; break; }
        const int regen = (int)h.regen;
        const uint8_t* L = b + h.hdr;  // where the literals of this block can be read
        const int litRle = h.ltype == 1 ? (int)b[h.hdr] : -1;
        if (h.ltype >= 2) {
            const uint8_t* q = b + h.hdr;
            int left = h.comp;
            if (h.ltype == 2) {
                const int used = zd_huf_table(q, left, S, lane, lits, P.lit_stride);
                if (used < 0) { err = 7; break; }
                q += used; left -= used;
            } else if (!S.iv[V_HUFOK]) { err = 8; break; }
            if (zd_huf_streams(q, left, h.four, h.regen, S, lane, lits)) { err = 10; break; }
            L = lits;
        }
        // ---- sequences section (blockdec.go:505-690) ----
        const uint8_t* sp = b + h.hdr + h.comp;
        int sn = bn - h.hdr - h.comp;
        int nSeq = 0, sh = 0;
        if (zd_seq_count(sp, sn, nSeq, sh)) { err = 11; break; }
        sp += sh; sn -= sh;
        if (nSeq == 0) {
            if (sn != 0 || d + (uint64_t)regen > want) { err = 11; break; }
            if (litRle >= 0) { for (int k = lane; k < regen; k += 64) out[d + k] = (uint8_t)litRle; }
            else { for (int k = lane; k < regen; k += 64) out[d + k] = L[k]; }
            d += (uint64_t)regen;
            KC_WAVE_SYNC();
            continue;
        }
        {
            const int used = zd_seq_tables(sp, sn, S, lane);
            if (used < 0) { err = 12; break; }
            sp += used; sn -= used;
        }
        // decode 64 sequences on lane 0, then execute them on all lanes (seqdec_generic.go)
        ZdSeqDec sq;
        if (zd_seq_open(sq, sp, sn, S, lane)) { err = 13; break; }
        int lp = 0;  // literals consumed
        for (int s0 = 0; s0 < nSeq && !err; s0 += 64) {
            const int cnt = nSeq - s0 < 64 ? nSeq - s0 : 64;
            // a repeat offset that resolves to 0 is refused here (the product path forces it to 1 as the reference does)
            const int e2 = zd_seq_group(sq, S, lane, s0, cnt, nSeq, [&](uint32_t ofVal, uint32_t llen, uint32_t& off) {
                off = zd_rep_offset(ofVal, llen, rep0, rep1, rep2);
                return off != 0;
            });
            if (e2) { err = e2 == KCZD_EOF ? 16 : 14; break; }
            for (int i = 0; i < cnt; i++) {
                const uint32_t llen = S.seqLL[i], mlen = S.seqML[i], off = S.seqOF[i];
                if ((uint64_t)lp + llen > (uint64_t)regen || d + llen + mlen > want || (uint64_t)off > d + llen + P.dict_len) { err = 18; break; }
                if (litRle >= 0) { for (uint32_t k = (uint32_t)lane; k < llen; k += 64) out[d + k] = (uint8_t)litRle; }
                else { for (uint32_t k = (uint32_t)lane; k < llen; k += 64) out[d + k] = L[lp + k]; }
                lp += (int)llen;
                d += llen;
                KC_WAVE_SYNC();
                if ((uint64_t)off > d) {  // the match starts in the dictionary (history in front of the frame, dict.go / history.go)
                    const uint32_t inDict = (uint32_t)((uint64_t)off - d);  // bytes of the match source that lie in the dictionary
                    for (uint32_t k = (uint32_t)lane; k < mlen; k += 64) {
                        const uint32_t j = off >= mlen ? k : k % off;  // an overlapping match repeats its first `off` bytes
                        out[d + k] = j < inDict ? P.dict[P.dict_len - inDict + j] : out[j - inDict];
                    }
                } else if (off >= mlen) { for (uint32_t k = (uint32_t)lane; k < mlen; k += 64) out[d + k] = out[d - off + k]; }
                else { for (uint32_t k = (uint32_t)lane; k < mlen; k += 64) out[d + k] = out[d - off + (k % off)]; }
                d += mlen;
                KC_WAVE_SYNC();
            }
        }
        if (err) break;
        // trailing literals
        const int tail = regen - lp;
        if (d + (uint64_t)tail > want) { err = 18; break; }
        if (litRle >= 0) { for (int k = lane; k < tail; k += 64) out[d + k] = (uint8_t)litRle; }
        else { for (int k = lane; k < tail; k += 64) out[d + k] = L[lp + k]; }
        d += (uint64_t)tail;
        KC_WAVE_SYNC();
    }
    if (!err && d != want) err = 2;
    uint32_t stored = 0xFFFFFFFFu;
    if (!err && checksum) {
        if (p + 4 > n) err = 19;
        else { stored = ld32(in + p); p += 4; }
    }
    if (!err && p != n) err = 19;  // one frame per unit
    if (lane == 0) { P.status[u] = (uint32_t)err; P.crc_stored[u] = (!err && checksum) ? stored : 0xFFFFFFFFu; P.has_crc[u] = (!err && checksum) ? 1u : 0u; }
}

void kc_launch_zstd_decode(const KcZstdDecParams& P, hipStream_t st) {
    if (P.n_units == 0) return;
    hipLaunchKernelGGL(kc_zstd_decode_kernel, dim3(P.n_units), dim3(64), 0, st, P);
}
