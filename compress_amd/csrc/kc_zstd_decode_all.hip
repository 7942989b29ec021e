// kc_zstd_decode_all.hip — zstd.Decoder.DecodeAll on the device as a product path (zstd/decoder.go:319-410 -> framedec.go:330-412 ->
// blockdec.go:227-650 -> seqdec.go:221-434, fse_decoder.go, huff0/decompress.go).  One wave per FRAME of the plan
// (kc_zstd_plan.hip): the frame decodes into its staging slot, from where the host compacts the inputs' frames into the dense
// output.  Unlike the verifier (kc_zstd_decode.hip) the kernel knows no decoded length, takes the dictionary the frame's id names
// — content as history, and for full-format dictionaries the repeat offsets and the Huffman / FSE tables as the "previous" tables
// of the first block —, checks offsets against the window and the block against min(window, 128 KiB) as the reference does, and
// executes a decoded group of 64 sequences together instead of one after the other (za_execute_group).  The compressed-block parser
// is the one all three decoders share (kc_zdec_dev.h); what is this kernel's own is the plan's frame record, the staging slot, the
// dictionary's tables in front of the first block and the group executor.
// Untrusted input: every read is checked against the frame's block range, every write against the frame's slot.
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zdec_dev.h"
#include "kc_zexec_dev.h"

__global__ __launch_bounds__(64) void kc_zstd_decode_all_kernel(KcZdDecodeParams P) {
    __shared__ ZdShared S;
    const int lane = (int)threadIdx.x;
    const uint32_t f = blockIdx.x;
    if (f >= P.n_frames) return;
    const KcZdFrame F = P.frames[f];
    const uint8_t* __restrict__ in = P.src;
    const uint64_t cap = F.slot_cap;
    // a frame that outgrows a slot cut to the size limit has exceeded that limit; any other slot is the frame's own promise
    const int capClass = (F.fcs == KC_ZD_NO_SIZE && cap == P.max_memory) ? KCZD_SIZE : KCZD_CORRUPT;
    uint8_t* __restrict__ lits = P.lits + (size_t)f * KC_ZD_LIT_STRIDE;
    ZaHist H;
    H.out = P.stage + F.slot_off;
    H.dict = nullptr;
    H.dict_len = 0;
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;
    if (lane < 16) S.iv[lane] = 0;
    KC_WAVE_SYNC();
    if (F.dict) {
        const KcZdDict* __restrict__ D = P.dicts + (F.dict - 1);
        H.dict = P.dict_arena + D->content_off;
        H.dict_len = D->content_len;
        rep0 = D->rep[0]; rep1 = D->rep[1]; rep2 = D->rep[2];
        if (D->full) {  // the dictionary's tables are the "previous" tables of the first block (history.setDict)
            for (int k = lane; k < (1 << 11); k += 64) S.huf[k] = D->huf[k];
            zd_cells_in(S.ll, D->ll, 1 << 9, lane);
            zd_cells_in(S.of, D->of, 1 << 8, lane);
            zd_cells_in(S.ml, D->ml, 1 << 9, lane);
            if (lane == 0) {
                S.iv[V_HUFLOG] = D->huf_log; S.iv[V_HUFOK] = 1;
                S.iv[V_LLLOG] = D->ll_log; S.iv[V_OFLOG] = D->of_log; S.iv[V_MLLOG] = D->ml_log;
                S.iv[V_LLOK] = 1; S.iv[V_OFOK] = 1; S.iv[V_MLOK] = 1;
            }
        }
        KC_WAVE_SYNC();
    }
    const uint64_t blockMax = F.window < ZA_MAX_BLOCK ? F.window : (uint64_t)ZA_MAX_BLOCK;
    int err = 0;
    uint64_t p = F.blk_begin;
    const uint64_t pend = F.blk_end;
    uint64_t d = 0;  // bytes produced
    bool last = false;
    while (!err && !last) {
        if (pend - p < 3) { err = KCZD_EOF; break; }
        const uint32_t bh = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
        p += 3;
        last = bh & 1;
        const int type = (bh >> 1) & 3;
        const uint32_t size = bh >> 3;
        if (type == 0 || type == 1) {  // raw, RLE
            const uint32_t have = type == 0 ? size : 1u;
            if (size > ZA_MAX_BLOCK || (uint64_t)size > F.window) { err = KCZD_WINDOW; break; }
            if (pend - p < have) { err = KCZD_EOF; break; }
            if (d + size > cap) { err = capClass; break; }
            if (type == 0) { for (uint32_t k = (uint32_t)lane; k < size; k += 64) H.out[d + k] = in[p + k]; }
            else { const uint8_t v = in[p]; for (uint32_t k = (uint32_t)lane; k < size; k += 64) H.out[d + k] = v; }
            d += size; p += have;
            KC_WAVE_SYNC();
            continue;
        }
        if (type == 3 || size > ZA_MAX_BLOCK || (uint64_t)size > F.window || size < 2) { err = KCZD_CORRUPT; break; }
        if (pend - p < size) { err = KCZD_EOF; break; }
        // ================= compressed block =================
        const uint8_t* __restrict__ b = in + p;
        const int bn = (int)size;
        p += size;
        const uint64_t blockStart = d;
        // ---- literals section (blockdec.go:275-474) ----
        ZdLitHdr h;
        if ((err = zd_lit_header(b, bn, F.window, h)) != 0) break;
        const uint32_t regen = h.regen;
        ZaLits LT;
        LT.L = b + h.hdr;
        LT.rle = h.ltype == 1 ? (int)b[h.hdr] : -1;
        if (h.ltype >= 2) {
            const uint8_t* q = b + h.hdr;
            int left = h.comp;
            if (h.ltype == 2) {
                const int used = zd_huf_table(q, left, S, lane, lits, KC_ZD_LIT_STRIDE);
                if (used < 0) { err = KCZD_CORRUPT; break; }
                q += used; left -= used;
            } else if (!S.iv[V_HUFOK]) { err = KCZD_CORRUPT; break; }  // "literal block was treeless, but no history was defined"
            if ((err = zd_huf_streams(q, left, h.four, regen, S, lane, lits)) != 0) break;
            LT.L = lits;
        }
        // ---- sequences section (blockdec.go:505-650) ----
        const uint8_t* sp = b + h.hdr + h.comp;
        int sn = bn - h.hdr - h.comp;
        int nSeq = 0, sh = 0;
        if ((err = zd_seq_count(sp, sn, nSeq, sh)) != 0) break;
        sp += sh; sn -= sh;
        if (nSeq == 0) {
            if (sn != 0) { err = KCZD_CORRUPT; break; }
            if (d + regen > cap) { err = capClass; break; }
            for (uint32_t k = (uint32_t)lane; k < regen; k += 64) H.out[d + k] = LT.at(k);
            d += regen;
            KC_WAVE_SYNC();
            continue;
        }
        {
            const int used = zd_seq_tables(sp, sn, S, lane);
            if (used < 0) { err = KCZD_CORRUPT; break; }
            sp += used; sn -= used;
        }
        // decode 64 sequences on lane 0, then execute them on all lanes (seqdec.go:221-434)
        ZdSeqDec sq;
        if ((err = zd_seq_open(sq, sp, sn, S, lane)) != 0) break;
        uint32_t lp = 0;  // literals consumed
        for (int s0 = 0; s0 < nSeq && !err; s0 += 64) {
            const int cnt = nSeq - s0 < 64 ? nSeq - s0 : 64;
            err = zd_seq_group(sq, S, lane, s0, cnt, nSeq, [&](uint32_t ofVal, uint32_t llen, uint32_t& off) {
                off = zd_rep_offset(ofVal, llen, rep0, rep1, rep2);
                if (off == 0) off = rep0 = 1;  // "0 is not valid; input is corrupted; force offset to 1" (seqdec.go:288-292)
                return true;
            });
            if (err) break;
            err = za_execute_group(S, cnt, lane, H, LT, d, lp, regen, cap, blockStart, blockMax, F.window, capClass);
        }
        if (err) break;
        // trailing literals
        const uint32_t tail = regen - lp;
        if ((d - blockStart) + tail > blockMax) { err = KCZD_CORRUPT; break; }
        if (d + tail > cap) { err = capClass; break; }
        for (uint32_t k = (uint32_t)lane; k < tail; k += 64) H.out[d + k] = LT.at(lp + k);
        d += tail;
        KC_WAVE_SYNC();
    }
    if (!err && F.fcs != KC_ZD_NO_SIZE && d != F.fcs) err = KCZD_CORRUPT;  // ErrFrameSizeMismatch
    if (lane == 0) {
        const uint32_t got = err ? 0u : (uint32_t)d;
        P.status[f] = (uint32_t)err;
        P.out_size[f] = got;
        P.crc_stored[f] = F.checksum ? ld32(in + F.blk_end) : 0u;
        P.hash_off[2 * (size_t)f] = F.slot_off;
        P.hash_off[2 * (size_t)f + 1] = F.slot_off + got;
    }
}

void kc_launch_zstd_decode_all(const KcZdDecodeParams& P, hipStream_t st) {
    if (P.n_frames == 0) return;
    hipLaunchKernelGGL(kc_zstd_decode_all_kernel, dim3(P.n_frames), dim3(64), 0, st, P);
}
