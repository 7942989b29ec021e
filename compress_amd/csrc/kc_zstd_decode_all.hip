// kc_zstd_decode_all.hip — zstd.Decoder.DecodeAll on the device as a product path (zstd/decoder.go:319-410 -> framedec.go:330-412 ->
// blockdec.go:227-650 -> seqdec.go:221-434, fse_decoder.go, huff0/decompress.go).  One wave per FRAME of the plan
// (kc_zstd_plan.hip): the frame decodes into its staging slot, from where the host compacts the inputs' frames into the dense
// output.  Unlike the verifier (kc_zstd_decode.hip) the kernel knows no decoded length, takes the dictionary the frame's id names
// — content as history, and for full-format dictionaries the repeat offsets and the Huffman / FSE tables as the "previous" tables
// of the first block —, checks offsets against the window and the block against min(window, 128 KiB) as the reference does, and
// executes a decoded group of 64 sequences together instead of one after the other (za_execute_group).
// Untrusted input: every read is checked against the frame's block range, every write against the frame's slot.
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zdec_dev.h"
#include "kc_zexec_dev.h"

namespace {

// One sequence table according to its mode (blockdec.go:556-622).  Lane 0 only.  Returns bytes consumed (>= 0) or -1.
// (The reference's table reader wants four readable bytes in front of it, fse_decoder.go:57.)
__device__ int za_seq_table(int mode, int kind, const uint8_t* p, int n, ZdShared& S) {
    if (mode == 2 && n < 4) return -1;
    return zd_seq_table(mode, kind, p, n, S);
}

}  // namespace

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
            for (int k = lane; k < (1 << 9); k += 64) {
                const KcZdCell a = D->ll[k], b = D->ml[k];
                S.ll[k].base = a.base; S.ll[k].sym = a.sym; S.ll[k].nb = a.nb;
                S.ml[k].base = b.base; S.ml[k].sym = b.sym; S.ml[k].nb = b.nb;
            }
            for (int k = lane; k < (1 << 8); k += 64) { const KcZdCell a = D->of[k]; S.of[k].base = a.base; S.of[k].sym = a.sym; S.of[k].nb = a.nb; }
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
        const int ltype = b[0] & 3, sf = (b[0] >> 2) & 3;
        {
            const int need = ltype < 2 ? ((sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3)) : (sf < 2 ? 3 : (sf == 2 ? 4 : 5));
            if (need > bn) { err = KCZD_CORRUPT; break; }
        }
        int hdr = 0, comp = 0;
        uint32_t regen = 0;
        bool four = false;
        ZaLits LT;
        LT.L = nullptr;
        LT.rle = -1;
        if (ltype < 2) {
            if ((sf & 1) == 0) { hdr = 1; regen = b[0] >> 3; }
            else if (sf == 1) { hdr = 2; regen = (b[0] >> 4) | ((uint32_t)b[1] << 4); }
            else { hdr = 3; regen = (b[0] >> 4) | ((uint32_t)b[1] << 4) | ((uint32_t)b[2] << 12); }
            if (regen > ZA_MAX_BLOCK || (uint64_t)regen > F.window) { err = KCZD_WINDOW; break; }
            if (ltype == 0) { if ((uint64_t)hdr + regen > (uint64_t)bn) { err = KCZD_CORRUPT; break; } LT.L = b + hdr; comp = (int)regen; }
            else { if (hdr + 1 > bn) { err = KCZD_CORRUPT; break; } LT.rle = b[hdr]; comp = 1; }
        } else {
            if (sf < 2) { const uint32_t v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16); hdr = 3; regen = (v >> 4) & 0x3FF; comp = (v >> 14) & 0x3FF; four = sf == 1; }
            else if (sf == 2) { const uint32_t v = ld32(b); hdr = 4; regen = (v >> 4) & 0x3FFF; comp = (v >> 18) & 0x3FFF; four = true; }
            else { const uint64_t v = (uint64_t)ld32(b) | ((uint64_t)b[4] << 32); hdr = 5; regen = (uint32_t)((v >> 4) & 0x3FFFF); comp = (int)((v >> 22) & 0x3FFFF); four = true; }
            if (regen > ZA_MAX_BLOCK || (uint64_t)regen > F.window) { err = KCZD_WINDOW; break; }
            if (hdr + comp > bn) { err = KCZD_CORRUPT; break; }
            const uint8_t* q = b + hdr;
            int left = comp;
            if (ltype == 2) {
                // Huffman_Tree_Description (huff0/decompress.go:29-168): weights on lane 0, table fill on all lanes
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
                        else { nw = zd_fse_weights(q + 1, hb, S, S.weights, lits, KC_ZD_LIT_STRIDE); if (nw <= 0) e2 = 1; }
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
                    S.iv[V_ERR] = e2;
                    S.iv[V_NBATCH] = used;
                }
                KC_WAVE_SYNC();
                const int e2 = S.iv[V_ERR], used = S.iv[V_NBATCH], tableLog = S.iv[V_HUFLOG];
                KC_EMU_SYNC();
                if (e2) { err = KCZD_CORRUPT; break; }
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
                q += used; left -= used;
            } else if (!S.iv[V_HUFOK]) { err = KCZD_CORRUPT; break; }  // "literal block was treeless, but no history was defined"
            // streams: one lane each (decompress.go Decompress1X / Decompress4X)
            const int hlog = S.iv[V_HUFLOG];
            int sOff[4] = {0, 0, 0, 0}, sLen[4] = {left, 0, 0, 0}, oOff[4] = {0, 0, 0, 0}, oLen[4] = {(int)regen, 0, 0, 0};
            int nstreams = 1;
            if (four) {
                if (left < 10) { err = KCZD_CORRUPT; break; }  // the jump table and a byte per stream (decompress_generic.go:19)
                const int s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8), s3 = q[4] | (q[5] << 8);
                if (6 + s1 + s2 + s3 > left) { err = KCZD_CORRUPT; break; }
                const int seg = ((int)regen + 3) / 4;
                if (seg * 3 > (int)regen) { err = KCZD_CORRUPT; break; }
                sOff[0] = 6; sLen[0] = s1; sOff[1] = 6 + s1; sLen[1] = s2; sOff[2] = 6 + s1 + s2; sLen[2] = s3;
                sOff[3] = 6 + s1 + s2 + s3; sLen[3] = left - sOff[3];
                for (int k = 0; k < 4; k++) { oOff[k] = k * seg; oLen[k] = k < 3 ? seg : (int)regen - 3 * seg; }
                nstreams = 4;
            }
            int serr = 0;
            if (lane < nstreams) {
                ZdRBits br;
                if (!br.init(q + sOff[lane], sLen[lane])) serr = 1;
                else {
                    uint8_t* o = lits + oOff[lane];
                    for (int i = 0; i < oLen[lane]; i++) {
                        const uint16_t e = S.huf[br.peek(hlog)];
                        o[i] = (uint8_t)(e >> 8);
                        br.pos -= (e & 0xFF);
                    }
                    if (br.pos != 0) serr = 1;
                }
            }
            if (ballot64(serr != 0)) { err = KCZD_CORRUPT; break; }
            KC_WAVE_SYNC();
            LT.L = lits;
        }
        // ---- sequences section (blockdec.go:505-650) ----
        const uint8_t* sp = b + hdr + comp;
        int sn = bn - hdr - comp;
        if (sn < 1) { err = KCZD_CORRUPT; break; }
        int nSeq = sp[0];
        int sh = 1;
        if (nSeq >= 128) {
            if (nSeq < 255) { if (sn < 2) { err = KCZD_CORRUPT; break; } nSeq = ((nSeq - 128) << 8) + sp[1]; sh = 2; }
            else { if (sn < 3) { err = KCZD_CORRUPT; break; } nSeq = sp[1] + (sp[2] << 8) + 0x7F00; sh = 3; }
        }
        sp += sh; sn -= sh;
        if (nSeq == 0) {
            if (sn != 0) { err = KCZD_CORRUPT; break; }
            if (d + regen > cap) { err = capClass; break; }
            for (uint32_t k = (uint32_t)lane; k < regen; k += 64) H.out[d + k] = LT.at(k);
            d += regen;
            KC_WAVE_SYNC();
            continue;
        }
        if (lane == 0) {
            int e2 = 0;
            int used = 0;
            if (sn < 1) e2 = 1;
            else {
                const uint8_t modes = sp[0];
                if (modes & 3) e2 = 1;
                int q2 = 1;
                for (int kind = 0; kind < 3 && !e2; kind++) {
                    const int mode = (modes >> (6 - 2 * kind)) & 3;
                    const int r = za_seq_table(mode, kind, sp + q2, sn - q2, S);
                    if (r < 0) e2 = 1; else q2 += r;
                }
                used = q2;
            }
            S.iv[V_ERR] = e2;
            S.iv[V_NBATCH] = used;
        }
        KC_WAVE_SYNC();
        {
            const int e2 = S.iv[V_ERR], used = S.iv[V_NBATCH];
            KC_EMU_SYNC();
            if (e2) { err = KCZD_CORRUPT; break; }
            sp += used; sn -= used;
        }
        // decode 64 sequences on lane 0, then execute them on all lanes (seqdec.go:221-434)
        ZdRBits br;
        br.p = nullptr; br.pos = 0;
        uint32_t llS = 0, ofS = 0, mlS = 0;
        int brErr = 0;
        if (lane == 0) {
            if (!br.init(sp, sn)) brErr = KCZD_CORRUPT;
            else {
                llS = br.read(S.iv[V_LLLOG]); ofS = br.read(S.iv[V_OFLOG]); mlS = br.read(S.iv[V_MLLOG]);
                if (br.pos < 0) brErr = KCZD_EOF;  // (the bit reader ran dry: io.ErrUnexpectedEOF)
            }
        }
        brErr = uni(brErr);
        if (brErr) { err = brErr; break; }
        uint32_t lp = 0;  // literals consumed
        for (int s0 = 0; s0 < nSeq && !err; s0 += 64) {
            const int cnt = nSeq - s0 < 64 ? nSeq - s0 : 64;
            if (lane == 0) {
                int e2 = 0;
                for (int i = 0; i < cnt && !e2; i++) {
                    const ZdSym cl = S.ll[llS], co = S.of[ofS], cm = S.ml[mlS];
                    if (cl.sym > 35 || cm.sym > 52 || co.sym > 30) { e2 = KCZD_CORRUPT; break; }
                    uint32_t ofVal;
                    if (co.sym <= 24) ofVal = (1u << co.sym) + br.read(co.sym);
                    else { const uint32_t hi = br.read(co.sym - 16); const uint32_t lo = br.read(16); ofVal = (1u << co.sym) + ((hi << 16) | lo); }
                    const uint32_t mlen = kMLBase[cm.sym] + br.read(kMLBits[cm.sym]);
                    const uint32_t llen = kLLBase[cl.sym] + br.read(kLLBits[cl.sym]);
                    uint32_t off;
                    if (co.sym > 1) { off = ofVal - 3; rep2 = rep1; rep1 = rep0; rep0 = off; }
                    else {
                        const uint32_t idx = ofVal + (llen == 0 ? 1u : 0u);  // 1: repeat 1, 2: repeat 2, 3: repeat 3, 4: repeat 1 minus one byte
                        if (idx == 1) off = rep0;
                        else {
                            off = idx == 4 ? rep0 - 1 : (idx == 2 ? rep1 : rep2);
                            if (off == 0) off = 1;  // "0 is not valid; input is corrupted; force offset to 1" (seqdec.go:288-292)
                            if (idx != 2) rep2 = rep1;
                            rep1 = rep0;
                            rep0 = off;
                        }
                    }
                    if (s0 + i + 1 < nSeq) {
                        llS = cl.base + br.read(cl.nb);
                        mlS = cm.base + br.read(cm.nb);
                        ofS = co.base + br.read(co.nb);
                    }
                    if (br.pos < 0) { e2 = KCZD_EOF; break; }
                    S.seqLL[i] = llen; S.seqML[i] = mlen; S.seqOF[i] = off;
                }
                if (!e2 && s0 + cnt >= nSeq && br.pos != 0) e2 = KCZD_CORRUPT;  // "extra bits on block"
                S.iv[V_ERR] = e2;
            }
            KC_WAVE_SYNC();
            const int e2 = S.iv[V_ERR];
            KC_EMU_SYNC();
            if (e2) { err = e2; break; }
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
