// kc_zstd_dstream.hip — zstd.Decoder as a stream reader on the device (zstd/decoder.go:120-312, :486-567, :649-940).  The reference's
// stream decoder splits a block's work into three stages (startStreamDecoder): read the block and decode its literals, decode its
// sequences, execute them in order.  The first two depend on earlier blocks only through the tables a block repeats, so here
//   * kc_zstd_dstream_entropy_kernel gives every compressed block of a launch a wave of its own: it takes each of the four tables
//     (Huffman, literal lengths, offsets, match lengths) from the block itself, from the earlier block of the launch that last defined
//     it — rebuilt from that block's bytes —, or from the stream's carried state, decodes the literals into the block's literal slice
//     and the sequences as raw triples (litLen, matchLen, ofVal) into its sequence slice;
//   * kc_zstd_dstream_execute_kernel walks the blocks in order on one wave: it resolves the repeat offsets — the only work left that
//     runs sequence by sequence — and executes the sequences in groups of 64 (za_execute_group) into the stream's history buffer;
//   * kc_xxh64_stream_kernel carries the frame's XXH64 over the bytes the launch produced.
// ofVal is the offset value before repeat-offset resolution: 1 .. 3 is a repeat code, 4 and up the offset ofVal - 3.
// Untrusted input: every read is checked against the block's range, every write against the block's slices / the history buffer;
// every loop runs to a count read and checked beforehand (nSeq, regen, the block's size, the blocks of the launch).
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zdec_dev.h"
#include "kc_zexec_dev.h"

namespace {

// The literals header of a compressed block (blockdec.go:275-345).  Returns 0 or the error class.
struct ZsLitHdr {
    int ltype, hdr, comp;
    uint32_t regen;
    bool four;
};
__device__ __forceinline__ int zs_lit_header(const uint8_t* b, int bn, uint64_t window, ZsLitHdr& h) {
    h.ltype = b[0] & 3;
    const int sf = (b[0] >> 2) & 3;
    const int need = h.ltype < 2 ? ((sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3)) : (sf < 2 ? 3 : (sf == 2 ? 4 : 5));
    if (need > bn) return KCZD_CORRUPT;
    h.four = false;
    if (h.ltype < 2) {
        if ((sf & 1) == 0) { h.hdr = 1; h.regen = b[0] >> 3; }
        else if (sf == 1) { h.hdr = 2; h.regen = (b[0] >> 4) | ((uint32_t)b[1] << 4); }
        else { h.hdr = 3; h.regen = (b[0] >> 4) | ((uint32_t)b[1] << 4) | ((uint32_t)b[2] << 12); }
        if (h.regen > ZA_MAX_BLOCK || (uint64_t)h.regen > window) return KCZD_WINDOW;
        if (h.ltype == 0) { if ((uint64_t)h.hdr + h.regen > (uint64_t)bn) return KCZD_CORRUPT; h.comp = (int)h.regen; }
        else { if (h.hdr + 1 > bn) return KCZD_CORRUPT; h.comp = 1; }
        return 0;
    }
    if (sf < 2) { const uint32_t v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16); h.hdr = 3; h.regen = (v >> 4) & 0x3FF; h.comp = (v >> 14) & 0x3FF; h.four = sf == 1; }
    else if (sf == 2) { const uint32_t v = ld32(b); h.hdr = 4; h.regen = (v >> 4) & 0x3FFF; h.comp = (v >> 18) & 0x3FFF; h.four = true; }
    else { const uint64_t v = (uint64_t)ld32(b) | ((uint64_t)b[4] << 32); h.hdr = 5; h.regen = (uint32_t)((v >> 4) & 0x3FFFF); h.comp = (int)((v >> 22) & 0x3FFFF); h.four = true; }
    if (h.regen > ZA_MAX_BLOCK || (uint64_t)h.regen > window) return KCZD_WINDOW;
    if (h.hdr + h.comp > bn) return KCZD_CORRUPT;
    return 0;
}

// Huffman_Tree_Description at q (left bytes) -> S.huf, S.iv[V_HUFLOG] (huff0/decompress.go:29-168): weights on lane 0, table fill on
// all lanes.  Whole wave.  Returns the bytes the description took, or -1.
__device__ __forceinline__ int zs_huf_table(const uint8_t* q, int left, ZdShared& S, int lane, uint8_t* scratch, uint32_t scratchBytes) {
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
        S.iv[V_ERR] = e2;
        S.iv[V_NBATCH] = used;
    }
    KC_WAVE_SYNC();
    const int e2 = S.iv[V_ERR], used = S.iv[V_NBATCH], tableLog = S.iv[V_HUFLOG];
    KC_EMU_SYNC();
    if (e2) return -1;
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

// The sequences header of a compressed block behind its literals section (blockdec.go:505-555): count and its bytes.  0 or the class.
__device__ __forceinline__ int zs_seq_count(const uint8_t* sp, int sn, int& nSeq, int& sh) {
    if (sn < 1) return KCZD_CORRUPT;
    nSeq = sp[0];
    sh = 1;
    if (nSeq >= 128) {
        if (nSeq < 255) { if (sn < 2) return KCZD_CORRUPT; nSeq = ((nSeq - 128) << 8) + sp[1]; sh = 2; }
        else { if (sn < 3) return KCZD_CORRUPT; nSeq = sp[1] + (sp[2] << 8) + 0x7F00; sh = 3; }
    }
    return 0;
}

// Table `kind` (0 ll, 1 of, 2 ml) as the earlier block R of the launch defined it, rebuilt from that block's bytes.  Lane 0.
// The descriptions in front of it are read for their length only.  Returns false when the block does not define the table.
__device__ __forceinline__ bool zs_seq_table_from(const uint8_t* in, uint64_t in_len, const KcZsBlock& R, uint64_t window, int kind, ZdShared& S) {
    if (R.type != 2 || R.pos > in_len || (uint64_t)R.size > in_len - R.pos || R.size < 2 || R.size > ZA_MAX_BLOCK) return false;
    const uint8_t* b = in + R.pos;
    const int bn = (int)R.size;
    ZsLitHdr h;
    if (zs_lit_header(b, bn, window, h)) return false;
    const uint8_t* sp = b + h.hdr + h.comp;
    int sn = bn - h.hdr - h.comp, nSeq = 0, sh = 0;
    if (zs_seq_count(sp, sn, nSeq, sh) || nSeq == 0) return false;
    sp += sh; sn -= sh;
    if (sn < 1) return false;
    const uint8_t modes = sp[0];
    int q2 = 1;
    for (int k = 0; k < kind; k++) {
        const int mode = (modes >> (6 - 2 * k)) & 3;
        if (mode == 1) q2 += 1;
        else if (mode == 2) {
            int ns = 0, tl = 0;
            if (sn - q2 < 4) return false;
            const int used = zd_read_ncount(sp + q2, sn - q2, k == 0 ? 35 : 30, 9, S.norm, &ns, &tl);
            if (used == 0 || used > sn - q2) return false;
            q2 += used;
        }
        if (q2 > sn) return false;
    }
    const int mode = (modes >> (6 - 2 * kind)) & 3;
    if (mode == 3 || (mode == 2 && sn - q2 < 4)) return false;
    return zd_seq_table(mode, kind, sp + q2, sn - q2, S) >= 0;
}

__device__ __forceinline__ void zs_cells_in(ZdSym* dst, const KcZdCell* src, int lane) {
    for (int k = lane; k < (1 << 9); k += 64) { const KcZdCell a = src[k]; dst[k].base = a.base; dst[k].sym = a.sym; dst[k].nb = a.nb; }
}
__device__ __forceinline__ void zs_cells_out(KcZdCell* dst, const ZdSym* src, int lane) {
    for (int k = lane; k < (1 << 9); k += 64) { KcZdCell a; a.base = src[k].base; a.sym = src[k].sym; a.nb = src[k].nb; dst[k] = a; }
}

}  // namespace

__global__ __launch_bounds__(64) void kc_zstd_dstream_entropy_kernel(KcZsEntropyParams P) {
    __shared__ ZdShared S;
    const int lane = (int)threadIdx.x;
    const uint32_t bi = blockIdx.x;
    if (bi >= P.n_blocks) return;
    const KcZsBlock R = P.blocks[bi];
    if (R.type != 2) { if (lane == 0) P.status[bi] = 0; return; }  // raw and RLE blocks are the executor's
    const uint8_t* __restrict__ in = P.in;
    if (lane < 16) S.iv[lane] = 0;
    KC_WAVE_SYNC();
    int err = 0;
    do {
        if (R.pos > P.in_len || (uint64_t)R.size > P.in_len - R.pos || R.size > ZA_MAX_BLOCK || (uint64_t)R.size > P.window || R.size < 2) { err = KCZD_CORRUPT; break; }
        const uint8_t* __restrict__ b = in + R.pos;
        const int bn = (int)R.size;
        uint8_t* wscr = R.wt_bytes ? P.wts + R.wt_off : nullptr;
        // ---- literals section (blockdec.go:275-474) ----
        ZsLitHdr h;
        if ((err = zs_lit_header(b, bn, P.window, h)) != 0) break;
        // the slices were sized by the host walk from the same bytes: a header it read otherwise is not decoded
        if (!R.parsed || (uint32_t)h.ltype != R.ltype || h.regen != R.regen || (uint32_t)h.comp != R.comp || (uint32_t)h.hdr != R.lhdr) { err = KCZD_CORRUPT; break; }
        if (h.ltype >= 2) {
            if (R.lit_off > P.lits_len || (uint64_t)h.regen > P.lits_len - R.lit_off) { err = KCZD_CORRUPT; break; }
            uint8_t* __restrict__ lits = P.lits + R.lit_off;
            const uint8_t* q = b + h.hdr;
            int left = h.comp;
            if (h.ltype == 3 && R.src[KC_ZS_HUF] == KC_ZS_CARRIED) {
                if (!P.cur->huf_ok) { err = KCZD_CORRUPT; break; }  // "literal block was treeless, but no history was defined"
                for (int k = lane; k < (1 << 11); k += 64) S.huf[k] = P.cur->huf[k];
                if (lane == 0) S.iv[V_HUFLOG] = P.cur->huf_log;
                KC_WAVE_SYNC();
            } else {
                // the tree's description: this block's own, or the one of the earlier block of the launch that defined the tree
                const uint8_t* hq = q;
                int hleft = left;
                if (h.ltype == 3) {
                    const uint32_t j = R.src[KC_ZS_HUF];
                    if (j >= bi) { err = KCZD_CORRUPT; break; }
                    const KcZsBlock J = P.blocks[j];
                    if (J.type != 2 || J.pos > P.in_len || (uint64_t)J.size > P.in_len - J.pos || J.size < 2 || J.size > ZA_MAX_BLOCK) { err = KCZD_CORRUPT; break; }
                    ZsLitHdr hj;
                    if (zs_lit_header(in + J.pos, (int)J.size, P.window, hj) || hj.ltype != 2) { err = KCZD_CORRUPT; break; }
                    hq = in + J.pos + hj.hdr;
                    hleft = hj.comp;
                }
                const int used = zs_huf_table(hq, hleft, S, lane, wscr, R.wt_bytes);
                if (used < 0) { err = KCZD_CORRUPT; break; }
                if (h.ltype == 2) { q += used; left -= used; }
            }
            if ((R.def >> KC_ZS_HUF) & 1) {
                for (int k = lane; k < (1 << 11); k += 64) P.next->huf[k] = S.huf[k];
                if (lane == 0) { P.next->huf_log = S.iv[V_HUFLOG]; P.next->huf_ok = 1; }
            }
            // streams: one lane each (decompress.go Decompress1X / Decompress4X)
            const int hlog = S.iv[V_HUFLOG];
            int sOff = 0, sLen = left, oOff = 0, oLen = (int)h.regen;  // this lane's stream and where its symbols go
            int nstreams = 1;
            if (h.four) {
                if (left < 10) { err = KCZD_CORRUPT; break; }  // the jump table and a byte per stream (decompress_generic.go:19)
                const int s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8), s3 = q[4] | (q[5] << 8);
                if (6 + s1 + s2 + s3 > left) { err = KCZD_CORRUPT; break; }
                const int seg = ((int)h.regen + 3) / 4;
                if (seg * 3 > (int)h.regen) { err = KCZD_CORRUPT; break; }
                const int k = lane & 3;
                sOff = 6 + (k > 0 ? s1 : 0) + (k > 1 ? s2 : 0) + (k > 2 ? s3 : 0);
                sLen = k == 0 ? s1 : (k == 1 ? s2 : (k == 2 ? s3 : left - sOff));
                oOff = k * seg;
                oLen = k < 3 ? seg : (int)h.regen - 3 * seg;
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
            if (ballot64(serr != 0)) { err = KCZD_CORRUPT; break; }
            KC_WAVE_SYNC();
        }
        // ---- sequences section (blockdec.go:505-650) ----
        const uint8_t* sp = b + h.hdr + h.comp;
        int sn = bn - h.hdr - h.comp;
        int nSeq = 0, sh = 0;
        if ((err = zs_seq_count(sp, sn, nSeq, sh)) != 0) break;
        sp += sh; sn -= sh;
        if ((uint32_t)nSeq != R.nseq) { err = KCZD_CORRUPT; break; }
        if (nSeq == 0) {
            if (sn != 0) err = KCZD_CORRUPT;
            break;
        }
        if (R.seq_off > P.seqs_len || 3 * (uint64_t)nSeq > P.seqs_len - R.seq_off) { err = KCZD_CORRUPT; break; }
        uint32_t* __restrict__ oLL = P.seqs + R.seq_off;
        uint32_t* __restrict__ oML = oLL + nSeq;
        uint32_t* __restrict__ oOF = oML + nSeq;
        // the carried tables first (all lanes), then lane 0 reads this block's descriptions and rebuilds what an earlier block defined
        const uint32_t srcLL = R.src[KC_ZS_LL], srcOF = R.src[KC_ZS_OF], srcML = R.src[KC_ZS_ML];
        auto seq_src = [&](int kind) { return kind == 0 ? srcLL : (kind == 1 ? srcOF : srcML); };
        const uint8_t modes = sn >= 1 ? sp[0] : 0;
        {
            int e2 = 0;
            for (int kind = 0; kind < 3; kind++) {
                if (sn >= 1 && ((modes >> (6 - 2 * kind)) & 3) == 3 && seq_src(kind) == KC_ZS_CARRIED) {
                    if (!P.cur->ok[kind]) { e2 = 1; break; }  // Repeat_Mode without a table
                    zs_cells_in(kind == 0 ? S.ll : (kind == 1 ? S.of : S.ml), kind == 0 ? P.cur->ll : (kind == 1 ? P.cur->of : P.cur->ml), lane);
                    if (lane == 0) S.iv[V_LLLOG + kind] = P.cur->log[kind];
                }
            }
            KC_WAVE_SYNC();
            if (e2) { err = KCZD_CORRUPT; break; }
        }
        if (lane == 0) {
            int e2 = 0;
            int used = 0;
            if (sn < 1) e2 = 1;
            else {
                if (modes & 3) e2 = 1;
                int q2 = 1;
                for (int kind = 0; kind < 3 && !e2; kind++) {
                    const int mode = (modes >> (6 - 2 * kind)) & 3;
                    if (mode == 3) {
                        const uint32_t j = seq_src(kind);
                        if (j == KC_ZS_CARRIED) continue;
                        if (j >= bi || !zs_seq_table_from(in, P.in_len, P.blocks[j], P.window, kind, S)) e2 = 1;
                        continue;
                    }
                    if (mode == 2 && sn - q2 < 4) { e2 = 1; break; }  // (the reference's table reader wants four readable bytes, fse_decoder.go:57)
                    const int r = zd_seq_table(mode, kind, sp + q2, sn - q2, S);
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
        if ((R.def >> KC_ZS_LL) & 1) { zs_cells_out(P.next->ll, S.ll, lane); if (lane == 0) { P.next->log[0] = S.iv[V_LLLOG]; P.next->ok[0] = 1; } }
        if ((R.def >> KC_ZS_OF) & 1) { zs_cells_out(P.next->of, S.of, lane); if (lane == 0) { P.next->log[1] = S.iv[V_OFLOG]; P.next->ok[1] = 1; } }
        if ((R.def >> KC_ZS_ML) & 1) { zs_cells_out(P.next->ml, S.ml, lane); if (lane == 0) { P.next->log[2] = S.iv[V_MLLOG]; P.next->ok[2] = 1; } }
        // decode 64 sequences on lane 0, then store them with all lanes (seqdec.go:221-434 without the offset history)
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
                    if (s0 + i + 1 < nSeq) {
                        llS = cl.base + br.read(cl.nb);
                        mlS = cm.base + br.read(cm.nb);
                        ofS = co.base + br.read(co.nb);
                    }
                    if (br.pos < 0) { e2 = KCZD_EOF; break; }
                    S.seqLL[i] = llen; S.seqML[i] = mlen; S.seqOF[i] = ofVal;
                }
                if (!e2 && s0 + cnt >= nSeq && br.pos != 0) e2 = KCZD_CORRUPT;  // "extra bits on block"
                S.iv[V_ERR] = e2;
            }
            KC_WAVE_SYNC();
            const int e2 = S.iv[V_ERR];
            if (!e2 && lane < cnt) { oLL[s0 + lane] = S.seqLL[lane]; oML[s0 + lane] = S.seqML[lane]; oOF[s0 + lane] = S.seqOF[lane]; }
            KC_EMU_SYNC();
            if (e2) err = e2;
        }
    } while (false);
    if (lane == 0) P.status[bi] = (uint32_t)err;
}

__global__ __launch_bounds__(64) void kc_zstd_dstream_execute_kernel(KcZsExecParams P) {
    __shared__ ZdShared S;
    const int lane = (int)threadIdx.x;
    const uint8_t* __restrict__ in = P.in;
    ZaHist H;
    H.out = P.hist;
    H.dict = P.dict;
    H.dict_len = P.dict_len;
    uint32_t rep0 = P.cur->rep[0], rep1 = P.cur->rep[1], rep2 = P.cur->rep[2];
    const uint64_t blockMax = P.window < ZA_MAX_BLOCK ? P.window : (uint64_t)ZA_MAX_BLOCK;
    const uint64_t cap = P.hist_cap;
    uint64_t d = P.hist_pos;
    uint32_t done = 0;
    int err = 0;
    for (uint32_t bi = 0; bi < P.n_blocks; bi++) {
        const KcZsBlock R = P.blocks[bi];
        const uint64_t blockStart = d;
        err = (int)P.estatus[bi];
        if (!err && R.type < 2) {  // raw, RLE: the whole wave copies / fills
            if (R.size > ZA_MAX_BLOCK || (uint64_t)R.size > P.window) err = KCZD_WINDOW;
            else if (d + R.size > cap) err = KCZD_CORRUPT;
            else {
                if (R.type == 0) { for (uint32_t k = (uint32_t)lane; k < R.size; k += 64) H.out[d + k] = in[R.pos + k]; }
                else { const uint8_t v = in[R.pos]; for (uint32_t k = (uint32_t)lane; k < R.size; k += 64) H.out[d + k] = v; }
                d += R.size;
                KC_WAVE_SYNC();
            }
        } else if (!err) {
            const uint8_t* __restrict__ b = in + R.pos;
            ZaLits LT;
            LT.L = R.ltype == 0 ? b + R.lhdr : P.lits + R.lit_off;
            LT.rle = R.ltype == 1 ? (int)b[R.lhdr] : -1;
            const uint32_t regen = R.regen;
            const int nSeq = (int)R.nseq;
            const uint32_t* __restrict__ iLL = P.seqs + R.seq_off;
            const uint32_t* __restrict__ iML = iLL + nSeq;
            const uint32_t* __restrict__ iOF = iML + nSeq;
            uint32_t lp = 0;  // literals consumed
            for (int s0 = 0; s0 < nSeq && !err; s0 += 64) {
                const int cnt = nSeq - s0 < 64 ? nSeq - s0 : 64;
                if (lane < cnt) { S.seqLL[lane] = iLL[s0 + lane]; S.seqML[lane] = iML[s0 + lane]; S.seqOF[lane] = iOF[s0 + lane]; }
                KC_WAVE_SYNC();
                if (lane == 0) {  // the offset history (seqdec.go:262-300): the one thing here that runs sequence by sequence
                    for (int i = 0; i < cnt; i++) {
                        const uint32_t ofVal = S.seqOF[i];
                        uint32_t off;
                        if (ofVal > 3) { off = ofVal - 3; rep2 = rep1; rep1 = rep0; rep0 = off; }
                        else {
                            const uint32_t idx = ofVal + (S.seqLL[i] == 0 ? 1u : 0u);  // 1: repeat 1, 2: repeat 2, 3: repeat 3, 4: repeat 1 minus one byte
                            if (idx == 1) off = rep0;
                            else {
                                off = idx == 4 ? rep0 - 1 : (idx == 2 ? rep1 : rep2);
                                if (off == 0) off = 1;  // "0 is not valid; input is corrupted; force offset to 1" (seqdec.go:288-292)
                                if (idx != 2) rep2 = rep1;
                                rep1 = rep0;
                                rep0 = off;
                            }
                        }
                        S.seqOF[i] = off;
                    }
                }
                KC_WAVE_SYNC();
                err = za_execute_group(S, cnt, lane, H, LT, d, lp, regen, cap, blockStart, blockMax, P.window, KCZD_CORRUPT);
            }
            if (!err) {  // trailing literals (all of them when the block has no sequences)
                const uint32_t tail = regen - lp;
                if ((d - blockStart) + tail > blockMax) err = KCZD_CORRUPT;
                else if (d + tail > cap) err = KCZD_CORRUPT;
                else {
                    for (uint32_t k = (uint32_t)lane; k < tail; k += 64) H.out[d + k] = LT.at(lp + k);
                    d += tail;
                    KC_WAVE_SYNC();
                }
            }
        }
        if (lane == 0) { P.status[bi] = (uint32_t)err; P.out_size[bi] = err ? 0u : (uint32_t)(d - blockStart); }
        if (err) { d = blockStart; break; }
        done++;
    }
    // the next state: the tables no block of the launch defined are carried over, the offset history is the executor's
    if (!((P.def_mask >> KC_ZS_HUF) & 1)) {
        for (int k = lane; k < (1 << 11); k += 64) P.next->huf[k] = P.cur->huf[k];
        if (lane == 0) { P.next->huf_log = P.cur->huf_log; P.next->huf_ok = P.cur->huf_ok; }
    }
    for (int kind = 0; kind < 3; kind++) {
        if ((P.def_mask >> (KC_ZS_LL + kind)) & 1) continue;
        const KcZdCell* s = kind == 0 ? P.cur->ll : (kind == 1 ? P.cur->of : P.cur->ml);
        KcZdCell* t = kind == 0 ? P.next->ll : (kind == 1 ? P.next->of : P.next->ml);
        for (int k = lane; k < (1 << 9); k += 64) t[k] = s[k];
        if (lane == 0) { P.next->log[kind] = P.cur->log[kind]; P.next->ok[kind] = P.cur->ok[kind]; }
    }
    if (lane == 0) {
        P.next->rep[0] = rep0; P.next->rep[1] = rep1; P.next->rep[2] = rep2;
        P.result[0] = d - P.hist_pos;
        P.result[1] = done;
    }
}

// XXH64 (seed 0) with carried state (zstd/internal/xxhash/xxhash.go:61-156 Write / Sum64): the four accumulators on four lanes like
// kc_xxh64_kernel (kc_misc.hip), the stripes running over what the last launch left (< 32 bytes) followed by this launch's bytes.
#define ZS_XP1 11400714785074694791ULL
#define ZS_XP2 14029467366897019727ULL
#define ZS_XP3 1609587929392839161ULL
#define ZS_XP4 9650029242287828579ULL
#define ZS_XP5 2870177450012600261ULL
namespace {
__device__ __forceinline__ uint64_t zs_rol(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t zs_round(uint64_t acc, uint64_t input) { return zs_rol(acc + input * ZS_XP2, 31) * ZS_XP1; }
__device__ __forceinline__ uint64_t zs_merge(uint64_t acc, uint64_t val) { return (acc ^ zs_round(0, val)) * ZS_XP1 + ZS_XP4; }
}  // namespace

__global__ __launch_bounds__(64) void kc_xxh64_stream_kernel(KcZsHashParams P) {
    __shared__ uint64_t acc[4];
    __shared__ uint8_t tailbuf[64];
    const int a = (int)threadIdx.x;
    KcZsHash* __restrict__ h = P.h;
    const uint8_t* __restrict__ p = P.hist + P.start;
    const uint64_t len = P.result[0];
    const uint32_t tn = h->tail_n < 32 ? h->tail_n : 0;  // (always < 32)
    const uint64_t n = (uint64_t)tn + len;               // the bytes in front of the accumulators now
    const uint64_t stripes = n >> 5;
    if (a < 4) {
        uint64_t v = h->v[a];
        uint64_t s = 0;
        if (stripes > 0 && tn > 0) {  // the stripe that starts in the carried tail
            uint64_t w = 0;
            for (int k = 0; k < 8; k++) {
                const uint32_t at = 8u * (uint32_t)a + (uint32_t)k;
                w |= (uint64_t)(at < tn ? h->tail[at] : p[at - tn]) << (8 * k);
            }
            v = zs_round(v, w);
            s = 1;
        }
        const uint8_t* q = p + (tn ? 32 - tn : 0) + 8 * a;  // stripe s >= (tn ? 1 : 0) is at q + 32 * (s - (tn ? 1 : 0))
        const uint64_t rest = stripes - s;
        uint64_t i = 0;
        for (; i + 4 <= rest; i += 4) {
            const uint64_t w0 = ld64(q + (i << 5)), w1 = ld64(q + ((i + 1) << 5)), w2 = ld64(q + ((i + 2) << 5)), w3 = ld64(q + ((i + 3) << 5));
            v = zs_round(v, w0); v = zs_round(v, w1); v = zs_round(v, w2); v = zs_round(v, w3);
        }
        for (; i < rest; i++) v = zs_round(v, ld64(q + (i << 5)));
        acc[a] = v;
    }
    // the new tail: the bytes behind the last whole stripe
    const uint32_t nt = (uint32_t)(n & 31);
    const uint64_t t0 = stripes << 5;  // its position in tail ++ bytes
    if (a < 32 && (uint32_t)a < nt) {
        const uint64_t at = t0 + (uint64_t)a;
        tailbuf[a] = at < tn ? h->tail[at] : p[at - tn];
    }
    __syncthreads();
    if (a < 4) h->v[a] = acc[a];
    if (a < 32 && (uint32_t)a < nt) h->tail[a] = tailbuf[a];
    if (a == 0) {
        const uint64_t total = h->total + len;
        h->total = total;
        h->tail_n = nt;
        if (P.final) {
            uint64_t x;
            if (total >= 32) {
                const uint64_t v1 = acc[0], v2 = acc[1], v3 = acc[2], v4 = acc[3];
                x = zs_rol(v1, 1) + zs_rol(v2, 7) + zs_rol(v3, 12) + zs_rol(v4, 18);
                x = zs_merge(x, v1); x = zs_merge(x, v2); x = zs_merge(x, v3); x = zs_merge(x, v4);
            } else {
                x = ZS_XP5;  // v3 + prime5 with v3 == 0
            }
            x += total;
            const uint8_t* t = tailbuf;
            int rem = (int)nt;
            for (; rem >= 8; t += 8, rem -= 8) { x ^= zs_round(0, ld64(t)); x = zs_rol(x, 27) * ZS_XP1 + ZS_XP4; }
            if (rem >= 4) { x ^= (uint64_t)ld32(t) * ZS_XP1; x = zs_rol(x, 23) * ZS_XP2 + ZS_XP3; t += 4; rem -= 4; }
            for (; rem > 0; t++, rem--) { x ^= (uint64_t)t[0] * ZS_XP5; x = zs_rol(x, 11) * ZS_XP1; }
            x ^= x >> 33; x *= ZS_XP2; x ^= x >> 29; x *= ZS_XP3; x ^= x >> 32;
            h->digest = x;
        }
    }
}

void kc_launch_zstd_dstream_entropy(const KcZsEntropyParams& P, hipStream_t st) {
    if (P.n_blocks == 0) return;
    hipLaunchKernelGGL(kc_zstd_dstream_entropy_kernel, dim3(P.n_blocks), dim3(64), 0, st, P);
}
void kc_launch_zstd_dstream_execute(const KcZsExecParams& P, hipStream_t st) {
    if (P.n_blocks == 0) return;
    hipLaunchKernelGGL(kc_zstd_dstream_execute_kernel, dim3(1), dim3(64), 0, st, P);
}
void kc_launch_xxh64_stream(const KcZsHashParams& P, hipStream_t st) {
    hipLaunchKernelGGL(kc_xxh64_stream_kernel, dim3(1), dim3(64), 0, st, P);
}
