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
// The block parser is the one all three decoders share (kc_zdec_dev.h; its literals header and sequence count also run on the host,
// kc_zblock_dev.h, where the walk sizes the slices); the reader's own is where a repeated table comes from and where the results go.
// Untrusted input: every read is checked against the block's range, every write against the block's slices / the history buffer;
// every loop runs to a count read and checked beforehand (nSeq, regen, the block's size, the blocks of the launch).
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_wave.h"
#include "kc_zdec_dev.h"
#include "kc_zexec_dev.h"

namespace {

// Table `kind` (0 ll, 1 of, 2 ml) as the earlier block R of the launch defined it, rebuilt from that block's bytes into S (with
// S.iv[V_LLOK + kind]).  Lane 0.  The descriptions in front of it are read for their length only.  Returns false when the block does
// not define the table.
__device__ __forceinline__ bool zs_seq_table_from(const uint8_t* in, uint64_t in_len, const KcZsBlock& R, uint64_t window, int kind, ZdShared& S) {
    if (R.type != 2 || R.pos > in_len || (uint64_t)R.size > in_len - R.pos || R.size < 2 || R.size > ZA_MAX_BLOCK) return false;
    const uint8_t* b = in + R.pos;
    const int bn = (int)R.size;
    ZdLitHdr h;
    if (zd_lit_header(b, bn, window, h)) return false;
    const uint8_t* sp = b + h.hdr + h.comp;
    int sn = bn - h.hdr - h.comp, nSeq = 0, sh = 0;
    if (zd_seq_count(sp, sn, nSeq, sh) || nSeq == 0) return false;
    sp += sh; sn -= sh;
    if (sn < 1) return false;
    const uint8_t modes = sp[0];
    int q2 = 1;
    for (int k = 0; k < kind; k++) {
        const int used = zd_seq_table_skip(zd_seq_mode(modes, k), k, sp + q2, sn - q2, S);
        if (used < 0) return false;
        q2 += used;
    }
    const int mode = zd_seq_mode(modes, kind);
    return mode != 3 && zd_seq_table(mode, kind, sp + q2, sn - q2, S) >= 0;
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
        ZdLitHdr h;
        if ((err = zd_lit_header(b, bn, P.window, h)) != 0) break;
        // the slices were sized by the host walk from the same bytes: a header it read otherwise is not decoded
        if (!R.parsed || (uint32_t)h.ltype != R.ltype || h.regen != R.regen || (uint32_t)h.comp != R.comp || (uint32_t)h.hdr != R.lhdr) { err = KCZD_CORRUPT; break; }
        if (h.ltype >= 2) {
            if (R.lit_off > P.lits_len || (uint64_t)h.regen > P.lits_len - R.lit_off) { err = KCZD_CORRUPT; break; }
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
                    ZdLitHdr hj;
                    if (zd_lit_header(in + J.pos, (int)J.size, P.window, hj) || hj.ltype != 2) { err = KCZD_CORRUPT; break; }
                    hq = in + J.pos + hj.hdr;
                    hleft = hj.comp;
                }
                const int used = zd_huf_table(hq, hleft, S, lane, wscr, R.wt_bytes);
                if (used < 0) { err = KCZD_CORRUPT; break; }
                if (h.ltype == 2) { q += used; left -= used; }
            }
            if ((R.def >> KC_ZS_HUF) & 1) {
                for (int k = lane; k < (1 << 11); k += 64) P.next->huf[k] = S.huf[k];
                if (lane == 0) { P.next->huf_log = S.iv[V_HUFLOG]; P.next->huf_ok = 1; }
            }
            if ((err = zd_huf_streams(q, left, h.four, h.regen, S, lane, P.lits + R.lit_off)) != 0) break;
        }
        // ---- sequences section (blockdec.go:505-650) ----
        const uint8_t* sp = b + h.hdr + h.comp;
        int sn = bn - h.hdr - h.comp;
        int nSeq = 0, sh = 0;
        if ((err = zd_seq_count(sp, sn, nSeq, sh)) != 0) break;
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
        // Repeat_Mode: the table comes from the carried state (all lanes copy it) or from the earlier block of the launch that defined
        // it (lane 0 rebuilds it from that block's bytes).  A table that is not there stays unmarked, and the block's own table reader
        // (zd_seq_tables) refuses the mode.
        const uint32_t srcLL = R.src[KC_ZS_LL], srcOF = R.src[KC_ZS_OF], srcML = R.src[KC_ZS_ML];
        for (int kind = 0; kind < 3 && sn >= 1; kind++) {
            if (zd_seq_mode(sp[0], kind) != 3) continue;
            const uint32_t j = kind == 0 ? srcLL : (kind == 1 ? srcOF : srcML);
            if (j == KC_ZS_CARRIED) {
                if (!P.cur->ok[kind]) continue;
                zd_cells_in(kind == 0 ? S.ll : (kind == 1 ? S.of : S.ml), kind == 0 ? P.cur->ll : (kind == 1 ? P.cur->of : P.cur->ml), 1 << 9, lane);
                if (lane == 0) { S.iv[V_LLLOG + kind] = P.cur->log[kind]; S.iv[V_LLOK + kind] = 1; }
            } else if (lane == 0 && j < bi) zs_seq_table_from(in, P.in_len, P.blocks[j], P.window, kind, S);
        }
        {
            const int used = zd_seq_tables(sp, sn, S, lane);
            if (used < 0) { err = KCZD_CORRUPT; break; }
            sp += used; sn -= used;
        }
        if ((R.def >> KC_ZS_LL) & 1) { zd_cells_out(P.next->ll, S.ll, 1 << 9, lane); if (lane == 0) { P.next->log[0] = S.iv[V_LLLOG]; P.next->ok[0] = 1; } }
        if ((R.def >> KC_ZS_OF) & 1) { zd_cells_out(P.next->of, S.of, 1 << 9, lane); if (lane == 0) { P.next->log[1] = S.iv[V_OFLOG]; P.next->ok[1] = 1; } }
        if ((R.def >> KC_ZS_ML) & 1) { zd_cells_out(P.next->ml, S.ml, 1 << 9, lane); if (lane == 0) { P.next->log[2] = S.iv[V_MLLOG]; P.next->ok[2] = 1; } }
        // decode 64 sequences on lane 0, then store them with all lanes: the offset values stay unresolved (the executor's)
        ZdSeqDec sq;
        if ((err = zd_seq_open(sq, sp, sn, S, lane)) != 0) break;
        for (int s0 = 0; s0 < nSeq && !err; s0 += 64) {
            const int cnt = nSeq - s0 < 64 ? nSeq - s0 : 64;
            err = zd_seq_group(sq, S, lane, s0, cnt, nSeq, [](uint32_t ofVal, uint32_t, uint32_t& off) { off = ofVal; return true; });
            if (!err && lane < cnt) { oLL[s0 + lane] = S.seqLL[lane]; oML[s0 + lane] = S.seqML[lane]; oOF[s0 + lane] = S.seqOF[lane]; }
            KC_EMU_SYNC();  // (lane 0 refills the three arrays for the next group)
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
                if (lane == 0) {  // the offset history: the one thing here that runs sequence by sequence
                    for (int i = 0; i < cnt; i++) {
                        uint32_t off = zd_rep_offset(S.seqOF[i], S.seqLL[i], rep0, rep1, rep2);
                        if (off == 0) off = rep0 = 1;  // "0 is not valid; input is corrupted; force offset to 1" (seqdec.go:288-292)
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
