// kc_flate_deflate.hip — flate.NewWriter(w, flate.HuffmanOnly) / gzip.NewWriterLevel(w, gzip.HuffmanOnly) over a batch of independent
// inputs: THREE LAUNCHES, cut by 32 KiB block so that one large input spreads over the chip as many small ones do
// (kc_deflate_dev.h has the plan; the host sequence is kc_deflate_host.h's).
//
//   plan   one wave per block: histogram (LDS adds), the quick check, the block's own table (generate: rank sort wave-wide,
//          bitCounts on one lane over LDS), its bits under that table, its codegen sequence, code-length code and headerSize
//   chain  one wave per input, blocks in order: lastHeader, the table in force and the bit position; reuseSize is a wave
//          reduction of the block's histogram against the lengths in force; gzip: the input's CRC-32 (s2_crc32c_wave, IEEE tables)
//   emit   one wave per block: owed EOB, header or stored header, the codes (lanes take contiguous spans, a wave scan of the spans'
//          bit lengths places them) or the raw bytes, EOB, and behind an input's last block the stream's end and gzip's trailer
//
// The words of dst are shared at every seam — between lanes, blocks and inputs —, so dst is zeroed by the host sequence and the
// seams are ORed in (DfSink).  No loop depends on the bytes compressed for its end: every one runs over a block's length, the 257
// symbols or the levels of bitCounts.
#include "kc_deflate_dev.h"
#include "kc_flate_dev.h"

struct DfPlanLds {
    uint32_t hist[260];
    DfGenLds G;
    uint8_t len[260];
    uint16_t code[260];
    uint8_t codegen[264];
    uint32_t cgfreq[20];
    uint8_t cglen[20];
    uint16_t cgcode[20];
    uint32_t flag, n_codegen, ncg, hdr_bits;
};

// the bytes of record r: [begin, end) in src; its input and its index in it
struct DfSpan { uint64_t begin, end; uint32_t input, idx, nblk; };
__device__ __forceinline__ DfSpan df_span(const KcDeflateParams& P, const uint32_t r) {
    DfSpan s;
    s.input = P.blk_in[r];
    s.idx = r - P.blk0[s.input];
    s.nblk = P.blk0[s.input + 1] - P.blk0[s.input];
    const uint64_t e = P.in_off[s.input + 1];
    s.begin = P.in_off[s.input] + (uint64_t)s.idx * P.block;
    s.end = s.begin + P.block < e ? s.begin + P.block : e;
    return s;
}

__global__ __launch_bounds__(64) void kc_deflate_plan_kernel(KcDeflateParams P) {
    __shared__ DfPlanLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= P.nblocks) return;
    const DfSpan sp = df_span(P, r);
    const uint32_t n = (uint32_t)(sp.end - sp.begin);
    const uint8_t* s = P.src + sp.begin;
    KcDfBlock& R = P.rec[r];
    for (int k = lane; k < 260; k += 64) L.hist[k] = 0;
    KC_WAVE_SYNC();
    for (uint32_t k = (uint32_t)lane * 4; k + 4 <= n; k += 256) {
        const uint32_t w = ld32(s + k);
        atomicAdd(&L.hist[w & 0xFF], 1u);
        atomicAdd(&L.hist[(w >> 8) & 0xFF], 1u);
        atomicAdd(&L.hist[(w >> 16) & 0xFF], 1u);
        atomicAdd(&L.hist[w >> 24], 1u);
    }
    if ((uint32_t)lane < (n & 3u)) atomicAdd(&L.hist[s[(n & ~3u) + (uint32_t)lane]], 1u);
    KC_WAVE_SYNC();
    for (int k = lane; k < 256; k += 64) R.hist[k] = (uint16_t)L.hist[k];
    if (lane == 0) {
        // the quick check of incompressible content (:1012-1033).  float64 in the reference, exact in integers:
        // sum (v - n/256)^2 < 2n  <=>  sum (256 v - n)^2 < 2 n 65536
        uint32_t quick = 0;
        if (n > 1024) {
            uint64_t acc = 0;
            for (int k = 0; k < 256; k++) {
                const int64_t d = (int64_t)256 * (int64_t)L.hist[k] - (int64_t)n;
                acc += (uint64_t)(d * d);
            }
            quick = acc < (uint64_t)2 * n * 65536u;
        }
        L.flag = quick;
        L.hist[256] = 1;  // literalFreq[endBlockMarker] = 1
    }
    KC_WAVE_SYNC();
    const uint32_t quick = L.flag;
    if (lane == 0) R.quick = quick;
    if (quick || n == 0) return;
    df_generate(L.hist, 257, 15, L.G, L.len, L.code, lane);
    uint32_t bits = 0;
    for (int k = lane; k < 257; k += 64) bits += L.hist[k] * L.len[k];
    const uint32_t self_bits = wave_reduce_sum(bits);
    if (lane == 0) L.n_codegen = df_codegen(L.len, L.codegen, L.cgfreq);
    KC_WAVE_SYNC();
    df_generate(L.cgfreq, 19, 7, L.G, L.cglen, L.cgcode, lane);
    if (lane == 0) {  // codegens / headerSize (:350-368)
        uint32_t ncg = 19;
        while (ncg > 4 && L.cgfreq[DF_CODEGEN_ORDER[ncg - 1]] == 0) ncg--;
        uint32_t h = 3 + 5 + 5 + 4 + 3 * ncg + L.cgfreq[16] * 2 + L.cgfreq[17] * 3 + L.cgfreq[18] * 7;
        for (int k = 0; k < 19; k++) h += L.cgfreq[k] * L.cglen[k];
        R.ncg = ncg;
        R.hdr_bits = h;
        R.n_codegen = L.n_codegen;
        R.self_bits = self_bits;
    }
    const uint32_t ncgn = L.n_codegen;
    for (int k = lane; k < 257; k += 64) { R.len[k] = L.len[k]; R.code[k] = L.code[k]; }
    for (uint32_t k = (uint32_t)lane; k < ncgn; k += 64) R.codegen[k] = L.codegen[k];
    if (lane < 19) { R.cglen[lane] = L.cglen[lane]; R.cgcode[lane] = L.cgcode[lane]; }
}

struct DfChainLds { uint32_t crcT[4][256], crcM[32], crcP[64]; };

__global__ __launch_bounds__(64) void kc_deflate_chain_kernel(KcDeflateParams P) {
    __shared__ DfChainLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    const uint32_t r0 = P.blk0[i], nblk = P.blk0[i + 1] - r0;
    const uint64_t begin = P.in_off[i], len = P.in_off[i + 1] - begin;
    uint32_t last_header = 0, table = 0;
    uint64_t bit = 0;
    for (uint32_t b = 0; b < nblk; b++) {
        KcDfBlock& R = P.rec[r0 + b];
        const uint64_t off = (uint64_t)b * P.block;
        const uint32_t n = (uint32_t)(len - off < P.block ? len - off : P.block);
        const bool last = b + 1 == nblk;
        uint32_t decision = KCDF_NONE, flags = last ? KCDF_F_LAST : 0u, prev = table;
        const uint64_t start = bit;
        if (n) {
            const uint32_t ssize = (n + 5) * 8;
            bool stored = uniu(R.quick) != 0;
            uint32_t est = 0;
            if (stored) decision = KCDF_QUICK;
            else {
                est = uniu(R.self_bits) + last_header;
                if (last_header == 0) est += KCDF_GUESS_HEADER_BITS;
                est += est >> P.penalty;
                if (ssize <= est) { stored = true; decision = KCDF_EST; }
            }
            if (stored) {  // writeStoredHeader + writeBytes: an owed EOB, 3 bits, to the byte, LEN NLEN, the bytes
                if (last_header) { flags |= KCDF_F_OWED; bit += P.rec[table].len[256]; last_header = 0; }
                bit += 3;
                bit = (bit + 7) & ~(uint64_t)7;
                bit += 32 + (uint64_t)n * 8;
            } else {
                uint32_t body;
                if (last_header) {  // canReuseBits of the table in force over literalFreq[:256] (:1055-1068)
                    const KcDfBlock& T = P.rec[table];
                    uint32_t sum = 0;
                    bool missing = false;
                    for (int k = lane; k < 256; k += 64) {
                        const uint32_t f = R.hist[k], l = T.len[k];
                        missing |= f && !l;
                        sum += f * l;
                    }
                    sum = wave_reduce_sum(sum);
                    const bool none = __ballot(missing) != 0;
                    const uint32_t reuse = none ? (uint32_t)DF_MAXI32 : sum;
                    if (est < reuse) {
                        decision = KCDF_NEW_OWED;
                        flags |= KCDF_F_OWED | (none ? KCDF_F_NOT_REUSABLE : 0u);
                        bit += T.len[256];
                        last_header = 0;
                    } else {
                        decision = KCDF_REUSE;
                        body = sum;
                    }
                } else {
                    decision = KCDF_FIRST;
                }
                if (last_header == 0) {
                    table = r0 + b;
                    last_header = uniu(R.hdr_bits);
                    bit += last_header;
                    body = uniu(R.self_bits) - R.len[256];
                }
                bit += body;
                if (last) {  // sync: the EOB, and nothing is owed
                    flags |= KCDF_F_SYNC;
                    bit += P.rec[table].len[256];
                    last_header = 0;
                }
            }
        }
        if (lane == 0) { R.decision = decision; R.flags = flags; R.table = table; R.prev_table = prev; R.start_bit = start; }
    }
    // writeStoredHeader(0, eof) and flush: nothing is owed here (the last block went out with sync)
    if (P.end == KCDF_END_CLOSE) bit += 10;
    else bit += 3;
    bit = (bit + 7) & ~(uint64_t)7;
    if (P.end == KCDF_END_FLUSH) bit += 32;
    uint64_t bytes = bit >> 3;
    if (P.gzip) {
        bytes += 10;
        if (P.end == KCDF_END_CLOSE) {
            bytes += 8;
            fl_crc_tables(L.crcT, lane);
            const uint8_t* s = P.src + begin;
            auto rd32 = [&](int k) -> uint32_t { return ld32(s + k); };
            auto rdb = [&](int k) -> uint32_t { return s[k]; };
            const uint32_t c = s2_crc32c_wave(rd32, rdb, (int)len, L.crcT, L.crcM, L.crcP, lane);
            if (lane == 0) P.crc[i] = c;
        }
    }
    if (lane == 0) P.size[i] = bytes;
}

struct DfEmitLds {
    uint32_t tab[260];  // code | len << 16 of the table in force
    uint8_t codegen[264];
    uint16_t cgcode[20];
    uint8_t cglen[20];
};

__global__ __launch_bounds__(64) void kc_deflate_emit_kernel(KcDeflateParams P) {
    __shared__ DfEmitLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= P.nblocks) return;
    const DfSpan sp = df_span(P, r);
    const uint32_t n = (uint32_t)(sp.end - sp.begin);
    const uint8_t* s = P.src + sp.begin;
    const KcDfBlock& R = P.rec[r];
    const uint32_t decision = uniu(R.decision), flags = uniu(R.flags);
    const bool huff = decision >= KCDF_FIRST, fresh = decision == KCDF_FIRST || decision == KCDF_NEW_OWED;

    DfSink S;
    const uint64_t mis = (uint64_t)(uintptr_t)P.dst & 3u;
    S.W = (uint32_t*)(P.dst - mis);
    S.live = lane == 0;
    S.elo = mis ? 0 : UINT64_MAX;
    S.ehi = ((mis + P.total) & 3u) ? (mis + P.total) >> 2 : UINT64_MAX;
    S.edge = P.edge;
    const uint64_t in0 = (mis + P.out0[sp.input]) * 8;            // the input's first bit, counted from W
    const uint64_t df0 = in0 + (P.gzip ? 80u : 0u);               // its DEFLATE stream's
    uint64_t bit = df0 + R.start_bit;

    if (huff) {
        const KcDfBlock& T = P.rec[uniu(R.table)];
        for (int k = lane; k < 257; k += 64) L.tab[k] = (uint32_t)T.code[k] | (uint32_t)T.len[k] << 16;
        if (fresh) {
            const uint32_t ncgn = uniu(R.n_codegen);
            for (uint32_t k = (uint32_t)lane; k < ncgn; k += 64) L.codegen[k] = R.codegen[k];
            if (lane < 19) { L.cglen[lane] = R.cglen[lane]; L.cgcode[lane] = R.cgcode[lane]; }
        }
        KC_WAVE_SYNC();
    }
    // ---- what comes before the block's bytes: every lane follows the position, lane 0 writes ----
    if (sp.idx == 0 && P.gzip) {  // 1f 8b 08 00 | MTIME 0 | XFL 0, OS 255 (gzip/gzip.go: the default Header at this level)
        df_seek(S, in0);
        df_put(S, 0x00088b1fu, 32); df_put(S, 0, 32); df_put(S, 0xff00u, 16);
        df_close(S);
    }
    df_seek(S, bit);
    if (flags & KCDF_F_OWED) {
        const KcDfBlock& O = P.rec[uniu(R.prev_table)];
        df_put(S, O.code[256], O.len[256]);
    }
    if (decision == KCDF_QUICK || decision == KCDF_EST) {  // writeStoredHeader(n, false): :521-528
        df_put(S, 0, 3);
        df_pad_to_byte(S);
        df_put(S, n, 16);
        df_put(S, ~n & 0xFFFFu, 16);
    } else if (fresh) {  // writeDynamicHeader(257, 1, ncg, false): :458-497
        const uint32_t ncg = uniu(R.ncg), ncgn = uniu(R.n_codegen);
        df_put(S, 4, 3); df_put(S, 0, 5); df_put(S, 0, 5); df_put(S, ncg - 4, 4);
        for (uint32_t k = 0; k < ncg; k++) df_put(S, L.cglen[DF_CODEGEN_ORDER[k]], 3);
        for (uint32_t k = 0; k < ncgn;) {
            const uint32_t w = L.codegen[k++];
            df_put(S, L.cgcode[w], L.cglen[w]);
            if (w == 16) df_put(S, L.codegen[k++], 2);
            else if (w == 17) df_put(S, L.codegen[k++], 3);
            else if (w == 18) df_put(S, L.codegen[k++], 7);
        }
    }
    df_close(S);
    bit = df_tell(S);
    // ---- the block's bytes ----
    if (huff) {
        const uint32_t span = (n + 63) / 64;
        const uint32_t a = (uint32_t)lane * span < n ? (uint32_t)lane * span : n;
        const uint32_t e = a + span < n ? a + span : n;
        uint32_t mybits = 0;
        uint32_t k = a;
        for (; k + 4 <= e; k += 4) {
            const uint32_t w = ld32(s + k);
            mybits += (L.tab[w & 0xFF] >> 16) + (L.tab[(w >> 8) & 0xFF] >> 16) + (L.tab[(w >> 16) & 0xFF] >> 16) + (L.tab[w >> 24] >> 16);
        }
        for (; k < e; k++) mybits += L.tab[s[k]] >> 16;
        const uint32_t incl = wave_incl_scan(mybits, lane);
        const uint32_t total = rdlane32(incl, 63);
        DfSink B = S;
        B.live = true;
        df_seek(B, bit + (incl - mybits));
        k = a;
        for (; k + 4 <= e; k += 4) {
            const uint32_t w = ld32(s + k);
            uint32_t t = L.tab[w & 0xFF]; df_put(B, t & 0xFFFFu, t >> 16);
            t = L.tab[(w >> 8) & 0xFF]; df_put(B, t & 0xFFFFu, t >> 16);
            t = L.tab[(w >> 16) & 0xFF]; df_put(B, t & 0xFFFFu, t >> 16);
            t = L.tab[w >> 24]; df_put(B, t & 0xFFFFu, t >> 16);
        }
        for (; k < e; k++) { const uint32_t t = L.tab[s[k]]; df_put(B, t & 0xFFFFu, t >> 16); }
        df_close(B);
        bit += total;
    } else if (n) {  // the raw bytes from a byte position: whole words of dst, the two at the ends ORed in
        const uint64_t d0 = bit >> 3, d1 = d0 + n;  // bytes from W
        DfSink B = S;
        B.live = true;
        for (uint64_t w = (d0 >> 2) + (uint64_t)lane; w * 4 < d1; w += 64) {
            uint32_t v = 0;
            const uint64_t b0 = w * 4;
            const bool whole = b0 >= d0 && b0 + 4 <= d1;
            if (whole) v = ld32(s + (b0 - d0));
            else for (uint32_t j = 0; j < 4; j++) if (b0 + j >= d0 && b0 + j < d1) v |= (uint32_t)s[b0 + j - d0] << (8 * j);
            if (whole) B.W[w] = v;
            else df_word_or(B, w, v);
        }
        bit += (uint64_t)n * 8;
    }
    // ---- what comes behind them ----
    df_seek(S, bit);
    if (flags & KCDF_F_SYNC) df_put(S, L.tab[256] & 0xFFFFu, L.tab[256] >> 16);
    if (flags & KCDF_F_LAST) {
        if (P.end == KCDF_END_CLOSE) {  // writeStoredHeader(0, true): the fixed block's header and its EOB (:513-518)
            df_put(S, 3, 3); df_put(S, 0, 7);
            df_pad_to_byte(S);
            if (P.gzip) { df_put(S, P.crc[sp.input], 32); df_put(S, (uint32_t)(P.in_off[sp.input + 1] - P.in_off[sp.input]), 32); }
        } else {  // writeStoredHeader(0, false): 00 00 ff ff from the next byte
            df_put(S, 0, 3);
            df_pad_to_byte(S);
            df_put(S, 0, 16); df_put(S, 0xFFFFu, 16);
        }
    }
    df_close(S);
}

// the bytes of dst in the two edge words (DfSink)
__global__ __launch_bounds__(64) void kc_deflate_edges_kernel(KcDeflateParams P) {
    const uint32_t t = threadIdx.x;
    if (t >= 8) return;
    const uint64_t mis = (uint64_t)(uintptr_t)P.dst & 3u;
    const uint64_t elo = mis ? 0 : UINT64_MAX, ehi = ((mis + P.total) & 3u) ? (mis + P.total) >> 2 : UINT64_MAX;
    const uint32_t which = t >> 2, j = t & 3u;
    const uint64_t w = which ? ehi : elo;
    if (w == UINT64_MAX || (which && ehi == elo)) return;
    const uint64_t byte = w * 4 + j;  // from dst - mis
    if (byte < mis || byte >= mis + P.total) return;
    P.dst[byte - mis] = (uint8_t)(P.edge[which] >> (8 * j));
}

void kc_launch_deflate_plan(const KcDeflateParams& P, hipStream_t st) {
    if (P.nblocks == 0) return;
    hipLaunchKernelGGL(kc_deflate_plan_kernel, dim3(P.nblocks), dim3(64), 0, st, P);
}
void kc_launch_deflate_chain(const KcDeflateParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_deflate_chain_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_deflate_emit(const KcDeflateParams& P, hipStream_t st) {
    if (P.nblocks == 0) return;
    hipLaunchKernelGGL(kc_deflate_emit_kernel, dim3(P.nblocks), dim3(64), 0, st, P);
    hipLaunchKernelGGL(kc_deflate_edges_kernel, dim3(1), dim3(64), 0, st, P);
}
