// kc_flate_stateless.hip — flate.StatelessDeflate / gzip.NewWriterLevel(w, gzip.StatelessCompression) over a batch of independent inputs:
// FOUR LAUNCHES, cut by the reference's own blocks (32767 - len(dict) bytes, then 24575 behind 8192 of history), all blocks of all
// inputs in one grid (kc_stateless_dev.h has the plan; the host sequence is kc_stateless_host.h's).
//
//   match  one wave per block: statelessEnc.  The 8192-entry table lives in LDS (16 KiB) and is cleared per block; the walk is the
//          reference's, sequential, every lane following it and lane 0 writing the table; match extension runs over the lanes
//          (wave_matchlen / wave_backlen); literal runs go to the token scratch 64 at a time.  Tokens to scratch, the three
//          histograms and n into the block's record.
//   plan   one wave per block: the class; for a dynamic block its two tables (generate), the codegen over both alphabets, the
//          code-length code, headerSize, its bits under its own tables, extraBitSize, fixedSize, EstimatedBits; for a Huffman-only
//          block what kc_deflate_plan_kernel computes
//   chain  one wave per input, blocks in order: lastHeader, lastHuffMan, the table in force, canReuse, reuse against the penalised
//          estimate, fixed, stored, the owed EOBs, sync / eof on the last block, the stream's end; gzip: the input's CRC-32
//   emit   one wave per block: owed EOB, header, the tokens (lanes take contiguous spans, a wave scan of the spans' bit lengths
//          places them) or the bytes, EOB, and behind an input's last block the stream's end and gzip's trailer
//
// dst is zeroed by the host sequence and every seam is ORed in (DfSink), as in kc_flate_deflate.hip.  With a dictionary, a launch in
// front (gather) lays the dictionary and every input's first block side by side in scratch, so that the match kernel reads one buffer.
#include "kc_stateless_dev.h"
#include "kc_flate_dev.h"

__global__ __launch_bounds__(64) void kc_stateless_gather_kernel(KcStatelessParams P) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= P.n) return;
    const uint64_t begin = P.in_off[i], len = P.in_off[i + 1] - begin;
    const uint32_t first = KCSL_MAX_BLOCK - P.dict_len;
    const uint32_t n = (uint32_t)(len < first ? len : first);
    uint8_t* out = P.comb + (uint64_t)i * KCSL_COMB;
    for (uint32_t k = lane; k < P.dict_len; k += 64) out[k] = P.dict[k];
    for (uint32_t k = lane; k < n; k += 64) out[P.dict_len + k] = P.src[begin + k];
}

struct SlMatchLds {
    uint16_t table[8192];
    uint32_t hist[320];
};

__global__ __launch_bounds__(64) void kc_stateless_match_kernel(KcStatelessParams P) {
    __shared__ SlMatchLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= P.nblocks) return;
    const SlSpan sp = sl_span(P, r);
    KcSlBlock& R = P.rec[r];
    // src[0, total): the history (the dictionary, or the 8192 bytes of the input in front of the block) and the block, which starts at `start`
    const uint8_t* src;
    int start;
    if (sp.idx != 0) { src = P.src + sp.begin + sp.pos - KCSL_MAX_DICT; start = (int)KCSL_MAX_DICT; }
    else if (P.dict_len) { src = P.comb + (uint64_t)sp.input * KCSL_COMB; start = (int)P.dict_len; }
    else { src = P.src + sp.begin; start = 0; }
    const int total = start + (int)sp.n;
    uint32_t* tok = P.tok + P.tok0[r];
    uint32_t ntok = 0;
    for (int k = lane; k < 320; k += 64) L.hist[k] = 0;
    auto tab_get = [&](uint32_t h) -> int { return (int)uniu(L.table[h]); };
    auto tab_set = [&](uint32_t h, int v) { if (lane == 0) L.table[h] = (uint16_t)v; };
    auto literals = [&](int from, int to) {  // emitLiteral: src[from, to)
        for (int k = from + lane; k < to; k += 64) {
            const uint32_t v = src[k];
            tok[ntok + (uint32_t)(k - from)] = v;
            atomicAdd(&L.hist[v], 1u);
        }
        ntok += (uint32_t)(to - from);
    };
    // The reference keeps its positions in int16 and tests nextS <= 0 for the wrap.  32-bit positions are equivalent: total is at most
    // 32767, so a value that would have wrapped is also above sLimit.
    if (total - start >= 13) {  // minNonLiteralBlockSize (:190)
        for (int k = lane; k < 8192; k += 64) L.table[k] = 0;
        KC_WAVE_SYNC();
        // index until startAt (:197-203): table[hash(src[i, i+4))] = i for i ascending.  64 at a time; where lanes of one store meet in
        // a slot the hardware keeps any one of them, so a lane whose position is above what stands there writes again
        for (int base = 0; base < start; base += 64) {
            const int i = base + lane;
            bool on = i < start;
            const uint32_t h = on ? sl_hash(ld32(src + i)) : 0u;
            for (;;) {
                if (on) L.table[h] = (uint16_t)i;
                KC_WAVE_SYNC();
                on = on && (int)L.table[h] < i;
                if (!ballot64(on)) break;
            }
        }
        KC_WAVE_SYNC();
        int s = start + 1, nextEmit = start;
        const int sLimit = total - 11;  // inputMargin
        uint32_t cv = ld32(src + s);
        bool run = true;
        while (run) {
            const int skipLog = 5, doEvery = 2;
            int nextS = s, cand = 0;
            bool found = false;
            for (;;) {
                uint32_t h = sl_hash(cv);
                cand = tab_get(h);
                nextS = s + doEvery + ((s - nextEmit) >> skipLog);
                if (nextS > sLimit) break;  // emitRemainder
                uint64_t now = ld64(src + nextS);
                tab_set(h, s);
                h = sl_hash((uint32_t)now);
                if (cv == ld32(src + cand)) { tab_set(h, nextS); found = true; break; }
                // do one right away
                cv = (uint32_t)now;
                s = nextS;
                nextS++;
                cand = tab_get(h);
                now >>= 8;
                tab_set(h, s);
                if (cv == ld32(src + cand)) { tab_set(h, nextS); found = true; break; }
                cv = (uint32_t)now;
                s = nextS;
            }
            if (!found) break;
            for (;;) {
                int t = cand;
                int l = wave_matchlen(src + s + 4, src + t + 4, total - (s + 4), lane) + 4;
                const int kmax = t < s - nextEmit ? t : s - nextEmit;  // t > 0 && s > nextEmit
                const int back = kmax > 0 ? wave_backlen(src, s, t, kmax, lane) : 0;
                s -= back; t -= back; l += back;
                if (nextEmit < s) literals(nextEmit, s);
                {   // AddMatchLong(l, s - t - 1), token.go:284-309
                    const uint32_t xoff = (uint32_t)(s - t - 1), oc = sl_offset_code(xoff);
                    int left = l;
                    while (left > 0) {
                        int xl = left;
                        if (xl > 258) xl = xl > 258 + 3 ? 258 : 258 - 3;
                        left -= xl;
                        xl -= 3;
                        if (lane == 0) {
                            atomicAdd(&L.hist[257 + sl_length_code((uint32_t)xl)], 1u);
                            atomicAdd(&L.hist[288 + oc], 1u);
                            tok[ntok] = KCSL_MATCH | (uint32_t)xl << 22 | oc << 16 | xoff;
                        }
                        ntok++;
                    }
                }
                s += l;
                nextEmit = s;
                if (nextS >= s) s = nextS + 1;
                if (s >= sLimit) { run = false; break; }
                uint64_t x = ld64(src + s - 2);
                const int o = s - 2;
                tab_set(sl_hash((uint32_t)x), o);
                x >>= 16;
                const uint32_t h = sl_hash((uint32_t)x);
                cand = tab_get(h);
                tab_set(h, o + 2);
                if ((uint32_t)x != ld32(src + cand)) { cv = (uint32_t)(x >> 8); s++; break; }
            }
        }
        if (nextEmit < total && ntok != 0) literals(nextEmit, total);  // "if nothing was added, don't encode literals"
    }
    KC_WAVE_SYNC();
    for (int k = lane; k < 320; k += 64) R.hist[k] = (uint16_t)L.hist[k];
    if (lane == 0) R.ntok = ntok;
}

struct SlPlanLds {
    uint32_t freq[320];   // KcSlBlock::hist's layout
    DfGenLds G;
    uint8_t len[288], olen[32];
    uint16_t code[288], ocode[32];
    uint8_t codegen[320];
    uint32_t cgfreq[20];
    uint8_t cglen[20];
    uint16_t cgcode[20];
    uint32_t flag, n_codegen, num_lit, num_off;
};

__global__ __launch_bounds__(64) void kc_stateless_plan_kernel(KcStatelessParams P) {
    __shared__ SlPlanLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= P.nblocks) return;
    const SlSpan sp = sl_span(P, r);
    const uint32_t n = sp.n;
    KcSlBlock& R = P.rec[r];
    const uint32_t ntok = uniu(R.ntok);
    const bool last = sp.idx + 1 == sp.nblk;
    const uint32_t cls = n == 0 ? KCSL_C_NONE : ntok == 0 ? KCSL_C_STORED : ntok > n - (n >> 4) ? KCSL_C_HUFF : KCSL_C_DYN;
    if (lane == 0) { R.cls = cls; R.quick = 0; }
    if (cls == KCSL_C_NONE || cls == KCSL_C_STORED) return;
    int nlit, noff;
    if (cls == KCSL_C_HUFF) {  // writeBlockHuff's own part, as kc_deflate_plan_kernel has it
        const uint8_t* s = P.src + sp.begin + sp.pos;
        for (int k = lane; k < 320; k += 64) L.freq[k] = 0;
        KC_WAVE_SYNC();
        for (uint32_t k = (uint32_t)lane * 4; k + 4 <= n; k += 256) {
            const uint32_t w = ld32(s + k);
            atomicAdd(&L.freq[w & 0xFF], 1u);
            atomicAdd(&L.freq[(w >> 8) & 0xFF], 1u);
            atomicAdd(&L.freq[(w >> 16) & 0xFF], 1u);
            atomicAdd(&L.freq[w >> 24], 1u);
        }
        if ((uint32_t)lane < (n & 3u)) atomicAdd(&L.freq[s[(n & ~3u) + (uint32_t)lane]], 1u);
        KC_WAVE_SYNC();
        for (int k = lane; k < 256; k += 64) R.hist[k] = (uint16_t)L.freq[k];
        if (lane == 0) {  // the quick check (:1012-1033), exact in integers: sum (256 v - n)^2 < 2 n 65536
            uint32_t quick = 0;
            if (n > 1024) {
                uint64_t acc = 0;
                for (int k = 0; k < 256; k++) {
                    const int64_t d = (int64_t)256 * (int64_t)L.freq[k] - (int64_t)n;
                    acc += (uint64_t)(d * d);
                }
                quick = acc < (uint64_t)2 * n * 65536u;
            }
            L.flag = quick;
            L.freq[256] = 1;
            L.olen[0] = 1;  // huffOffset: one offset code of length 1
        }
        KC_WAVE_SYNC();
        const uint32_t quick = L.flag;
        if (lane == 0) R.quick = quick;
        if (quick) return;
        nlit = 257; noff = 1;
        df_generate(L.freq, 257, 15, L.G, L.len, L.code, lane);
    } else {  // indexTokens(t, true), :784-815, and generate, :817-820
        for (int k = lane; k < 320; k += 64) L.freq[k] = R.hist[k];
        KC_WAVE_SYNC();
        if (lane == 0) {
            L.freq[256] = 1;
            uint32_t a = 286, b = 30;
            while (L.freq[a - 1] == 0) a--;
            while (b > 0 && L.freq[288 + b - 1] == 0) b--;
            if (b == 0) { L.freq[288] = 1; b = 1; }
            L.num_lit = a; L.num_off = b;
            R.hist[256] = 1;
            R.hist[288] = (uint16_t)L.freq[288];
        }
        KC_WAVE_SYNC();
        nlit = (int)L.num_lit; noff = (int)L.num_off;
        df_generate(L.freq, 286, 15, L.G, L.len, L.code, lane);
        df_generate(L.freq + 288, 30, 15, L.G, L.olen, L.ocode, lane);
    }
    uint32_t bits = 0, extra = 0, fixed = 0;
    for (int k = lane; k < (cls == KCSL_C_HUFF ? 257 : 286); k += 64) {
        const uint32_t f = L.freq[k];
        bits += f * L.len[k];
        fixed += f * (sl_fixed_lit((uint32_t)k) >> 16);
        if (k > 256) extra += f * sl_length_extra((uint32_t)k - 257);
    }
    if (cls == KCSL_C_DYN && lane < 30) {
        const uint32_t f = L.freq[288 + lane];
        bits += f * L.olen[lane];
        fixed += f * 5;
        extra += f * sl_offset_extra((uint32_t)lane);
    }
    const uint32_t self_bits = wave_reduce_sum(bits);
    const uint32_t extra_bits = wave_reduce_sum(extra);
    const uint32_t fixed_bits = 3 + wave_reduce_sum(fixed) + extra_bits;
    if (lane == 0) {
        L.n_codegen = sl_codegen(L.len, nlit, L.olen, noff, L.codegen, L.cgfreq);
        R.est_bits = cls == KCSL_C_DYN ? sl_estimated_bits(L.freq, ntok + (last ? 1u : 0u)) : 0u;
    }
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
        R.num_lit = (uint32_t)nlit;
        R.num_off = (uint32_t)noff;
        R.self_bits = self_bits;
        R.extra_bits = extra_bits;
        R.fixed_bits = fixed_bits;
    }
    const uint32_t ncgn = L.n_codegen;
    for (int k = lane; k < 288; k += 64) { const bool in = k < (cls == KCSL_C_HUFF ? 257 : 286); R.len[k] = in ? L.len[k] : 0; R.code[k] = in ? L.code[k] : 0; }
    if (lane < 32) { const bool in = cls == KCSL_C_DYN && lane < 30; R.olen[lane] = in ? L.olen[lane] : 0; R.ocode[lane] = in ? L.ocode[lane] : 0; }
    for (uint32_t k = (uint32_t)lane; k < ncgn; k += 64) R.codegen[k] = L.codegen[k];
    if (lane < 19) { R.cglen[lane] = L.cglen[lane]; R.cgcode[lane] = L.cgcode[lane]; }
}

struct SlChainLds { uint32_t crcT[4][256], crcM[32], crcP[64]; };

__global__ __launch_bounds__(64) void kc_stateless_chain_kernel(KcStatelessParams P) {
    __shared__ SlChainLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    const uint32_t r0 = P.blk0[i], nblk = P.blk0[i + 1] - r0;
    const uint64_t begin = P.in_off[i], len = P.in_off[i + 1] - begin;
    const bool eof = P.eof != 0 && P.gzip == 0;
    uint32_t last_header = 0, table = 0;
    bool last_huffman = false;
    uint64_t bit = 0;
    auto count = [&](int which) { if (lane == 0) atomicAdd(&P.counts[which], 1u); };
    for (uint32_t b = 0; b < nblk; b++) {
        KcSlBlock& R = P.rec[r0 + b];
        const uint32_t cls = uniu(R.cls);
        if (cls == KCSL_C_NONE) {
            if (lane == 0) { R.how = KCSL_W_NONE; R.flags = KCSL_F_LAST; R.table = 0; R.prev_table = 0; R.start_bit = 0; }
            break;
        }
        const uint32_t first = KCSL_MAX_BLOCK - P.dict_len;
        const uint64_t pos = b == 0 ? 0 : first + (uint64_t)(b - 1) * KCSL_LATER;
        const uint32_t most = b == 0 ? first : KCSL_LATER;
        const uint32_t n = (uint32_t)(len - pos < most ? len - pos : most);
        const bool last = b + 1 == nblk, is_eof = eof && last, sync = last;
        const uint32_t ssize = (n + 5) * 8;
        uint32_t how = KCSL_W_NONE, flags = last ? KCSL_F_LAST : 0u;
        const uint32_t prev = table;
        const uint64_t start = bit;
        auto owed = [&]() {  // the EOB owed to the table in force
            if (last_header) { flags |= KCSL_F_OWED; bit += P.rec[table].len[256]; last_header = 0; }
        };
        auto stored = [&]() {  // writeStoredHeader(n, isEof) + writeBytes: an owed EOB, 3 bits, to the byte, LEN NLEN, the bytes
            owed();
            if (is_eof) flags |= KCSL_F_FINAL;
            bit += 3;
            bit = (bit + 7) & ~(uint64_t)7;
            bit += 32 + (uint64_t)n * 8;
            how = KCSL_W_STORED;
        };
        auto fixed = [&]() {  // writeFixedHeader(isEof), the tokens and an EOB under the fixed tables: fixedSize(extraBits) bits
            owed();
            if (is_eof) flags |= KCSL_F_FINAL;
            flags |= KCSL_F_EOB;
            bit += uniu(R.fixed_bits);
            how = KCSL_W_FIXED;
            count(KCSL_N_DYN_FIXED);
        };
        if (cls == KCSL_C_STORED) {
            count(KCSL_N_STORED_NO_MATCH);
            stored();
        } else if (cls == KCSL_C_HUFF) {  // writeBlockHuff(isEof, uncompressed, sync), :987-1174
            count(KCSL_N_HUFFMAN_ONLY);
            uint32_t est = 0;
            bool st = uniu(R.quick) != 0;
            if (st) count(KCSL_N_H_QUICK);
            else {
                est = uniu(R.self_bits) + last_header;
                if (last_header == 0) est += KCDF_GUESS_HEADER_BITS;
                est += est >> P.penalty;
                if (ssize <= est) { st = true; count(KCSL_N_H_EST); }
            }
            if (st) stored();
            else {
                uint32_t body = 0;
                if (last_header) {  // canReuseBits of the table in force over literalFreq[:256] (:1055-1068)
                    const KcSlBlock& T = P.rec[table];
                    uint32_t sum = 0;
                    bool missing = false;
                    for (int k = lane; k < 256; k += 64) {
                        const uint32_t f = R.hist[k], l = T.len[k];
                        missing |= f && !l;
                        sum += f * l;
                    }
                    sum = wave_reduce_sum(sum);
                    const bool none = ballot64(missing) != 0;
                    const uint32_t reuse = none ? (uint32_t)DF_MAXI32 : sum;
                    if (est < reuse) {
                        count(KCSL_N_H_NEW_OWED);
                        if (none) count(KCSL_N_H_NOT_REUSABLE);
                        owed();
                    } else {
                        count(KCSL_N_H_REUSE);
                        body = sum;
                    }
                } else {
                    count(KCSL_N_H_FIRST);
                }
                if (last_header == 0) {
                    table = r0 + b;
                    last_header = uniu(R.hdr_bits);
                    bit += last_header;
                    body = uniu(R.self_bits) - R.len[256];
                    flags |= KCSL_F_HEADER | (is_eof ? KCSL_F_FINAL : 0u);
                    last_huffman = true;
                }
                bit += body;
                how = KCSL_W_BYTES;
                if (is_eof || sync) {
                    flags |= KCSL_F_EOB;
                    bit += P.rec[table].len[256];
                    last_header = 0;
                    last_huffman = false;
                }
            }
        } else {  // writeBlockDynamic(dst, isEof, uncompressed, sync), :620-765
            const uint32_t ntok = uniu(R.ntok) + (sync ? 1u : 0u);  // tokens.AddEOB
            if ((last_huffman || is_eof) && last_header) { owed(); last_huffman = false; }
            uint32_t reuse = 0;
            if (last_header) {  // canReuse (:163-190) and dynamicReuseSize (:371-375) under the table in force
                const KcSlBlock& T = P.rec[table];
                uint32_t sum = 0;
                bool missing = false;
                for (int k = lane; k < 320; k += 64) {
                    const uint32_t f = R.hist[k], l = k < 288 ? T.len[k] : T.olen[k - 288];
                    missing |= f && !l;
                    sum += f * l;
                }
                reuse = wave_reduce_sum(sum);
                if (ballot64(missing) != 0) { count(KCSL_N_CANNOT_REUSE); owed(); }
            }
            const bool first_table = last_header == 0;
            const uint32_t extra = uniu(R.extra_bits), fixed_bits = uniu(R.fixed_bits);
            bool done = false;
            if (last_header) {
                uint32_t new_size = last_header + uniu(R.est_bits);
                new_size += P.rec[table].len[256] + (new_size >> P.penalty);
                const uint32_t reuse_size = reuse + extra;
                uint32_t size;
                if (new_size < reuse_size) { count(KCSL_N_DYN_NEW_OWED); owed(); size = new_size; }
                else size = reuse_size;
                if (ntok < KCSL_PREDEF && fixed_bits + 7 < size) {
                    if (ssize <= size) { count(KCSL_N_DYN_STORED); stored(); } else fixed();
                    done = true;
                } else if (ssize <= size) { count(KCSL_N_DYN_STORED); stored(); done = true; }
            }
            if (!done && last_header == 0) {  // a new table
                const uint32_t size = uniu(R.hdr_bits) + uniu(R.self_bits) + extra;  // dynamicSize
                if (ntok < KCSL_PREDEF && fixed_bits <= size) {
                    if (ssize <= fixed_bits) { count(KCSL_N_DYN_STORED); stored(); } else fixed();
                    done = true;
                } else if (ssize <= size) { count(KCSL_N_DYN_STORED); stored(); done = true; }
                else {
                    if (first_table) count(KCSL_N_DYN_FIRST);
                    flags |= KCSL_F_HEADER | (is_eof ? KCSL_F_FINAL : 0u);
                    bit += uniu(R.hdr_bits);
                    table = r0 + b;
                    reuse = uniu(R.self_bits);
                    if (!sync) last_header = uniu(R.hdr_bits);
                    last_huffman = false;
                }
            } else if (!done) {
                count(KCSL_N_DYN_REUSE);
            }
            if (!done) {  // writeTokens under the table in force: its codes without the EOB counted in, the extra bits, the EOB with sync
                bit += reuse - P.rec[table].len[256] + extra;
                if (sync) { flags |= KCSL_F_EOB; bit += P.rec[table].len[256]; last_header = 0; }
                how = KCSL_W_TOKENS;
            }
        }
        if (lane == 0) { R.how = how; R.flags = flags; R.table = table; R.prev_table = prev; R.start_bit = start; }
    }
    // The stream's end.  Nothing is owed here: an input's last block went out with sync.  An eof call on nothing is the ten-bit fixed
    // block alone (:84-90); a non-eof call ends with the empty stored block (:156-159); then flush.
    if (eof) { if (len == 0) bit += 10; }
    else {
        bit += 3;
        bit = (bit + 7) & ~(uint64_t)7;
        bit += 32;
    }
    bit = (bit + 7) & ~(uint64_t)7;
    uint64_t bytes = bit >> 3;
    if (P.gzip) {  // the header in front; Close: StatelessDeflate(nil, true) = 03 00, CRC-32, ISIZE
        bytes += 10 + 2 + 8;
        fl_crc_tables(L.crcT, lane);
        const uint8_t* s = P.src + begin;
        auto rd32 = [&](int k) -> uint32_t { return ld32(s + k); };
        auto rdb = [&](int k) -> uint32_t { return s[k]; };
        const uint32_t c = s2_crc32c_wave(rd32, rdb, (int)len, L.crcT, L.crcM, L.crcP, lane);
        if (lane == 0) P.crc[i] = c;
    }
    if (lane == 0) P.size[i] = bytes;
}

struct SlEmitLds {
    uint32_t tab[288], otab[32];  // code | len << 16 of the tables the block is written under
    uint8_t codegen[320];
    uint16_t cgcode[20];
    uint8_t cglen[20];
};

// the bits of one token under the tables in LDS: the literal / length code with the length's extra bits, the offset code with its
__device__ __forceinline__ void sl_token_fields(const SlEmitLds& L, const uint32_t t, uint32_t& v1, uint32_t& n1, uint32_t& v2, uint32_t& n2) {
    if (t < KCSL_MATCH) {
        const uint32_t e = L.tab[t];
        v1 = e & 0xFFFFu; n1 = e >> 16; v2 = 0; n2 = 0;
        return;
    }
    const uint32_t xl = (t >> 22) & 0xFFu, lc = sl_length_code(xl), le = sl_length_extra(lc);
    const uint32_t oc = (t >> 16) & 31u, oe = sl_offset_extra(oc), xoff = t & 0xFFFFu;
    const uint32_t a = L.tab[257 + lc], b = L.otab[oc];
    n1 = a >> 16;
    v1 = (a & 0xFFFFu) | (xl & ((1u << le) - 1)) << n1;
    n1 += le;
    n2 = b >> 16;
    v2 = (b & 0xFFFFu) | (xoff & ((1u << oe) - 1)) << n2;
    n2 += oe;
}

__global__ __launch_bounds__(64) void kc_stateless_emit_kernel(KcStatelessParams P) {
    __shared__ SlEmitLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t r = blockIdx.x;
    if (r >= P.nblocks) return;
    const SlSpan sp = sl_span(P, r);
    const uint32_t n = sp.n;
    const uint8_t* s = P.src + sp.begin + sp.pos;
    const KcSlBlock& R = P.rec[r];
    const uint32_t how = uniu(R.how), flags = uniu(R.flags);
    const bool eof = P.eof != 0 && P.gzip == 0;

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

    if (how == KCSL_W_TOKENS || how == KCSL_W_BYTES) {
        const KcSlBlock& T = P.rec[uniu(R.table)];
        for (int k = lane; k < 288; k += 64) L.tab[k] = (uint32_t)T.code[k] | (uint32_t)T.len[k] << 16;
        if (lane < 32) L.otab[lane] = (uint32_t)T.ocode[lane] | (uint32_t)T.olen[lane] << 16;
    } else if (how == KCSL_W_FIXED) {
        for (int k = lane; k < 288; k += 64) L.tab[k] = sl_fixed_lit((uint32_t)k);
        if (lane < 32) L.otab[lane] = sl_fixed_off((uint32_t)lane);
    }
    if (flags & KCSL_F_HEADER) {
        const uint32_t ncgn = uniu(R.n_codegen);
        for (uint32_t k = (uint32_t)lane; k < ncgn; k += 64) L.codegen[k] = R.codegen[k];
        if (lane < 19) { L.cglen[lane] = R.cglen[lane]; L.cgcode[lane] = R.cgcode[lane]; }
    }
    KC_WAVE_SYNC();
    // ---- what comes before the block's codes: every lane follows the position, lane 0 writes ----
    if (sp.idx == 0 && P.gzip) {  // 1f 8b 08 00 | MTIME 0 | XFL 0, OS 255 (gzip/gzip.go: the default Header at this level)
        df_seek(S, in0);
        df_put(S, 0x00088b1fu, 32); df_put(S, 0, 32); df_put(S, 0xff00u, 16);
        df_close(S);
    }
    df_seek(S, bit);
    const uint32_t fin = (flags & KCSL_F_FINAL) ? 1u : 0u;
    if (flags & KCSL_F_OWED) {
        const KcSlBlock& O = P.rec[uniu(R.prev_table)];
        df_put(S, O.code[256], O.len[256]);
    }
    if (how == KCSL_W_STORED) {  // writeStoredHeader(n, isEof): :521-528
        df_put(S, fin, 3);
        df_pad_to_byte(S);
        df_put(S, n, 16);
        df_put(S, ~n & 0xFFFFu, 16);
    } else if (how == KCSL_W_FIXED) {  // writeFixedHeader(isEof): :541-546
        df_put(S, 2 + fin, 3);
    } else if (flags & KCSL_F_HEADER) {  // writeDynamicHeader(numLiterals, numOffsets, numCodegens, isEof): :458-497
        const uint32_t ncg = uniu(R.ncg), ncgn = uniu(R.n_codegen);
        df_put(S, 4 + fin, 3); df_put(S, uniu(R.num_lit) - 257, 5); df_put(S, uniu(R.num_off) - 1, 5); df_put(S, ncg - 4, 4);
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
    // ---- the block itself ----
    if (how == KCSL_W_TOKENS || how == KCSL_W_FIXED) {  // writeTokens, :824-975
        const uint32_t* tok = P.tok + P.tok0[r];
        const uint32_t ntok = uniu(R.ntok);
        const uint32_t span = (ntok + 63) / 64;
        const uint32_t a = (uint32_t)lane * span < ntok ? (uint32_t)lane * span : ntok;
        const uint32_t e = a + span < ntok ? a + span : ntok;
        uint32_t mybits = 0;
        for (uint32_t k = a; k < e; k++) {
            uint32_t v1, n1, v2, n2;
            sl_token_fields(L, tok[k], v1, n1, v2, n2);
            mybits += n1 + n2;
        }
        const uint32_t incl = wave_incl_scan(mybits, lane);
        const uint32_t total = rdlane32(incl, 63);
        DfSink B = S;
        B.live = true;
        df_seek(B, bit + (incl - mybits));
        for (uint32_t k = a; k < e; k++) {
            uint32_t v1, n1, v2, n2;
            sl_token_fields(L, tok[k], v1, n1, v2, n2);
            df_put(B, v1, n1);
            df_put(B, v2, n2);
        }
        df_close(B);
        bit += total;
    } else if (how == KCSL_W_BYTES) {
        const uint32_t span = (n + 63) / 64;
        const uint32_t a = (uint32_t)lane * span < n ? (uint32_t)lane * span : n;
        const uint32_t e = a + span < n ? a + span : n;
        uint32_t mybits = 0;
        for (uint32_t k = a; k < e; k++) mybits += L.tab[s[k]] >> 16;
        const uint32_t incl = wave_incl_scan(mybits, lane);
        const uint32_t total = rdlane32(incl, 63);
        DfSink B = S;
        B.live = true;
        df_seek(B, bit + (incl - mybits));
        for (uint32_t k = a; k < e; k++) { const uint32_t t = L.tab[s[k]]; df_put(B, t & 0xFFFFu, t >> 16); }
        df_close(B);
        bit += total;
    } else if (how == KCSL_W_STORED && n) {  // the raw bytes from a byte position: whole words of dst, the two at the ends ORed in
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
    // ---- what comes behind it ----
    df_seek(S, bit);
    if (flags & KCSL_F_EOB) df_put(S, L.tab[256] & 0xFFFFu, L.tab[256] >> 16);
    if (flags & KCSL_F_LAST) {
        if (!eof) {  // writeStoredHeader(0, false): 00 00 ff ff from the next byte
            df_put(S, 0, 3);
            df_pad_to_byte(S);
            df_put(S, 0, 16); df_put(S, 0xFFFFu, 16);
        } else if (how == KCSL_W_NONE) {  // writeStoredHeader(0, true): the fixed block's header and its EOB (:513-518)
            df_put(S, 3, 3); df_put(S, 0, 7);
        }
        df_pad_to_byte(S);
        if (P.gzip) {  // Close: the eof call on nothing, CRC-32, ISIZE
            df_put(S, 3, 3); df_put(S, 0, 7);
            df_pad_to_byte(S);
            df_put(S, P.crc[sp.input], 32);
            df_put(S, (uint32_t)(P.in_off[sp.input + 1] - P.in_off[sp.input]), 32);
        }
    }
    df_close(S);
}

// the bytes of dst in the two edge words (DfSink)
__global__ __launch_bounds__(64) void kc_stateless_edges_kernel(KcStatelessParams P) {
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

void kc_launch_stateless_gather(const KcStatelessParams& P, hipStream_t st) {
    if (P.n == 0 || P.dict_len == 0) return;
    hipLaunchKernelGGL(kc_stateless_gather_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_stateless_match(const KcStatelessParams& P, hipStream_t st) {
    if (P.nblocks == 0) return;
    hipLaunchKernelGGL(kc_stateless_match_kernel, dim3(P.nblocks), dim3(64), 0, st, P);
}
void kc_launch_stateless_plan(const KcStatelessParams& P, hipStream_t st) {
    if (P.nblocks == 0) return;
    hipLaunchKernelGGL(kc_stateless_plan_kernel, dim3(P.nblocks), dim3(64), 0, st, P);
}
void kc_launch_stateless_chain(const KcStatelessParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_stateless_chain_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_stateless_emit(const KcStatelessParams& P, hipStream_t st) {
    if (P.nblocks == 0) return;
    hipLaunchKernelGGL(kc_stateless_emit_kernel, dim3(P.nblocks), dim3(64), 0, st, P);
    hipLaunchKernelGGL(kc_stateless_edges_kernel, dim3(1), dim3(64), 0, st, P);
}
