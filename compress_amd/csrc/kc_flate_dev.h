// kc_flate_dev.h — one DEFLATE stream (and the gzip members around it) decoded by ONE WAVE: the bit reader, the Huffman tables in
// LDS, the block walk and the wave-wide copies, shared by the sizing pass and the write pass of kc_flate_inflate.hip.
//
// Semantics: the decompressor of flate/inflate.go (nextBlock :352-395, readHuffman :464-597, dataBlock / copyData :600-670,
// huffSym :740-783, huffmanDecoder.init :116-176) with the block body of flate/inflate_gen.go:45-270, and gzip.Reader's header,
// trailer and member loop (gzip/gunzip.go:183-295).  The input is untrusted: every read is checked against the input's end and every
// write against the input's own planned range, and all checks of an operation come before any of its writes.
//
// All 64 lanes run the same control flow.  What is read from memory or LDS and steers it goes through v_readfirstlane (uniu), so
// positions, bit buffer, lengths, distances and branches are scalar; the lanes differ only where bytes are moved: literals collect
// one per lane and leave as one store, a match is one byte per lane per round from `d - dist + k % dist` (bytes in front of the
// match, so a match that overlaps itself needs no second pass), stored blocks go 8 bytes per lane.
//
// The reference feeds its bit buffer one byte at a time, and only as many as the shortest code needs (maxRead): whether a short
// input is io.ErrUnexpectedEOF or a CorruptInputError, and how many bytes were read at the end, follows from that.  `gnb` below is
// the reference's f.nb — the bits of the bytes it has read and not used — kept beside the device's own wider buffer.
#pragma once
#include "kc_dev.h"
#include "kc_s2_dev.h"
#include "kc_wave.h"

// per-input verdicts: the KC_FL_* of include/kcgpu.h
#define KCFL_OK 0u
#define KCFL_CORRUPT 1u
#define KCFL_EOF 2u
#define KCFL_HEADER 3u
#define KCFL_CHECKSUM 4u
#define KCFL_SIZE 5u
#define KCFL_DICTIONARY 6u
#define KCFL_RAW_EOF 100u  // internal: the raw io.EOF of inflate_gen.go:114-122, 142-151, 210-219 — ReadAll ends without an error
#define KCFL_OVER 101u     // internal: the next bytes would pass the room the caller gave (O.cap, or KCFL_MAX_OUT without writing): fl_over()
#define KCFL_MAX_OUT ((uint64_t)1 << 30)  // decoded bytes per input this library serves

struct KcFlateParams {
    const uint8_t* src;          // the inputs, concatenated
    const uint64_t* in_off;      // n + 1
    uint32_t n;
    uint32_t gzip;               // 0: raw DEFLATE; 1: gzip members; 2: zlib (KCFL_FMT_*; the flate kernels see 0 or 1 only)
    uint32_t multistream;        // gzip.Reader.Multistream
    const uint8_t* dict;         // the preset dictionary's last dict_len <= 32768 bytes (raw DEFLATE; zlib where the stream has FDICT)
    uint32_t dict_len;
    // sizing pass: written; write pass: read
    uint64_t* size;              // planned bytes: the whole input when it stands, else the gzip members complete in front of the error
    uint32_t* status;            // KCFL_* short of the CRC-32
    uint64_t* consumed;          // input bytes read when the input stands, else 0
    uint32_t* members;           // members to write: gzip's complete ones; raw DEFLATE: 1 when the input stands
    // write pass
    const uint64_t* out0;        // where input i's range starts in dst
    uint8_t* dst;
    uint32_t* wstatus;           // the final verdict of every input the write pass ran for
    uint32_t dict_id;            // zlib: the Adler-32 of the WHOLE preset dictionary (1 without one), what a DICTID is compared with
};
#define KCFL_FMT_FLATE 0u
#define KCFL_FMT_GZIP 1u
#define KCFL_FMT_ZLIB 2u
void kc_launch_flate_size(const KcFlateParams& P, hipStream_t st);
void kc_launch_flate_write(const KcFlateParams& P, hipStream_t st);
void kc_launch_zlib_size(const KcFlateParams& P, hipStream_t st);
void kc_launch_zlib_write(const KcFlateParams& P, hipStream_t st);

#define KCFL_PB_L 10  // primary-table bits: literal/length, distance, code-length codes
#define KCFL_PB_D 9
#define KCFL_PB_C 7

// One code: a primary table over the low `pb` bits (entry = symbol << 4 | length, 0 = not here) and, for longer codes, the canonical
// walk over cnt[] / sym[] (symbols ordered by length, then value).
struct FlTab {
    uint16_t* prim;
    uint16_t* sym;
    uint32_t* cnt;   // [16] codes per length
    uint32_t* aux;   // [32] first code / first index per length (build only)
};
struct FlCode { uint32_t min_len, max_len; };  // max_len 0: the empty code

// the LDS of one wave
struct FlLds {
    uint16_t prim_l[1 << KCFL_PB_L], prim_d[1 << KCFL_PB_D], prim_c[1 << KCFL_PB_C], prim_f[1 << KCFL_PB_L];  // _f: the fixed code
    uint16_t sym_l[288], sym_d[32], sym_c[32], sym_f[288];
    uint32_t cnt[4][16], aux[4][32];
    uint8_t lens[320];
    uint32_t crcT[4][256], crcM[32], crcP[64];
};

// the bit reader: buf holds cnt bits from bitpos on (zero behind the input's end), next is the byte the next refill loads
struct FlBits {
    const uint8_t* src;
    uint64_t end;      // the input's end in src
    uint64_t bitpos;   // absolute bit position in src of the next unused bit
    uint64_t next;
    uint64_t buf;
    uint32_t cnt;
    uint32_t gnb;      // the reference's f.nb
};

__device__ __forceinline__ void fl_seek(FlBits& B, uint64_t byte) {
    B.bitpos = byte * 8; B.next = byte; B.buf = 0; B.cnt = 0; B.gnb = 0;
}
__device__ __forceinline__ uint64_t fl_read_pos(const FlBits& B) { return (B.bitpos + B.gnb) >> 3; }  // the reference's read offset
// at least 32 bits in buf
__device__ __forceinline__ void fl_refill(FlBits& B) {
    if (B.cnt >= 32) return;
    uint32_t w = 0;
    if (B.next + 4 <= B.end) w = ld32(B.src + B.next);
    else
        for (uint32_t k = 0; k < 4 && B.next + k < B.end; k++) w |= (uint32_t)B.src[B.next + k] << (8 * k);
    B.buf |= (uint64_t)uniu(w) << B.cnt;
    B.cnt += 32;
    B.next += 4;
}
// moreBits until f.nb >= n: false when the input ends first (every byte it has is then read)
__device__ __forceinline__ bool fl_need(FlBits& B, uint32_t n) {
    if (B.gnb >= n) return true;
    const uint64_t k = (n - B.gnb + 7) >> 3, have = B.end - fl_read_pos(B);
    if (k > have) { B.gnb += (uint32_t)have * 8; return false; }
    B.gnb += (uint32_t)k * 8;
    return true;
}
__device__ __forceinline__ void fl_drop(FlBits& B, uint32_t n) {
    B.buf >>= n; B.cnt -= n; B.bitpos += n; B.gnb -= n;
}
// n <= 16 bits; false: the input ended
__device__ __forceinline__ bool fl_take(FlBits& B, uint32_t n, uint32_t* v) {
    fl_refill(B);
    if (!fl_need(B, n)) return false;
    *v = (uint32_t)B.buf & ((1u << n) - 1u);
    fl_drop(B, n);
    return true;
}

__device__ __forceinline__ uint32_t fl_rev16(uint32_t v) {  // bits.Reverse16
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
    return ((v >> 8) & 0xFFu) | ((v & 0xFFu) << 8);
}

// huffmanDecoder.init over lens[0, n), n <= 64 * NCHUNK, parallel over the symbols: lane j takes symbols j, j + 64, ...; a ballot
// per code length gives every symbol its rank among the symbols of its length, and the counts.  False: the code is refused
// (neither complete, nor the single code of length 1, nor empty).  All lanes call; lens must be visible (KC_WAVE_SYNC before).
template <int NCHUNK, int PB>
__device__ __forceinline__ bool fl_build(const uint8_t* lens, const uint32_t n, const FlTab T, FlCode* C, const int lane) {
    uint32_t run[16];
    uint32_t myl[NCHUNK], myr[NCHUNK];
#pragma unroll
    for (int l = 0; l < 16; l++) run[l] = 0;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) {
        const uint32_t idx = (uint32_t)c * 64 + (uint32_t)lane;
        const uint32_t l = idx < n ? lens[idx] : 0;
        myl[c] = l;
        myr[c] = 0;
#pragma unroll
        for (int len = 1; len < 16; len++) {
            const uint64_t m = ballot64(l == (uint32_t)len);
            if (l == (uint32_t)len) myr[c] = run[len] + (uint32_t)__popcll(m & below);
            run[len] += (uint32_t)__popcll(m);
        }
    }
    uint32_t mn = 0, mx = 0;
#pragma unroll
    for (int len = 1; len < 16; len++)
        if (run[len]) { if (!mn) mn = len; mx = len; }
    C->min_len = mn;
    C->max_len = mx;
    if (mx == 0) return true;  // empty: whoever reads a symbol through it fails
    uint32_t code = 0, index = 0;
#pragma unroll
    for (int len = 1; len < 16; len++) {
        code <<= 1;
        if (lane == 0) { T.cnt[len] = run[len]; T.aux[len] = code; T.aux[16 + len] = index; }
        code += run[len];
        index += run[len];
        if ((uint32_t)len == mx) break;
    }
    if (code != (1u << mx) && !(code == 1 && mx == 1)) return false;
    for (uint32_t i = (uint32_t)lane; i < (1u << PB); i += 64) T.prim[i] = 0;
    KC_WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) {
        const uint32_t l = myl[c], idx = (uint32_t)c * 64 + (uint32_t)lane;
        if (l) {
            T.sym[T.aux[16 + l] + myr[c]] = (uint16_t)idx;
            if (l <= (uint32_t)PB) {
                const uint32_t r = fl_rev16(T.aux[l] + myr[c]) >> (16 - l);
                for (uint32_t off = r; off < (1u << PB); off += 1u << l) T.prim[off] = (uint16_t)((idx << 4) | l);
            }
        }
    }
    KC_WAVE_SYNC();
    return true;
}

// the code that is a prefix of the bits v (LSB first, zero where the reference has read nothing yet): symbol << 4 | length, or 0
template <int PB>
__device__ __forceinline__ uint32_t fl_lookup(const FlTab T, const FlCode C, const uint32_t v) {
    if (C.max_len == 0) return 0;
    const uint32_t e = uniu((uint32_t)T.prim[v & ((1u << PB) - 1u)]);
    if (e || C.max_len <= (uint32_t)PB) return e;
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= C.max_len; len++) {  // (at most 15 rounds)
        code |= (v >> (len - 1)) & 1u;
        const uint32_t c = uniu(T.cnt[len]);
        if (code < first + c) return (uniu((uint32_t)T.sym[index + (code - first)]) << 4) | len;
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return 0;
}

// huffSym: KCFL_OK and *sym, KCFL_EOF, or KCFL_CORRUPT (a code that is not there)
template <int PB>
__device__ __forceinline__ uint32_t fl_sym(FlBits& B, const FlTab T, const FlCode C, const uint32_t max_read, uint32_t* sym) {
    fl_refill(B);
    uint32_t n = max_read;
    for (int round = 0; round < 17; round++) {  // n grows from round to round and is at most 15 after the first
        if (!fl_need(B, n)) return KCFL_EOF;
        const uint32_t valid = B.gnb >= 32 ? 0xFFFFFFFFu : (1u << B.gnb) - 1u;
        const uint32_t e = fl_lookup<PB>(T, C, (uint32_t)B.buf & valid);
        n = e & 15u;
        if (n <= B.gnb) {
            if (n == 0) return KCFL_CORRUPT;
            fl_drop(B, n);
            *sym = e >> 4;
            return KCFL_OK;
        }
    }
    return KCFL_CORRUPT;
}

// CRC-32 (IEEE, reflected 0xEDB88320) slicing-by-4 tables; all lanes call
__device__ __forceinline__ void fl_crc_tables(uint32_t (*crcT)[256], int lane) {
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        crcT[0][i] = c;
    }
    KC_WAVE_SYNC();
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = crcT[0][i];
        for (int t = 1; t < 4; t++) { c = crcT[0][c & 0xFF] ^ (c >> 8); crcT[t][i] = c; }
    }
    KC_WAVE_SYNC();
}

// the output of one input: dst[0, cap) is its planned range, d what stands so far (pending literals included)
struct FlOut {
    uint8_t* dst;
    uint64_t cap;
    uint64_t d;
    const uint8_t* hist;   // the preset dictionary's tail, hist_len bytes in front of output position 0 of the running stream
    uint32_t hist_len;
    uint64_t base;         // output position where the running stream (gzip member) started: distances do not reach in front of it
    uint32_t nlit;         // literals waiting in the lanes
    uint32_t lit;          // this lane's
};

template <bool WRITE>
__device__ __forceinline__ void fl_flush(FlOut& O, const int lane) {
    if (WRITE && O.nlit) {
        if ((uint32_t)lane < O.nlit) O.dst[O.d - O.nlit + (uint32_t)lane] = (uint8_t)O.lit;
    }
    O.nlit = 0;
}

// what KCFL_OVER is to the flate, gzip and zlib passes: the write pass was planned by the sizing pass, so bytes beyond the plan are a
// broken stream; the sizing pass met the library's limit
template <bool WRITE>
__device__ __forceinline__ uint32_t fl_over(const uint32_t e) { return e == KCFL_OVER ? (WRITE ? KCFL_CORRUPT : KCFL_SIZE) : e; }

// One DEFLATE stream from B on.  KCFL_OK: the final block ended (or the raw io.EOF of the reference's extra-bit reads: what was
// decoded stands); the bit reader is left where the reference's is.  KCFL_OVER: the room ended; nothing is written beyond it.
// AVAIL_FIRST (zip): a stored block that the input's end cuts short is KCFL_OVER where the bytes it HAS pass the room -- the
// reference hands those out before it reports the short read (copyData, inflate.go:634-670) -- and its bytes count towards O.d.
template <bool WRITE, bool AVAIL_FIRST = false>
__device__ __forceinline__ uint32_t fl_inflate(FlBits& B, FlOut& O, FlLds& L, const int lane) {
    const FlTab TL = {L.prim_l, L.sym_l, L.cnt[0], L.aux[0]}, TD = {L.prim_d, L.sym_d, L.cnt[1], L.aux[1]}, TC = {L.prim_c, L.sym_c, L.cnt[2], L.aux[2]};
    const FlTab TF = {L.prim_f, L.sym_f, L.cnt[3], L.aux[3]};
    FlCode CL = {0, 0}, CD = {0, 0}, CC = {0, 0}, CF = {0, 0};
    bool have_fixed = false;  // TF holds the fixed code: built once per stream, at its first fixed block
    const uint64_t limit = WRITE ? O.cap : KCFL_MAX_OUT;
    // every round reads the three header bits of a block or ends the input
    for (;;) {
        uint32_t hdr;
        if (!fl_take(B, 3, &hdr)) return KCFL_EOF;
        const bool final = hdr & 1u;
        const uint32_t typ = hdr >> 1;
        if (typ == 3) return KCFL_CORRUPT;
        if (typ == 0) {  // stored: dataBlock / copyData
            const uint64_t p = (B.bitpos + 7) >> 3;
            if (B.end - p < 4) { fl_seek(B, B.end); return KCFL_EOF; }
            const uint32_t w = uniu(ld32(B.src + p));
            const uint32_t len = w & 0xFFFFu;
            if ((w >> 16) != (len ^ 0xFFFFu)) { fl_seek(B, p + 4); return KCFL_CORRUPT; }
            if (B.end - (p + 4) < len) {
                if (AVAIL_FIRST) {
                    if (B.end - (p + 4) > limit - O.d) return KCFL_OVER;
                    O.d += B.end - (p + 4);  // (handed out by the reference; a failed input's range is zero-filled, so not copied)
                }
                fl_seek(B, B.end);
                return KCFL_EOF;
            }
            if (len > limit - O.d) return KCFL_OVER;
            if (WRITE) {
                fl_flush<WRITE>(O, lane);
                uint8_t* o = O.dst + O.d;
                const uint8_t* a = B.src + p + 4;
                const uint32_t body = len & ~7u;
                for (uint32_t k = (uint32_t)lane * 8; k < body; k += 512) st64(o + k, ld64(a + k));
                for (uint32_t k = body + (uint32_t)lane; k < len; k += 64) o[k] = a[k];
            }
            O.d += len;
            fl_seek(B, p + 4 + len);
            if (final) break;
            continue;
        }
        uint32_t max_read;
        if (typ == 1) {
            if (!have_fixed) {
                KC_WAVE_SYNC();  // (lens is rewritten: the last build's reads are done)
                for (uint32_t i = (uint32_t)lane; i < 288; i += 64) L.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                KC_WAVE_SYNC();
                (void)fl_build<5, KCFL_PB_L>(L.lens, 288, TF, &CF, lane);
                have_fixed = true;
            }
            max_read = 7;
        } else {  // readHuffman
            uint32_t v;
            if (!fl_take(B, 14, &v)) return KCFL_EOF;
            const uint32_t nlit = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, nclen = (v >> 10) + 4;
            if (nlit > 286) return KCFL_CORRUPT;
            if (ndist > 30) return KCFL_CORRUPT;
            KC_WAVE_SYNC();  // (lens is rewritten: the last build's reads are done)
            if (lane < 19) L.lens[lane] = 0;
            KC_WAVE_SYNC();
            for (uint32_t i = 0; i < nclen; i++) {  // 3 bits each
                if (!fl_take(B, 3, &v)) return KCFL_EOF;
                // codeOrder: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const int ord = i < 3 ? (int)(16 + i) : i == 3 ? 0 : (i & 1u) ? (int)(8 - ((i - 3) >> 1)) : (int)(8 + ((i - 4) >> 1));
                if (lane == 0) L.lens[ord] = (uint8_t)v;
            }
            KC_WAVE_SYNC();
            if (!fl_build<1, KCFL_PB_C>(L.lens, 19, TC, &CC, lane)) return KCFL_CORRUPT;
            const uint32_t n = nlit + ndist;
            uint32_t prev = 0;
            // every round reads a code-length symbol (at least one bit) or ends the input
            for (uint32_t i = 0; i < n;) {
                uint32_t x;
                const uint32_t e = fl_sym<KCFL_PB_C>(B, TC, CC, CC.min_len, &x);
                if (e) return e;
                if (x < 16) {
                    if (lane == 0) L.lens[i] = (uint8_t)x;
                    prev = x;
                    i++;
                    continue;
                }
                uint32_t rep, b = 0, nb;
                if (x == 16) {
                    if (i == 0) return KCFL_CORRUPT;
                    rep = 3; nb = 2; b = prev;
                } else if (x == 17) { rep = 3; nb = 3; }
                else { rep = 11; nb = 7; }
                if (!fl_take(B, nb, &v)) return KCFL_EOF;
                rep += v;
                if (i + rep > n) return KCFL_CORRUPT;
                for (uint32_t j = (uint32_t)lane; j < rep; j += 64) L.lens[i + j] = (uint8_t)b;
                prev = b;
                i += rep;
            }
            KC_WAVE_SYNC();
            const uint32_t eob_len = uniu((uint32_t)L.lens[256]);
            const bool okl = fl_build<5, KCFL_PB_L>(L.lens, nlit, TL, &CL, lane);
            const bool okd = fl_build<1, KCFL_PB_D>(L.lens + nlit, ndist, TD, &CD, lane);
            if (!okl || !okd) return KCFL_CORRUPT;
            max_read = CL.min_len > eob_len ? CL.min_len : eob_len;  // inflate.go:582-594
            if (!final) max_read += 10;
        }
        const FlTab TB = typ == 1 ? TF : TL;
        const FlCode CB = typ == 1 ? CF : CL;
        // the block body: every round reads a literal/length symbol (at least one bit) or ends the input
        for (;;) {
            uint32_t v;
            uint32_t e = fl_sym<KCFL_PB_L>(B, TB, CB, max_read, &v);
            if (e) return e;
            if (v < 256) {
                if (O.d >= limit) return KCFL_OVER;
                if (WRITE) {
                    if ((uint32_t)lane == O.nlit) O.lit = v;
                    O.nlit++;
                    O.d++;
                    if (O.nlit == 64) fl_flush<WRITE>(O, lane);
                } else {
                    O.d++;
                }
                continue;
            }
            if (v == 256) break;
            if (v >= 286) return KCFL_CORRUPT;
            uint32_t length, x;
            if (v < 265) length = v - 254;
            else if (v == 285) length = 258;
            else {
                const uint32_t eb = (v - 261) >> 2;
                length = 3 + ((4u + ((v - 265) & 3u)) << eb);
                if (!fl_take(B, eb, &x)) return KCFL_RAW_EOF;
                length += x;
            }
            uint32_t dist;
            if (typ == 1) {
                if (!fl_take(B, 5, &x)) return KCFL_RAW_EOF;
                dist = fl_rev16(x) >> 11;
            } else {
                e = fl_sym<KCFL_PB_D>(B, TD, CD, CD.min_len, &dist);
                if (e) return e;
            }
            if (dist < 4) dist++;
            else if (dist < 30) {
                const uint32_t nb = (dist - 2) >> 1;
                if (!fl_take(B, nb, &x)) return KCFL_RAW_EOF;
                dist = (1u << (nb + 1)) + 1 + ((dist & 1u) << nb) + x;
            } else return KCFL_CORRUPT;
            const uint64_t mine = O.d - O.base;  // bytes of this stream so far
            if ((uint64_t)dist > mine + O.hist_len) return KCFL_CORRUPT;  // dist > dict.histSize()
            if (length > limit - O.d) return KCFL_OVER;
            if (WRITE) {
                fl_flush<WRITE>(O, lane);
                KC_WAVE_SYNC();  // what other lanes wrote so far is read back from here on
                uint8_t* o = O.dst + O.d;
                for (uint32_t k = (uint32_t)lane; k < length; k += 64) {
                    const uint32_t r = dist >= length ? k : k % dist;
                    const uint64_t back = (uint64_t)dist - r;  // 1 .. dist bytes in front of the match
                    o[k] = back <= mine ? *(o - back) : O.hist[O.hist_len - (uint32_t)(back - mine)];
                }
            }
            O.d += length;
        }
        if (final) break;
    }
    return KCFL_OK;
}

// One input.  Raw DEFLATE: the stream.  gzip: header, stream, trailer with the ISIZE compare, member after member; in the write pass
// `members` of them, each followed by the CRC-32 of its bytes against the trailer.  The verdict short of / with the CRC; *size, *used
// and *n_members as KcFlateParams describes them.
template <bool WRITE>
__device__ __forceinline__ uint32_t fl_input(const KcFlateParams& P, const uint64_t begin, const uint64_t end, uint8_t* dst, const uint64_t cap,
                                             const uint32_t members, FlLds& L, uint64_t* size, uint64_t* used, uint32_t* n_members, const int lane) {
    FlBits B;
    B.src = P.src; B.end = end;
    FlOut O;
    O.dst = dst; O.cap = cap; O.d = 0; O.hist = P.dict; O.hist_len = P.gzip ? 0 : P.dict_len; O.base = 0; O.nlit = 0; O.lit = 0;
    *size = 0; *used = 0; *n_members = 0;
    if (!P.gzip) {
        fl_seek(B, begin);
        uint32_t e = fl_over<WRITE>(fl_inflate<WRITE>(B, O, L, lane));
        if (e == KCFL_RAW_EOF) e = KCFL_OK;
        fl_flush<WRITE>(O, lane);
        if (e) return e;
        *size = O.d; *used = fl_read_pos(B) - begin; *n_members = 1;
        return KCFL_OK;
    }
    fl_crc_tables(L.crcT, lane);
    const uint8_t* s = P.src;
    uint64_t pos = begin;
    uint32_t done = 0;
    // every round reads a member's ten header bytes or ends the input
    for (;;) {
        if (WRITE && done == members) break;
        // readHeader, gunzip.go:183-253
        if (end - pos < 10) {
            if (end == pos && done) break;  // io.EOF behind a member: the file ends here
            return KCFL_EOF;                 // (in front of the first one: NewReader's io.EOF)
        }
        const uint32_t w = uniu(ld32(s + pos));
        if ((w & 0xFFFFFFu) != 0x088B1Fu) return KCFL_HEADER;
        const uint32_t flg = w >> 24;
        uint64_t p = pos + 10;
        if (flg & 4u) {
            if (end - p < 2) return KCFL_EOF;
            const uint32_t xlen = uniu((uint32_t)ld16(s + p));
            p += 2;
            if (end - p < xlen) return KCFL_EOF;
            p += xlen;
        }
        bool ended = false;
        for (uint32_t f = 8; f <= 16 && !ended; f <<= 1) {  // FNAME, FCOMMENT: readString
            if (!(flg & f)) continue;
            // every round reads one byte of the string, at most 512
            for (uint32_t i = 0;; i++) {
                if (i >= 512) return KCFL_HEADER;
                if (p + i >= end) { ended = true; break; }  // the raw io.EOF (gunzip.go:157-160)
                if (uniu((uint32_t)s[p + i]) == 0) { p += i + 1; break; }
            }
        }
        if (ended) {
            if (done) { *used = end - begin; break; }  // the file ends there, and the reader has read all of it looking for the string's end
            return KCFL_EOF;
        }
        if (flg & 2u) {
            if (end - p < 2) return KCFL_EOF;
            uint32_t c = 0xFFFFFFFFu;
            for (uint64_t k = pos; k < p; k++) c = L.crcT[0][(c ^ s[k]) & 0xFFu] ^ (c >> 8);
            if ((uniu(~c) & 0xFFFFu) != uniu((uint32_t)ld16(s + p))) return KCFL_HEADER;
            p += 2;
        }
        if (flg >> 5) return KCFL_HEADER;
        fl_seek(B, p);
        O.base = O.d;
        uint32_t e = fl_over<WRITE>(fl_inflate<WRITE>(B, O, L, lane));
        fl_flush<WRITE>(O, lane);
        if (e == KCFL_RAW_EOF) e = KCFL_OK;  // the member "ends": the trailer read below then finds nothing
        if (e) return e;
        p = fl_read_pos(B);
        if (end - p < 8) return KCFL_EOF;
        const uint32_t crc = uniu(ld32(s + p)), isize = uniu(ld32(s + p + 4));
        const uint64_t msize = O.d - O.base;
        if (isize != (uint32_t)msize) return KCFL_CHECKSUM;
        if (WRITE) {
            KC_WAVE_SYNC();
            const uint8_t* r = O.dst + O.base;
            auto rd32 = [&](int i) -> uint32_t { return ld32(r + i); };
            auto rdb = [&](int i) -> uint32_t { return r[i]; };
            if (uniu(s2_crc32c_wave(rd32, rdb, (int)msize, L.crcT, L.crcM, L.crcP, lane)) != crc) return KCFL_CHECKSUM;
        }
        pos = p + 8;
        done++;
        *size = O.d; *used = pos - begin; *n_members = done;
        if (!P.multistream) break;
    }
    return KCFL_OK;
}

// ---- zlib (RFC 1950): zlib/reader.go:134-187 (Reset: the header), :93-121 (Read: the trailer) ----

#define KCFL_ADLER_MOD 65521u
#define KCFL_ADLER_CHUNK 16384u  // bytes the wave sums between two reductions: 256 per lane, whatever n is

// The Adler-32 of ptr[0, n), wave-wide, of bytes this wave has written (KC_WAVE_SYNC before).  All lanes call and all get the value;
// n = 0 gives 1.  With s1 = 1 + sum b[i] and s2 = n + sum (n - i) * b[i], a chunk of L bytes that holds the plain sum A and the
// position-weighted sum W = sum k * b[k] (k from the chunk's start) moves the pair by s2 += L * s1 + L * A - W, s1 += A.
// The range is read as the aligned words that cover it: it is taken to begin `mis` bytes earlier, at the word boundary, with bytes
// of zero there that are never loaded; they add nothing to s1 and 1 each to s2, which starts that much lower.  Lane j takes the
// words j, j + 64, ... of a chunk: 64 lanes, 64 consecutive words per round.  A first or last word that the range covers in part
// is put together from its bytes inside the range.
// Overflow, for the fixed chunk of 16384 bytes: a lane sums 64 words = 256 bytes per chunk, so its plain sum is at most
// 256 * 255 = 65 280 and its weighted sum at most 255 * 256 * 16383 < 1.07e9 < 2^32.  The weighted sums are taken mod 65521 in
// the lanes before they are added up (64 * 65520 < 2^23; unreduced, 255 * 16384^2 / 2 would pass 2^32); the chunk's plain sum is
// at most 16384 * 255 < 2^22.  The scalar update is 64-bit: L * s1 + L * A <= 16384 * (65520 + 4 177 920) < 2^36.
__device__ __forceinline__ uint32_t fl_adler32_wave(const uint8_t* ptr, const uint64_t n, const int lane) {
    const uint32_t mis = (uint32_t)((uintptr_t)ptr & 3u);
    const uint8_t* q = ptr - mis;          // word-aligned; q[v] is in the range for mis <= v < total
    const uint64_t total = n + mis;
    uint32_t s1 = 1, s2 = KCFL_ADLER_MOD - mis;
    // every round takes a chunk: KCFL_ADLER_CHUNK bytes, or the rest
    for (uint64_t c0 = 0; c0 < total; c0 += KCFL_ADLER_CHUNK) {
        const uint32_t L = total - c0 < KCFL_ADLER_CHUNK ? (uint32_t)(total - c0) : KCFL_ADLER_CHUNK;
        const uint8_t* c = q + c0;
        uint32_t a = 0, w = 0;
        auto add = [&](const uint32_t k, const uint32_t x) {
            const uint32_t b0 = x & 0xFFu, b1 = (x >> 8) & 0xFFu, b2 = (x >> 16) & 0xFFu, b3 = x >> 24;
            const uint32_t sum = b0 + b1 + b2 + b3;
            a += sum;
            w += k * sum + b1 + 2u * b2 + 3u * b3;
        };
        if (L == KCFL_ADLER_CHUNK && (c0 || !mis)) {  // a whole chunk inside the range: 64 words per lane
#pragma unroll 8
            for (uint32_t j = 0; j < KCFL_ADLER_CHUNK / 256u; j++) {
                const uint32_t k = 4u * ((uint32_t)lane + 64u * j);
                add(k, ld32(c + k));
            }
        } else {
            // every round takes this lane's next word of the chunk, 256 bytes on
            for (uint32_t k = 4u * (uint32_t)lane; k < L; k += 256u) {
                uint32_t x = 0;
                if (c0 + k >= mis && k + 4u <= L) x = ld32(c + k);
                else
                    for (uint32_t t = 0; t < 4u; t++)
                        if (c0 + k + t >= mis && k + t < L) x |= (uint32_t)c[k + t] << (8u * t);
                add(k, x);
            }
        }
        const uint32_t A = wave_reduce_sum(a), W = wave_reduce_sum(w % KCFL_ADLER_MOD);
        s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)L * s1 + (uint64_t)L * A + 64u * KCFL_ADLER_MOD - W) % KCFL_ADLER_MOD);
        s1 = (s1 + A) % KCFL_ADLER_MOD;
    }
    return (s2 % KCFL_ADLER_MOD) << 16 | s1;
}

// One zlib input, as io.ReadAll(zlib.NewReaderDict(input, dict)) from a fresh reader: the two header bytes, the DICTID against
// P.dict_id, the DEFLATE stream, and the big-endian Adler-32 behind the byte that holds its last bit; what follows is not read.
// The verdict short of / with the Adler-32 (the write pass computes it); *size and *used as KcFlateParams describes them.
// (A reader that is REUSED hands its dictionary to the decompressor even without FDICT, reader.go:177-179: not modelled, there is
// no reused reader here.)
template <bool WRITE>
__device__ __forceinline__ uint32_t fl_zlib_input(const KcFlateParams& P, const uint64_t begin, const uint64_t end, uint8_t* dst, const uint64_t cap,
                                                  FlLds& L, uint64_t* size, uint64_t* used, const int lane) {
    *size = 0; *used = 0;
    const uint8_t* s = P.src;
    if (end - begin < 2) return KCFL_EOF;                                      // reader.go:143-149
    const uint32_t cmf = uniu((uint32_t)s[begin]), flg = uniu((uint32_t)s[begin + 1]);
    if ((cmf & 0x0Fu) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u) return KCFL_HEADER;   // :150-154
    uint64_t p = begin + 2;
    const bool have_dict = flg & 0x20u;
    if (have_dict) {                                                           // :155-169
        if (end - p < 4) return KCFL_EOF;
        if (__builtin_bswap32(uniu(ld32(s + p))) != P.dict_id) return KCFL_DICTIONARY;
        p += 4;
    }
    FlBits B;
    B.src = s; B.end = end;
    FlOut O;
    O.dst = dst; O.cap = cap; O.d = 0; O.hist = P.dict; O.hist_len = have_dict ? P.dict_len : 0; O.base = 0; O.nlit = 0; O.lit = 0;
    fl_seek(B, p);
    uint32_t e = fl_over<WRITE>(fl_inflate<WRITE>(B, O, L, lane));
    fl_flush<WRITE>(O, lane);
    if (e == KCFL_RAW_EOF) e = KCFL_OK;  // the stream "ends" at the input's end: the trailer read below then finds nothing
    if (e) return e;
    p = fl_read_pos(B);
    if (end - p < 4) return KCFL_EOF;                                          // :107-113
    const uint32_t want = __builtin_bswap32(uniu(ld32(s + p)));
    if (WRITE) {
        KC_WAVE_SYNC();
        if (uniu(fl_adler32_wave(O.dst, O.d, lane)) != want) return KCFL_CHECKSUM;   // :115-119
    }
    *size = O.d; *used = p + 4 - begin;
    return KCFL_OK;
}
