// kc_zip_dev.h — the members of zip archives read on the device: the parameters and launchers of kc_zip.hip, and the device
// functions of its four kernels.  One source buffer, a table of n members (include/kcgpu.h kc_zip_member; offsets absolute in the
// buffer), one verdict per member: that of f.Open(), io.ReadAll, Close of zip/reader.go:247-362 (Open, checksumReader.Read),
// :368-381 (findBodyOffset), :566-603 (readDataDescriptor).  The central directory states every member's decoded size, so each
// member is decoded ONCE, straight to its place, with the stated size as the room it may fill: there is no sizing pass.
//
// The input is untrusted: every read is checked against the buffer's end and every write against the member's own range before it
// is made.  Control flow is scalar (uniu), as in kc_flate_dev.h.
#pragma once
#include "../../include/kcgpu.h"
#include "kc_flate_dev.h"

// per-member verdicts beside KCFL_OK / KCFL_CORRUPT / KCFL_EOF: the KC_ZIP_* of include/kcgpu.h
#define KCZP_FORMAT 16u
#define KCZP_ALGORITHM 19u
#define KCZP_CHECKSUM 20u
#define KCZP_READAT 21u
#define KCZP_SIZE 22u
// what the host's plan made of a member
#define KCZP_NONE 0u      // its verdict follows from the table and the local header: no range, no work
#define KCZP_INFLATE 1u   // deflated: decoded to its range, bounded by the stated size
#define KCZP_WALK 2u      // deflated, and the stated size is more than DEFLATE can expand to: walked without writing, no range
#define KCZP_STORE 3u     // stored, clipped compressed size = stated size: copied by chunks
#define KCZP_CHUNK 65536u // bytes one wave of the store kernel copies

struct KcZipParams {
    const uint8_t* src;
    uint64_t src_len;
    const kc_zip_member* mem;    // n
    uint32_t n;
    // locate kernel: written
    uint64_t* body;              // where the body starts, clipped to the buffer
    uint64_t* body_end;          // body + compressed size, clipped to the buffer
    uint32_t* lstatus;           // KCFL_OK, KCZP_READAT or KCZP_FORMAT: the local header
    uint32_t* dstatus;           // members with flag bit 3: KCFL_OK, KCFL_EOF (no whole descriptor) or KCZP_CHECKSUM (its CRC field)
    // the plan, from the host
    const uint32_t* kind;        // KCZP_*
    const uint64_t* out0;        // where the member's range starts in dst
    const uint32_t* chunk0;      // n + 1: the first chunk of every stored member
    const uint32_t* chunk_mem;   // per chunk: its member
    uint32_t n_chunks;
    uint8_t* dst;
    // inflate and store kernels: written; finish kernel: read
    uint32_t* verdict;           // deflated members: the size rules' verdict
    uint32_t* crc;               // deflated members that stand so far: the CRC-32 of what was written
    uint32_t* chunk_crc;         // per chunk
    uint32_t* status;            // finish kernel: the final verdict of every member with a kind
};
void kc_launch_zip_locate(const KcZipParams& P, hipStream_t st);
void kc_launch_zip_inflate(const KcZipParams& P, bool write, hipStream_t st);  // write: the KCZP_INFLATE members, else the KCZP_WALK ones
void kc_launch_zip_store(const KcZipParams& P, hipStream_t st);
void kc_launch_zip_finish(const KcZipParams& P, hipStream_t st);

// the CRC tables of one wave (s2_crc32c_wave's) where no Huffman tables are needed
struct ZpCrcLds { uint32_t crcT[4][256], crcM[32], crcP[64]; };
// x^(8 * 2^b) modulo the polynomial as 32 columns, b = 0 .. 16: the operator "b zero bytes follow" of the reflected CRC register
struct ZpPowLds { uint32_t pow[17][32]; };

// findBodyOffset (reader.go:368-381), the SectionReader's clipping (:268-269) and readDataDescriptor's verdict short of the hash
// (:566-603) for member t.  One lane per member.
__device__ __forceinline__ void zp_locate(const KcZipParams& P, const uint32_t t) {
    const kc_zip_member m = P.mem[t];
    uint32_t ls = KCFL_OK, ds = KCFL_OK;
    uint64_t body = P.src_len, bend = P.src_len;
    if (m.header_offset < 0 || P.src_len < 30 || (uint64_t)m.header_offset > P.src_len - 30) ls = KCZP_READAT;  // ReadAt, :370
    else {
        const uint8_t* h = P.src + m.header_offset;
        if (ld32(h) != 0x04034b50u) ls = KCZP_FORMAT;                            // :374-376
        else {
            const uint64_t b = (uint64_t)m.header_offset + 30 + ld16(h + 26) + ld16(h + 28);  // the LOCAL lengths, :378-380
            bool desc = false;    // body + compressed size lies inside the buffer
            if (b <= P.src_len) {
                body = b;
                if (m.compressed_size <= P.src_len - b) { bend = b + m.compressed_size; desc = true; }
            }
            if (m.flags & 8u) {                                                  // :276-278, 566-603
                const uint64_t have = desc ? P.src_len - bend : 0;
                if (have < 4) ds = KCFL_EOF;
                else {
                    const uint32_t w = ld32(P.src + bend);
                    const bool sig = w == 0x08074b50u;
                    if (have < (sig ? 16u : 12u)) ds = KCFL_EOF;
                    else if ((sig ? ld32(P.src + bend + 4) : w) != m.crc32) ds = KCZP_CHECKSUM;
                }
            }
        }
    }
    P.body[t] = body; P.body_end[t] = bend; P.lstatus[t] = ls; P.dstatus[t] = ds;
}

// One deflated member by one wave: flate.NewReader over the clipped body, with checksumReader's size rules (:324-340).  WRITE: the
// members of kind KCZP_INFLATE, decoded to their ranges; else those of kind KCZP_WALK, walked without a write.
template <bool WRITE>
__device__ __forceinline__ void zp_inflate(const KcZipParams& P, const uint32_t i, FlLds& L, const int lane) {
    if (uniu(P.kind[i]) != (WRITE ? KCZP_INFLATE : KCZP_WALK)) return;
    const uint64_t usize = P.mem[i].uncompressed_size;
    FlBits B;
    B.src = P.src; B.end = P.body_end[i];
    fl_seek(B, P.body[i]);
    FlOut O;
    O.dst = WRITE ? P.dst + P.out0[i] : nullptr;
    O.cap = usize; O.d = 0; O.base = 0; O.nlit = 0; O.lit = 0;
    O.hist = P.src; O.hist_len = 0;  // no preset dictionary: hist is never read (a constant null here crashes the compiler's simplifycfg pass)
    if (WRITE) fl_crc_tables(L.crcT, lane);
    uint32_t e = fl_inflate<WRITE, true>(B, O, L, lane), crc = 0;
    fl_flush<WRITE>(O, lane);
    if (e == KCFL_RAW_EOF) e = KCFL_OK;                  // the raw io.EOF is an end (:337)
    if (e == KCFL_OVER || O.d > usize) e = KCZP_FORMAT;  // nread > UncompressedSize64, whatever follows (:331-333)
    else if (e == KCFL_OK && O.d != usize) e = KCFL_EOF;  // :338-340
    if (WRITE && e == KCFL_OK) {
        KC_WAVE_SYNC();
        const uint8_t* r = O.dst;
        auto rd32 = [&](int k) -> uint32_t { return ld32(r + k); };
        auto rdb = [&](int k) -> uint32_t { return r[k]; };
        crc = uniu(s2_crc32c_wave(rd32, rdb, (int)usize, L.crcT, L.crcM, L.crcP, lane));
    }
    if (lane == 0) { P.verdict[i] = e; P.crc[i] = crc; }
}

// One chunk of a stored member by one wave: copied source to range, 8 bytes per lane between a head and a tail done by byte so
// that the stores are aligned, and its CRC-32 from the source bytes.
__device__ __forceinline__ void zp_store(const KcZipParams& P, const uint32_t c, ZpCrcLds& L, const int lane) {
    const uint32_t i = uniu(P.chunk_mem[c]);
    const uint64_t at = (uint64_t)(c - uniu(P.chunk0[i])) * KCZP_CHUNK, usize = P.mem[i].uncompressed_size;
    if (at >= usize) return;  // (never: the plan counts the chunks from the same size)
    const uint32_t len = usize - at < KCZP_CHUNK ? (uint32_t)(usize - at) : KCZP_CHUNK;
    const uint8_t* s = P.src + P.body[i] + at;  // [body, body + usize) is inside the buffer: the plan checked the clipped size
    uint8_t* o = P.dst + P.out0[i] + at;
    fl_crc_tables(L.crcT, lane);
    uint32_t head = (uint32_t)((8u - ((uintptr_t)o & 7u)) & 7u);
    if (head > len) head = len;
    const uint32_t mid = (len - head) & ~7u;
    if ((uint32_t)lane < head) o[lane] = s[lane];
    for (uint32_t k = (uint32_t)lane * 8; k < mid; k += 512) *(uint64_t*)(o + head + k) = ld64(s + head + k);
    for (uint32_t k = head + mid + (uint32_t)lane; k < len; k += 64) o[k] = s[k];
    auto rd32 = [&](int k) -> uint32_t { return ld32(s + k); };
    auto rdb = [&](int k) -> uint32_t { return s[k]; };
    const uint32_t crc = uniu(s2_crc32c_wave(rd32, rdb, (int)len, L.crcT, L.crcM, L.crcP, lane));
    if (lane == 0) P.chunk_crc[c] = crc;
}

// v moved over the zero bytes that the columns M stand for
__device__ __forceinline__ uint32_t zp_apply(const uint32_t* M, uint32_t v) {
    uint32_t a = 0;
    for (int k = 0; k < 32; k++)
        if ((v >> k) & 1u) a ^= M[k];
    return a;
}

// CRC-32 of a stored member from its chunks' values, in order: CRC(a || b) = CRC(a) * x^(8 * len(b)) + CRC(b) modulo the polynomial
// (the initial and final inversions cancel).  All lanes call; every lane gets the value.
__device__ __forceinline__ uint32_t zp_combine(const uint32_t* chunk_crc, const uint32_t n, const uint32_t last_len, ZpPowLds& L, const int lane) {
    if (n == 0) return 0;
    uint32_t acc = uniu(chunk_crc[0]);
    if (n == 1) return acc;
    if (lane < 32) {  // one zero byte: eight shifts of the reflected register
        uint32_t v = 1u << lane;
        for (int k = 0; k < 8; k++) v = (v & 1u) ? (v >> 1) ^ 0xEDB88320u : v >> 1;
        L.pow[0][lane] = v;
    }
    KC_WAVE_SYNC();
    for (int b = 1; b <= 16; b++) {  // twice as many zero bytes: the operator applied to its own columns
        if (lane < 32) L.pow[b][lane] = zp_apply(L.pow[b - 1], L.pow[b - 1][lane]);
        KC_WAVE_SYNC();
    }
    for (uint32_t j = 1; j + 1 < n; j++) acc = zp_apply(L.pow[16], acc) ^ uniu(chunk_crc[j]);
    for (int b = 0; b <= 16; b++)
        if ((last_len >> b) & 1u) acc = zp_apply(L.pow[b], acc);
    return acc ^ uniu(chunk_crc[n - 1]);
}

// The final verdict of member i by one wave: the stored members' CRC from their chunks, the data descriptor and the CRC compare
// (:341-358), and no byte of a failed member left in its range.
__device__ __forceinline__ void zp_finish(const KcZipParams& P, const uint32_t i, ZpPowLds& L, const int lane) {
    const uint32_t kind = uniu(P.kind[i]);
    if (kind == KCZP_NONE) return;
    const kc_zip_member m = P.mem[i];
    uint32_t v = KCFL_OK, crc;
    if (kind == KCZP_STORE) {
        const uint32_t c0 = uniu(P.chunk0[i]), nc = uniu(P.chunk0[i + 1]) - c0;
        crc = zp_combine(P.chunk_crc + c0, nc, nc ? (uint32_t)(m.uncompressed_size - (uint64_t)(nc - 1) * KCZP_CHUNK) : 0, L, lane);
    } else {
        v = uniu(P.verdict[i]);
        crc = uniu(P.crc[i]);
    }
    if (v == KCFL_OK) {
        if (m.flags & 8u) {
            v = uniu(P.dstatus[i]);                                             // :341-347
            if (v == KCFL_OK && crc != m.crc32) v = KCZP_CHECKSUM;              // :348-350
        } else if (m.crc32 != 0 && crc != m.crc32) v = KCZP_CHECKSUM;           // :352-357
    }
    if (v != KCFL_OK && kind != KCZP_WALK) {
        KC_WAVE_SYNC();
        uint8_t* o = P.dst + P.out0[i];
        for (uint64_t k = (uint64_t)lane; k < m.uncompressed_size; k += 64) o[k] = 0;
    }
    if (lane == 0) P.status[i] = v;
}
