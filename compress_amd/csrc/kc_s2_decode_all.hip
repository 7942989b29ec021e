// kc_s2_decode_all.hip — s2.Decode / the data chunks of s2.Reader on the device, as a product: ONE WAVE PER CHUNK, the grid is the
// chunk table the plan kernel wrote (kc_s2_plan.hip).  The decoded length of every chunk is known from its header, so a chunk
// decodes straight to its final place in dst; nothing is staged or compacted.
//
// Semantics: s2Decode (s2/decode_other.go:22-290) — literals in all five length forms, copy1 / copy2 / copy4, the repeat forms with
// their extended lengths, `offset <= 0 || d < offset || length > len(dst) - d`, both literal bounds, `d != dLen` at the end.  The
// input is untrusted: every read is checked against the chunk's end and every write against the chunk's own output range, and all
// checks of an operation come before any of its writes.
//
// The tag stream is parsed once per wave: all lanes load the same (up to) 8 bytes at the tag, the value goes through
// v_readfirstlane, and everything derived from it — lengths, offsets, positions, the branches — is scalar.  Every copy is spread
// over the 64 lanes: 8 bytes per lane for literals and for matches that do not overlap their source; an overlapping match of up
// to 64 bytes is one byte per lane from the period; a longer one doubles — each round copies the whole periodic region written so
// far, which is a copy without overlap.  CRC32C of the decoded chunk (s2_crc32c_wave, the writer's own) follows in the same
// kernel and is compared in the masked form the stream stores (s2/s2.go:120-125).
#include "kc_s2_dec_dev.h"

__global__ __launch_bounds__(64) void kc_s2_decode_all_kernel(KcS2DecodeAllParams P) {
    __shared__ uint32_t crcT[4][256];
    __shared__ uint32_t crcM[32];
    __shared__ uint32_t crcP[64];
    const int lane = (int)threadIdx.x;
    const uint32_t ci = blockIdx.x;
    if (ci >= P.n_chunks) return;
    const KcS2Chunk C = P.chunks[ci];
    const uint8_t* __restrict__ src = P.src + C.body_off;
    const uint32_t n = C.body_len;
    uint8_t* dst = P.dst + C.out_off;
    const uint64_t dLen = C.dlen;
    const bool want_crc = !(C.kind & KC_S2C_NOCRC) && !P.ignore_crc;
    if (want_crc) s2d_crc_tables(crcT, lane);
    const uint32_t err = s2d_decode_chunk(src, n, dst, dLen, C.kind, want_crc, C.crc, crcT, crcM, crcP, lane);
    if (lane == 0) P.status[ci] = err;
}

void kc_launch_s2_decode_all(const KcS2DecodeAllParams& P, hipStream_t st) {
    if (P.n_chunks == 0) return;
    hipLaunchKernelGGL(kc_s2_decode_all_kernel, dim3(P.n_chunks), dim3(64), 0, st, P);
}
