// kc_s2_rstream.hip — the data chunks of one window of the S2 stream reader (s2.NewReader(r).Read, s2/reader.go:249-405): ONE WAVE
// PER CHUNK RECORD.  The host state machine (kc_s2rstream_host.h) walked the chunk headers, staged the bytes from the first body of
// the window to the end of the last one and wrote one record per data chunk; every offset in a record is relative to the window.
//
// The decoder is s2d_decode_chunk (kc_s2_dec_dev.h), shared with the whole-input kernel and the ranged one: every read is checked
// against the chunk's end, every write against the chunk's own dlen bytes, and the CRC32C of the decoded chunk is compared in the
// masked form the stream stores.  In front of it the wave checks the record itself against the window — a body that does not lie
// inside the staged bytes, or an output range outside the window, is KCS2D_CORRUPT and nothing is read or written.  The verdict of
// the window (the first failing chunk in stream order, the bytes in front of it) is the host's, from the per-chunk verdicts.
#include "kc_s2_dec_dev.h"

__global__ __launch_bounds__(64) void kc_s2_rstream_kernel(KcS2RstreamParams P) {
    __shared__ uint32_t crcT[4][256];
    __shared__ uint32_t crcM[32];
    __shared__ uint32_t crcP[64];
    const int lane = (int)threadIdx.x;
    const uint32_t ci = blockIdx.x;
    if (ci >= P.n_chunks) return;
    const KcS2WChunk R = P.chunks[ci];
    const bool inside = R.body_off <= P.in_len && (uint64_t)R.body_len <= P.in_len - R.body_off && R.out_off <= P.out_len &&
                        (uint64_t)R.dlen <= P.out_len - R.out_off;
    uint32_t err = KCS2D_CORRUPT;
    if (inside) {
        const uint8_t* __restrict__ src = P.in + R.body_off;
        uint8_t* dst = P.out + R.out_off;
        const bool want_crc = !P.ignore_crc;
        if (want_crc) s2d_crc_tables(crcT, lane);
        err = s2d_decode_chunk(src, R.body_len, dst, R.dlen, R.kind & KC_S2C_STORED, want_crc, R.crc, crcT, crcM, crcP, lane);
    }
    if (lane == 0) P.status[ci] = err;
}

void kc_launch_s2_rstream(const KcS2RstreamParams& P, hipStream_t st) {
    if (P.n_chunks == 0) return;
    hipLaunchKernelGGL(kc_s2_rstream_kernel, dim3(P.n_chunks), dim3(64), 0, st, P);
}
