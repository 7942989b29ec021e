// kc_s2_ranges.hip — s2.ReadSeeker.ReadAt over a batch of requests (input, offset, length): the ranged plan and the clipped decode.
//
// The plan: one lane per request runs kc_s2_walk_range (kc_s2_plan_dev.h) from where Index.Find put it — the input's start, or an
// index entry, then in the state the reader has behind the identifier at the input's front.  Chunks in front of the range are
// passed by their headers alone (Reader.Skip, s2/reader.go:674-842: no body and no CRC is touched); every chunk from the one that
// holds `off` onwards gets a record, and the walk reads nothing behind the chunk whose decoded end reaches off + len.  The first
// pass sizes the request (covered chunks, bytes it will get, scratch for its clipped chunks, first header-level status); the second
// pass writes the records.  The output layout is the prefix sum of the requests' lengths and depends on nothing in the data.
//
// The decode: one wave per covered chunk, the decoder of kc_s2_dec_dev.h.  A chunk that lies wholly inside its request decodes
// straight to its place in dst.  A clipped one — at most the first and the last of a request — decodes into a scratch slot of dlen
// bytes, its CRC is checked over the whole chunk, and the same wave then copies [clip_lo, clip_hi) to dst.  The decoder checks its
// writes against the dlen bytes of the slot or, for an inner chunk, of the chunk's place inside the request's own range.
#include "kc_s2_dec_dev.h"
#include "kc_s2_plan_dev.h"

__global__ __launch_bounds__(64) void kc_s2_range_plan_kernel(KcS2RangePlanParams P) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.m) return;
    const bool fill = P.chunks != nullptr;
    const uint8_t* __restrict__ in = P.src;
    const KcS2Req Q = P.reqs[j];
    KcS2RChunk* out = fill ? P.chunks + Q.chunk0 : nullptr;
    const uint64_t hi = Q.off + Q.len;  // (the host refused a range that wraps)
    uint64_t slot_bytes = 0;
    auto cover = [&](uint32_t index, uint64_t body_off, uint32_t body_len, uint32_t kind, uint64_t a, uint32_t dlen, uint32_t crc) {
        const uint64_t b = a + dlen;
        const uint32_t lo = a < Q.off ? (uint32_t)(Q.off - a) : 0u;
        const uint32_t chi = b > hi ? (uint32_t)(hi - a) : dlen;  // (a <= hi: the walk ends once it has reached hi)
        const bool clipped = lo > 0 || chi < dlen;
        const uint64_t slot = slot_bytes;
        if (clipped) slot_bytes += ((uint64_t)dlen + 15) & ~(uint64_t)15;
        if (!fill) return;
        KcS2RChunk R;
        R.c.body_off = body_off; R.c.out_off = Q.out0 + ((a < Q.off ? Q.off : a) - Q.off); R.c.body_len = body_len; R.c.dlen = dlen; R.c.crc = crc;
        R.c.kind = kind; R.c.stream = j; R.c.index = index;
        R.slot_off = clipped ? Q.slot0 + slot : KC_S2R_NO_SLOT;
        R.clip_lo = lo; R.clip_hi = chi;
        out[index] = R;
    };
    bool readHeader = P.ignore_id != 0, snappy = false;
    uint32_t front = KCS2D_OK;
    if (Q.flags & KC_S2R_MID) {
        readHeader = true;
        if (Q.flags & KC_S2R_KNOWN) snappy = (Q.flags & KC_S2R_SNAPPY) != 0;
        else front = kc_s2_front_state(in, Q.front, Q.end, P.ignore_id != 0, &snappy);
    }
    KcS2RangeWalk W;
    if (front) { W.status = front; W.n_cover = 0; W.got = 0; }
    else W = kc_s2_walk_range(in, Q.pos, Q.end, P.max_block, P.max_buf, readHeader, snappy, Q.u, Q.off, Q.len, cover);
    if (fill) return;
    KcS2ReqPlan R;
    R.got = W.got; R.slot_bytes = slot_bytes; R.n_chunks = W.n_cover; R.status = W.status;
    P.plan[j] = R;
}

__global__ __launch_bounds__(64) void kc_s2_range_decode_kernel(KcS2RangeDecodeParams P) {
    __shared__ uint32_t crcT[4][256];
    __shared__ uint32_t crcM[32];
    __shared__ uint32_t crcP[64];
    const int lane = (int)threadIdx.x;
    const uint32_t ci = blockIdx.x;
    if (ci >= P.n_chunks) return;
    const KcS2RChunk R = P.chunks[ci];
    const uint8_t* __restrict__ src = P.src + R.c.body_off;
    const bool clipped = R.slot_off != KC_S2R_NO_SLOT;
    uint8_t* out = P.dst + R.c.out_off;
    uint8_t* dst = clipped ? P.slots + R.slot_off : out;
    const bool want_crc = !(R.c.kind & KC_S2C_NOCRC) && !P.ignore_crc;
    if (want_crc) s2d_crc_tables(crcT, lane);
    const uint32_t err = s2d_decode_chunk(src, R.c.body_len, dst, R.c.dlen, R.c.kind, want_crc, R.c.crc, crcT, crcM, crcP, lane);
    if (!err && clipped && R.clip_lo < R.clip_hi && R.clip_hi <= R.c.dlen) {
        KC_WAVE_SYNC();  // the slot was written by all lanes
        const uint8_t* a = dst + R.clip_lo;
        const uint32_t n = R.clip_hi - R.clip_lo;
        const uint32_t body = n & ~15u;
        for (uint32_t k = (uint32_t)lane * 16; k < body; k += 1024) s2d_st128u(out + k, ld128u(a + k));
        for (uint32_t k = body + (uint32_t)lane; k < n; k += 64) out[k] = a[k];
    }
    if (lane == 0) P.status[ci] = err;
}

void kc_launch_s2_range_plan(const KcS2RangePlanParams& P, hipStream_t st) {
    if (P.m == 0) return;
    hipLaunchKernelGGL(kc_s2_range_plan_kernel, dim3((P.m + 63) / 64), dim3(64), 0, st, P);
}

void kc_launch_s2_range_decode(const KcS2RangeDecodeParams& P, hipStream_t st) {
    if (P.n_chunks == 0) return;
    hipLaunchKernelGGL(kc_s2_range_decode_kernel, dim3(P.n_chunks), dim3(64), 0, st, P);
}
