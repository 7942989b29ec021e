// kc_s2_dec_api.cpp — s2.Reader and s2.Decode over a batch of independent inputs: the reader options and the entry points
// kc_s2_decode_streams[_bound][_dev] / kc_s2_decode_blocks_all[_bound][_dev] of include/kcgpu.h.
//
// One call: the plan kernel's first pass sizes every input (kc_s2_plan.hip: data chunks, decoded bytes, first header-level error);
// the prefix sum of those sizes IS the output layout, because an S2 chunk's decoded length stands in its header; the second pass
// writes the chunk records with their final places in dst and the decode kernel decodes one chunk per wave straight to its place
// and checks its CRC (kc_s2_decode_all.hip).  The host then settles every input — the first failing chunk in stream order, else
// the plan's error — and zero-fills the range of every input that failed.  Nothing is staged and nothing is compacted.
#include "kc_host.h"
#include "kc_s2_plan_dev.h"

namespace {

enum { SD_IN_OFF, SD_NC, SD_BOUND, SD_STATUS, SD_CHUNK0, SD_OUT0, SD_CHUNKS, SD_CSTATUS };  // c->s2d[]

struct Mode {  // what one call decodes: framed streams under the reader's options, or bare blocks
    uint32_t max_block = (uint32_t)KC_S2_MAX_FRAMED_BLOCK;
    int ignore_crc = 0, ignore_id = 0, blocks = 0;
};
Mode mode_of(const kc_s2_ropts* o) {
    Mode m;
    m.max_block = o->max_block; m.ignore_crc = o->ignore_crc; m.ignore_id = o->ignore_id;
    return m;
}
Mode mode_blocks() {
    Mode m;
    m.blocks = 1;
    return m;
}
uint32_t max_buf_of(const Mode& m) { return (uint32_t)kc_s2_max_encoded_len((int64_t)m.max_block) + 4u; }  // Reader.maxBufSize (s2/reader.go:42)

struct PlanHost {
    std::vector<uint32_t> nc, status;
    std::vector<uint64_t> bound;
};

// the walk of one input on the host: the same function the plan kernel runs
KcS2Walk walk_host(const Mode& m, const uint8_t* src, uint64_t pos, uint64_t end) {
    auto none = [](uint32_t, uint64_t, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t) {};
    if (!m.blocks) return kc_s2_walk(src, pos, end, m.max_block, max_buf_of(m), m.ignore_id != 0, none);
    KcS2Walk W;
    W.status = KCS2D_OK; W.n_chunks = 0; W.total = 0;
    uint32_t dl = 0, hdr = 0;
    if (end - pos > 0xffffffffull) W.status = KCS2D_SIZE;
    else if (!kc_s2_decoded_len(src, pos, end, &dl, &hdr)) W.status = KCS2D_CORRUPT;
    else { W.n_chunks = 1; W.total = dl; }
    return W;
}

// the plan's first pass over all inputs; its results on the host.  The inputs' offsets stay on the device.
kc_status plan_inputs(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcS2PlanParams& P, PlanHost& H) {
    hipStream_t st = c->stream;
    kc_status s;
    DevBuf* z = c->s2d;
    if ((s = ensure(c, z[SD_IN_OFF], (size_t)(n + 1) * 8)) || (s = ensure(c, z[SD_NC], (size_t)n * 4)) || (s = ensure(c, z[SD_BOUND], (size_t)n * 8)) ||
        (s = ensure(c, z[SD_STATUS], (size_t)n * 4)) || (s = ensure(c, z[SD_CHUNK0], (size_t)n * 4)) || (s = ensure(c, z[SD_OUT0], (size_t)n * 8)))
        return s;
    HIPCHK(c, hipMemcpyAsync(z[SD_IN_OFF].p, in_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    memset(&P, 0, sizeof(P));
    P.src = d_src;
    P.in_off = (const uint64_t*)z[SD_IN_OFF].p;
    P.n = n;
    P.max_block = m.max_block;
    P.max_buf = max_buf_of(m);
    P.ignore_id = m.ignore_id;
    P.blocks = m.blocks;
    P.n_chunks = (uint32_t*)z[SD_NC].p;
    P.bound = (uint64_t*)z[SD_BOUND].p;
    P.status = (uint32_t*)z[SD_STATUS].p;
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    kc_launch_s2_plan(P, st);
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    H.nc.resize(n); H.status.resize(n); H.bound.resize(n);
    HIPCHK(c, hipMemcpyAsync(H.nc.data(), P.n_chunks, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.status.data(), P.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.bound.data(), P.bound, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
    c->last.prep_ms += t;
    return KC_OK;
}

const uint64_t kPerChunk = sizeof(KcS2Chunk) + 4;  // device scratch one data chunk takes: its record and its verdict

kc_status check_args(kc_ctx* c, const void* src, const uint64_t* in_off, uint32_t n) {
    if (!c || !in_off || (n && !src)) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    for (uint32_t i = 0; i < n; i++)
        if (in_off[i + 1] < in_off[i]) { c->err = "in_off not ascending"; return KC_ERR_BAD_ARG; }
    return KC_OK;
}

kc_status decode_dev(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                     uint64_t* out_off, uint32_t* status) {
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last_batches = 0;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf* z = c->s2d;
    KcS2PlanParams P;
    PlanHost H;
    kc_status s = plan_inputs(c, m, d_src, in_off, n, P, H);
    if (s != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.bound[i];  // the planned layout
    if (out_off[n] > dst_cap) { c->err = "dst_cap too small for the planned layout"; return KC_ERR_DST_TOO_SMALL; }  // (nothing written yet)
    const uint64_t budget = scratch_budget(c);
    std::vector<uint32_t> chunk0(n), cstatus;
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: inputs i0 .. i1 whose chunk records fit the budget (ensure() over-allocates by 1/8) ----
        uint32_t i1 = i0, nc = 0;
        while (i1 < n) {
            const uint64_t all = ((uint64_t)nc + H.nc[i1]) * kPerChunk;
            if (i1 > i0 && (all + (all >> 3) > budget || (uint64_t)nc + H.nc[i1] > 0x3FFFFFFFu)) break;
            chunk0[i1] = nc;
            nc += H.nc[i1];
            i1++;
        }
        const uint32_t nb = i1 - i0;
        if (nc) {
            if ((s = ensure(c, z[SD_CHUNKS], (size_t)nc * sizeof(KcS2Chunk))) || (s = ensure(c, z[SD_CSTATUS], (size_t)nc * 4))) return s;
            HIPCHK(c, hipMemcpyAsync((uint32_t*)z[SD_CHUNK0].p + i0, chunk0.data() + i0, (size_t)nb * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync((uint64_t*)z[SD_OUT0].p + i0, out_off + i0, (size_t)nb * 8, hipMemcpyHostToDevice, st));
            KcS2PlanParams Q = P;  // second pass over this batch's inputs: the chunk records
            Q.in_off = P.in_off + i0;
            Q.n = nb;
            Q.chunk0 = (const uint32_t*)z[SD_CHUNK0].p + i0;
            Q.out0 = (const uint64_t*)z[SD_OUT0].p + i0;
            Q.chunks = (KcS2Chunk*)z[SD_CHUNKS].p;
            KcS2DecodeAllParams D;
            memset(&D, 0, sizeof(D));
            D.src = d_src;
            D.chunks = Q.chunks;
            D.n_chunks = nc;
            D.dst = d_dst;
            D.ignore_crc = m.ignore_crc;
            D.status = (uint32_t*)z[SD_CSTATUS].p;
            HIPCHK(c, hipEventRecord(c->ev[0], st));
            kc_launch_s2_plan(Q, st);
            HIPCHK(c, hipEventRecord(c->ev[1], st));
            kc_launch_s2_decode_all(D, st);
            HIPCHK(c, hipEventRecord(c->ev[2], st));
            cstatus.resize(nc);
            HIPCHK(c, hipMemcpyAsync(cstatus.data(), D.status, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            float t01 = 0, t12 = 0;
            (void)hipEventElapsedTime(&t01, c->ev[0], c->ev[1]);
            (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
            c->last.prep_ms += t01;
            c->last.match_ms += t12;
        }
        // ---- settle: the first failing chunk in stream order wins over the header-level error behind it (inside a chunk the
        // reference's order is DecodedLen, Snappy limit, max block — the plan — then decode, CRC — the kernel); a failed input's
        // planned range is zero-filled: no byte decoded from a corrupt stream stays in dst ----
        for (uint32_t i = i0; i < i1; i++) {
            uint32_t v = KCS2D_OK;
            for (uint32_t k = 0; k < H.nc[i] && !v; k++) v = cstatus[chunk0[i] + k];
            if (!v) v = H.status[i];
            status[i] = v;
            if (v && H.bound[i]) HIPCHK(c, hipMemsetAsync(d_dst + out_off[i], 0, (size_t)H.bound[i], st));
        }
        c->last_batches++;
        i0 = i1;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    c->last.total_ms = c->last.prep_ms + c->last.match_ms;
    return KC_OK;
}

kc_status bound_dev(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, d_src, in_off, n);
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    KcS2PlanParams P;
    PlanHost H;
    if ((s = plan_inputs(c, m, d_src, in_off, n, P, H)) != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) { bound[i] = H.bound[i]; status[i] = H.status[i]; }
    c->last.total_ms = c->last.prep_ms;
    return KC_OK;
}

kc_status bound_host(kc_ctx* c, const Mode& m, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) {  // the headers are in host memory: the walk runs where they are
        const KcS2Walk W = walk_host(m, src, in_off[i], in_off[i + 1]);
        bound[i] = W.total;
        status[i] = W.status;
    }
    return KC_OK;
}

// Host buffers: the walk runs on the host first (the layout, and DST_TOO_SMALL before anything is written); the inputs then go to
// the device in groups, cut between inputs, whose bytes and decoded bytes together fit a quarter of the scratch budget.  An input
// that does not fit alone gets KC_S2D_SIZE_EXCEEDED: it keeps its planned range, zero-filled like any other failed input's.
kc_status decode_host(kc_ctx* c, const Mode& m, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                      uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !dst && dst_cap) return KC_ERR_BAD_ARG;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    std::vector<uint64_t> bound(n);
    for (uint32_t i = 0; i < n; i++) {
        bound[i] = walk_host(m, src, in_off[i], in_off[i + 1]).total;
        out_off[i + 1] = out_off[i] + bound[i];
    }
    if (out_off[n] > dst_cap) { c->err = "dst_cap too small for the planned layout"; return KC_ERR_DST_TOO_SMALL; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    kc_timings sum = {0, 0, 0, 0, 0, 0};
    int batches = 0;
    std::vector<uint64_t> rel, oo;
    std::vector<uint32_t> stt;
    uint32_t i0 = 0;
    while (i0 < n) {
        const uint64_t quarter = scratch_budget(c) / 4;
        auto cost = [&](uint32_t a, uint32_t b) { return (in_off[b] - in_off[a]) + (out_off[b] - out_off[a]); };
        if (cost(i0, i0 + 1) > quarter) {
            status[i0] = KC_S2D_SIZE_EXCEEDED;
            if (bound[i0]) memset(dst + out_off[i0], 0, (size_t)bound[i0]);
            i0++;
            continue;
        }
        uint32_t i1 = i0 + 1;
        while (i1 < n && cost(i0, i1 + 1) <= quarter) i1++;
        const uint32_t nb = i1 - i0;
        const uint64_t bytes = in_off[i1] - in_off[i0], need = out_off[i1] - out_off[i0];
        if ((s = ensure(c, c->tmp_src, (size_t)bytes + 64)) || (s = ensure(c, c->tmp_dst, (size_t)need + 64))) return s;
        if (bytes) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src + in_off[i0], (size_t)bytes, hipMemcpyHostToDevice, st));
        rel.resize(nb + 1); oo.resize(nb + 1); stt.resize(nb);
        for (uint32_t k = 0; k <= nb; k++) rel[k] = in_off[i0 + k] - in_off[i0];
        if ((s = decode_dev(c, m, (const uint8_t*)c->tmp_src.p, rel.data(), nb, (uint8_t*)c->tmp_dst.p, need, oo.data(), stt.data())) != KC_OK) return s;
        if (oo[nb] != need) { c->err = "internal: the device plan and the host plan disagree"; return KC_ERR_INTERNAL; }
        if (need) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (uint32_t k = 0; k < nb; k++) status[i0 + k] = stt[k];
        sum.prep_ms += c->last.prep_ms; sum.match_ms += c->last.match_ms; sum.total_ms += c->last.total_ms;
        batches += c->last_batches;
        i0 = i1;
    }
    c->last = sum;
    c->last_batches = batches;
    return KC_OK;
}

kc_status decode_dev_checked(kc_ctx* c, const Mode& m, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                             uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, d_src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !d_dst && dst_cap) return KC_ERR_BAD_ARG;
    return decode_dev(c, m, d_src, in_off, n, d_dst, dst_cap, out_off, status);
}

}  // namespace

extern "C" {

kc_s2_ropts* kc_s2_ropts_default(void) {
    try { return new kc_s2_ropts(); } catch (...) { return nullptr; }
}
void kc_s2_ropts_free(kc_s2_ropts* o) { delete o; }
int kc_s2_ropts_max_block_size(kc_s2_ropts* o, int64_t n) {  // ReaderMaxBlockSize, s2/reader.go:64-75
    if (!o || n <= 0 || n > (int64_t)KC_S2_MAX_FRAMED_BLOCK) return -1;
    o->max_block = (uint32_t)n;
    return 0;
}
int kc_s2_ropts_ignore_crc(kc_s2_ropts* o, int b) {  // ReaderIgnoreCRC, s2/reader.go:120-125
    if (!o) return -1;
    o->ignore_crc = b != 0;
    return 0;
}
int kc_s2_ropts_ignore_stream_identifier(kc_s2_ropts* o, int b) {  // ReaderIgnoreStreamIdentifier, s2/reader.go:95-100
    if (!o) return -1;
    o->ignore_id = b != 0;
    return 0;
}

// io.ReadAll(s2.NewReader(input)) per input: s2/reader.go:249-405
kc_status kc_s2_decode_streams_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                   uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return decode_dev_checked(c, mode_of(o), d_src, in_off, n, d_dst, dst_cap, out_off, status);
}
kc_status kc_s2_decode_streams(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                               uint64_t* out_off, uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return decode_host(c, mode_of(o), src, in_off, n, dst, dst_cap, out_off, status);
}
// the chunk headers of s2/reader.go:259-404 alone
kc_status kc_s2_decode_streams_bound_dev(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                         uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return bound_dev(c, mode_of(o), d_src, in_off, n, bound, status);
}
kc_status kc_s2_decode_streams_bound(kc_ctx* c, const kc_s2_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                     uint32_t* status) {
    if (!o) return KC_ERR_BAD_ARG;
    return bound_host(c, mode_of(o), src, in_off, n, bound, status);
}
// N x s2.Decode(nil, block): s2/decode.go:58-76 -> s2Decode, s2/decode_other.go:22-290
kc_status kc_s2_decode_blocks_all_dev(kc_ctx* c, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                                      uint64_t* out_off, uint32_t* status) {
    return decode_dev_checked(c, mode_blocks(), d_src, in_off, n, d_dst, dst_cap, out_off, status);
}
kc_status kc_s2_decode_blocks_all(kc_ctx* c, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* out_off,
                                  uint32_t* status) {
    return decode_host(c, mode_blocks(), src, in_off, n, dst, dst_cap, out_off, status);
}
// N x s2.DecodedLen(block): s2/decode.go:29-47
kc_status kc_s2_decode_blocks_all_bound_dev(kc_ctx* c, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    return bound_dev(c, mode_blocks(), d_src, in_off, n, bound, status);
}
kc_status kc_s2_decode_blocks_all_bound(kc_ctx* c, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status) {
    return bound_host(c, mode_blocks(), src, in_off, n, bound, status);
}

}  // extern "C"
