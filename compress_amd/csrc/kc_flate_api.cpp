// kc_flate_api.cpp — flate.NewReader / flate.NewReaderDict / gzip.NewReader over a batch of independent inputs: the reader options
// and the entry points kc_flate_inflate[_bound][_dev] / kc_gzip_inflate[_bound][_dev] of include/kcgpu.h.
//
// One call: the sizing pass (kc_flate_inflate.hip) walks every input and yields its decoded size, its verdict short of the CRC-32
// and the bytes it read; the prefix sum of the sizes IS the output layout; the write pass decodes every input straight to its
// place, checks the gzip CRCs and zero-fills what failed.  Nothing is staged and nothing is compacted.
#include "kc_host.h"
#include "kc_flate_dev.h"

struct kc_flate_ropts {
    std::vector<uint8_t> dict;  // flate.NewReaderDict: its last 32 KiB
    int multistream = 1;        // gzip.Reader.Multistream
};

namespace {

enum { FL_IN_OFF, FL_SIZE, FL_STATUS, FL_CONSUMED, FL_MEMBERS, FL_OUT0, FL_WSTATUS, FL_DICT, FL_COUNT };  // c->fl[]
static_assert(FL_COUNT == sizeof(kc_ctx::fl) / sizeof(DevBuf), "kc_ctx::fl has one slot per FL_* buffer");

struct PlanHost {
    std::vector<uint64_t> size, consumed;
    std::vector<uint32_t> status, members;
};

kc_status check_args(kc_ctx* c, const kc_flate_ropts* o, const void* src, const uint64_t* in_off, uint32_t n) {
    if (!c || !o || !in_off || (n && !src)) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    for (uint32_t i = 0; i < n; i++)
        if (in_off[i + 1] < in_off[i]) { c->err = "in_off not ascending"; return KC_ERR_BAD_ARG; }
    return KC_OK;
}

// the device arrays of n inputs and the parameters both passes share
kc_status prepare(kc_ctx* c, const kc_flate_ropts* o, bool gzip, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcFlateParams& P) {
    hipStream_t st = c->stream;
    DevBuf* z = c->fl;
    kc_status s;
    if ((s = ensure(c, z[FL_IN_OFF], (size_t)(n + 1) * 8)) || (s = ensure(c, z[FL_SIZE], (size_t)n * 8)) || (s = ensure(c, z[FL_STATUS], (size_t)n * 4)) ||
        (s = ensure(c, z[FL_CONSUMED], (size_t)n * 8)) || (s = ensure(c, z[FL_MEMBERS], (size_t)n * 4)) || (s = ensure(c, z[FL_OUT0], (size_t)n * 8)) ||
        (s = ensure(c, z[FL_WSTATUS], (size_t)n * 4)))
        return s;
    HIPCHK(c, hipMemcpyAsync(z[FL_IN_OFF].p, in_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    memset(&P, 0, sizeof(P));
    P.src = d_src;
    P.in_off = (const uint64_t*)z[FL_IN_OFF].p;
    P.n = n;
    P.gzip = gzip;
    P.multistream = o->multistream != 0;
    if (!gzip && !o->dict.empty()) {
        if ((s = ensure(c, z[FL_DICT], o->dict.size())) != KC_OK) return s;
        HIPCHK(c, hipMemcpyAsync(z[FL_DICT].p, o->dict.data(), o->dict.size(), hipMemcpyHostToDevice, st));
        P.dict = (const uint8_t*)z[FL_DICT].p;
        P.dict_len = (uint32_t)o->dict.size();
    }
    P.size = (uint64_t*)z[FL_SIZE].p;
    P.status = (uint32_t*)z[FL_STATUS].p;
    P.consumed = (uint64_t*)z[FL_CONSUMED].p;
    P.members = (uint32_t*)z[FL_MEMBERS].p;
    P.out0 = (const uint64_t*)z[FL_OUT0].p;
    P.wstatus = (uint32_t*)z[FL_WSTATUS].p;
    return KC_OK;
}

// the sizing pass over n inputs; its results on the host (appended at H[at ...])
kc_status size_inputs(kc_ctx* c, const KcFlateParams& P, PlanHost& H, uint32_t at) {
    hipStream_t st = c->stream;
    const uint32_t n = P.n;
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    kc_launch_flate_size(P, st);
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    HIPCHK(c, hipMemcpyAsync(H.size.data() + at, P.size, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.status.data() + at, P.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.consumed.data() + at, P.consumed, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.members.data() + at, P.members, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
    c->last.prep_ms += t;
    return KC_OK;
}

// the write pass over the n inputs of P, planned as H[at ...] says, input i at d_dst + out0[i]; the verdicts settle status / consumed
kc_status write_inputs(kc_ctx* c, KcFlateParams P, const PlanHost& H, uint32_t at, const uint64_t* out0, uint8_t* d_dst, uint32_t* status,
                       uint64_t* consumed, bool plan_on_device) {
    hipStream_t st = c->stream;
    const uint32_t n = P.n;
    if (!plan_on_device) {  // the host forms re-group between the sweeps: the plan of THESE inputs goes up again
        HIPCHK(c, hipMemcpyAsync(P.size, H.size.data() + at, (size_t)n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(P.status, H.status.data() + at, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(P.members, H.members.data() + at, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemcpyAsync((void*)P.out0, out0, (size_t)n * 8, hipMemcpyHostToDevice, st));
    P.dst = d_dst;
    std::vector<uint32_t> wst(n);
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    kc_launch_flate_write(P, st);
    HIPCHK(c, hipEventRecord(c->ev[2], st));
    HIPCHK(c, hipMemcpyAsync(wst.data(), P.wstatus, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[1], c->ev[2]);
    c->last.match_ms += t;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = H.members[at + i] ? wst[i] : H.status[at + i];
        status[i] = v;
        if (consumed) consumed[i] = v ? 0 : H.consumed[at + i];
    }
    return KC_OK;
}

void resize(PlanHost& H, uint32_t n) {
    H.size.assign(n, 0); H.consumed.assign(n, 0); H.status.assign(n, 0); H.members.assign(n, 0);
}

kc_status inflate_dev(kc_ctx* c, const kc_flate_ropts* o, bool gzip, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                      uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound) {
    const bool bound_only = bound != nullptr;
    if ((!bound_only && !out_off) || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, d_src, in_off, n);
    if (s != KC_OK) return s;
    if (!bound_only && n && !d_dst && dst_cap) return KC_ERR_BAD_ARG;
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last_batches = 0;
    if (!bound_only) out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    KcFlateParams P;
    PlanHost H;
    resize(H, n);
    if ((s = prepare(c, o, gzip, d_src, in_off, n, P)) != KC_OK || (s = size_inputs(c, P, H, 0)) != KC_OK) return s;
    if (bound_only) {
        for (uint32_t i = 0; i < n; i++) { bound[i] = H.size[i]; status[i] = H.status[i]; if (consumed) consumed[i] = H.consumed[i]; }
        c->last.total_ms = c->last.prep_ms;
        return KC_OK;
    }
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.size[i];  // the planned layout
    if (out_off[n] > dst_cap) { c->err = "dst_cap too small for the planned layout"; return KC_ERR_DST_TOO_SMALL; }  // (nothing written yet)
    if ((s = write_inputs(c, P, H, 0, out_off, d_dst, status, consumed, true)) != KC_OK) return s;
    c->last_batches = 1;
    c->last.total_ms = c->last.prep_ms + c->last.match_ms;
    return KC_OK;
}

// Host buffers.  Nothing is known about an input's decoded size before the sizing pass has walked it, so the call makes two sweeps,
// both cut between inputs: the first stages groups of inputs whose bytes fit a quarter of the scratch budget and sizes them — the
// whole layout, and DST_TOO_SMALL before anything is written; the second stages groups whose bytes and decoded bytes together fit
// the quarter, and writes.  (A call that is one group in both sweeps stages its inputs once.)  An input that does not fit alone
// gets KC_FL_SIZE_EXCEEDED: an empty range in the first sweep, its planned range zero-filled in the second.
kc_status inflate_host(kc_ctx* c, const kc_flate_ropts* o, bool gzip, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound) {
    const bool bound_only = bound != nullptr;
    if ((!bound_only && !out_off) || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, src, in_off, n);
    if (s != KC_OK) return s;
    if (!bound_only && n && !dst && dst_cap) return KC_ERR_BAD_ARG;
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last_batches = 0;
    if (!bound_only) out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const uint64_t quarter = scratch_budget(c) / 4;
    PlanHost H;
    resize(H, n);
    KcFlateParams P;
    std::vector<uint64_t> rel;
    uint32_t res0 = 0, res1 = 0;  // the inputs c->tmp_src holds
    int groups = 0;
    auto stage = [&](uint32_t i0, uint32_t i1) -> kc_status {
        const uint64_t bytes = in_off[i1] - in_off[i0];
        kc_status e;
        if ((e = ensure(c, c->tmp_src, (size_t)bytes + 64)) != KC_OK) return e;
        if (bytes && !(res0 == i0 && res1 == i1)) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src + in_off[i0], (size_t)bytes, hipMemcpyHostToDevice, st));
        res0 = i0; res1 = i1;
        rel.resize(i1 - i0 + 1);
        for (uint32_t k = 0; k <= i1 - i0; k++) rel[k] = in_off[i0 + k] - in_off[i0];
        return prepare(c, o, gzip, (const uint8_t*)c->tmp_src.p, rel.data(), i1 - i0, P);
    };
    for (uint32_t i0 = 0; i0 < n;) {  // ---- first sweep: sizes ----
        if (in_off[i0 + 1] - in_off[i0] > quarter) { H.status[i0] = KCFL_SIZE; i0++; continue; }
        uint32_t i1 = i0 + 1;
        while (i1 < n && in_off[i1 + 1] - in_off[i0] <= quarter) i1++;
        if ((s = stage(i0, i1)) != KC_OK || (s = size_inputs(c, P, H, i0)) != KC_OK) return s;
        groups++;
        i0 = i1;
    }
    if (bound_only) {
        for (uint32_t i = 0; i < n; i++) { bound[i] = H.size[i]; status[i] = H.status[i]; if (consumed) consumed[i] = H.consumed[i]; }
        c->last.total_ms = c->last.prep_ms;
        return KC_OK;
    }
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.size[i];
    if (out_off[n] > dst_cap) { c->err = "dst_cap too small for the planned layout"; return KC_ERR_DST_TOO_SMALL; }
    auto cost = [&](uint32_t a, uint32_t b) { return (in_off[b] - in_off[a]) + (out_off[b] - out_off[a]); };
    std::vector<uint64_t> oo;
    groups = 0;
    for (uint32_t i0 = 0; i0 < n;) {  // ---- second sweep: the bytes ----
        if (cost(i0, i0 + 1) > quarter) {
            status[i0] = KCFL_SIZE;
            if (consumed) consumed[i0] = 0;
            if (H.size[i0]) memset(dst + out_off[i0], 0, (size_t)H.size[i0]);
            i0++;
            continue;
        }
        uint32_t i1 = i0 + 1;
        while (i1 < n && cost(i0, i1 + 1) <= quarter) i1++;
        const uint32_t nb = i1 - i0;
        const uint64_t need = out_off[i1] - out_off[i0];
        if ((s = stage(i0, i1)) != KC_OK || (s = ensure(c, c->tmp_dst, (size_t)need + 64)) != KC_OK) return s;
        oo.resize(nb);
        for (uint32_t k = 0; k < nb; k++) oo[k] = out_off[i0 + k] - out_off[i0];
        if ((s = write_inputs(c, P, H, i0, oo.data(), (uint8_t*)c->tmp_dst.p, status + i0, consumed ? consumed + i0 : nullptr, false)) != KC_OK) return s;
        if (need) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        groups++;
        i0 = i1;
    }
    c->last_batches = groups;
    c->last.total_ms = c->last.prep_ms + c->last.match_ms;
    return KC_OK;
}

}  // namespace

extern "C" {

kc_flate_ropts* kc_flate_ropts_default(void) {
    try { return new kc_flate_ropts(); } catch (...) { return nullptr; }
}
void kc_flate_ropts_free(kc_flate_ropts* o) { delete o; }
int kc_flate_ropts_dict(kc_flate_ropts* o, const uint8_t* bytes, uint64_t len) {  // flate.NewReaderDict, flate/inflate.go:948-957: the window's worth counts
    if (!o || (len && !bytes)) return -1;
    const uint64_t keep = len > 32768 ? 32768 : len;
    try { o->dict.assign(bytes + (len - keep), bytes + len); } catch (...) { return -1; }
    return 0;
}
int kc_flate_ropts_multistream(kc_flate_ropts* o, int b) {  // gzip.Reader.Multistream, gzip/gunzip.go:142-144
    if (!o) return -1;
    o->multistream = b != 0;
    return 0;
}

// io.ReadAll(flate.NewReaderDict(input, dict)) per input: flate/inflate.go:352-395, 464-597, 600-670, flate/inflate_gen.go
kc_status kc_flate_inflate_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                               uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_dev(c, o, false, d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_flate_inflate(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_host(c, o, false, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_flate_inflate_bound_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                     uint32_t* status, uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_dev(c, o, false, d_src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
kc_status kc_flate_inflate_bound(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status,
                                 uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_host(c, o, false, src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
// io.ReadAll(gzip.NewReader(input)) per input: gzip/gunzip.go:94-124, 183-295
kc_status kc_gzip_inflate_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                              uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_dev(c, o, true, d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_gzip_inflate(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                          uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_host(c, o, true, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_gzip_inflate_bound_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                    uint32_t* status, uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_dev(c, o, true, d_src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
kc_status kc_gzip_inflate_bound(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status,
                                uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_host(c, o, true, src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}

}  // extern "C"
