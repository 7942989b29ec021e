// kc_flate_api.cpp — flate.NewReader / flate.NewReaderDict / gzip.NewReader over a batch of independent inputs: the reader options
// and the entry points kc_flate_inflate[_bound][_dev] / kc_gzip_inflate[_bound][_dev] / kc_zlib_inflate[_bound][_dev] of include/kcgpu.h.  The sequence of one
// device call is kc_flate_host.h's; this file gives it the device (HipDevice over kc_ctx::fl), checks the arguments and serves
// host buffers.
#include "kc_decdev_hip.h"
#include "kc_flate_host.h"

struct kc_flate_ropts {
    std::vector<uint8_t> dict;  // flate.NewReaderDict / zlib.NewReaderDict: its last 32 KiB
    uint32_t dict_id = 1;       // adler32 of ALL its bytes (zlib's DICTID; adler32(nil) = 1)
    int multistream = 1;        // gzip.Reader.Multistream
};

namespace {

static_assert(FL_N == sizeof(kc_ctx::fl) / sizeof(DevBuf), "kc_ctx::fl has one slot per FL_* buffer");

KcFlOpts opts_of(const kc_flate_ropts* o, uint32_t format) {
    KcFlOpts f;
    f.format = format; f.multistream = o->multistream; f.dict = o->dict.data(); f.dict_len = (uint32_t)o->dict.size(); f.dict_id = o->dict_id;
    return f;
}

// what both forms check; bound != null: the sizing pass alone
kc_status check_inflate_args(kc_ctx* c, const kc_flate_ropts* o, const void* src, const uint64_t* in_off, uint32_t n, const void* dst, uint64_t dst_cap,
                             const uint64_t* out_off, const uint32_t* status, const uint64_t* bound) {
    if ((!bound && !out_off) || (n && !status) || !o) return KC_ERR_BAD_ARG;
    const kc_status s = check_batch_args(c, src, in_off, n);
    if (s != KC_OK) return s;
    return !bound && n && !dst && dst_cap ? KC_ERR_BAD_ARG : KC_OK;
}

kc_status inflate_dev(kc_ctx* c, const kc_flate_ropts* o, uint32_t format, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                      uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound) {
    kc_status s = check_inflate_args(c, o, d_src, in_off, n, d_dst, dst_cap, out_off, status, bound);
    if (s != KC_OK) return s;
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->fl);
    return take_outcome(c, T, kc_fl_inflate(&dev, opts_of(o, format), d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, bound, T),
                        "dst_cap too small for the planned layout");
}

// Host buffers.  Nothing is known about an input's decoded size before the sizing pass has walked it, so the call makes two sweeps,
// both cut between inputs: the first stages groups of inputs whose bytes fit a quarter of the scratch budget and sizes them — the
// whole layout, and DST_TOO_SMALL before anything is written; the second stages groups whose bytes and decoded bytes together fit
// the quarter, and writes.  (A call that is one group in both sweeps stages its inputs once.)  An input that does not fit alone
// gets KC_FL_SIZE_EXCEEDED: an empty range in the first sweep, its planned range zero-filled in the second.
kc_status host_sweeps(kc_ctx* c, KcDecDevice* dev, const KcFlOpts& o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                      uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound, KcDecTimes& T) {
    hipStream_t st = c->stream;
    const uint64_t quarter = scratch_budget(c) / 4;
    KcFlPlan H;
    H.resize(n);
    std::vector<uint64_t> rel;
    uint32_t res0 = 0, res1 = 0;  // the inputs c->tmp_src holds
    kc_status s;
    auto stage = [&](uint32_t i0, uint32_t i1) -> kc_status {
        const kc_status e = stage_group(c, src, in_off, i0, i1, rel, !(res0 == i0 && res1 == i1));
        if (e != KC_OK) return e;
        res0 = i0; res1 = i1;
        return (kc_status)kc_fl_prepare(dev, o, (const uint8_t*)c->tmp_src.p, rel.data(), i1 - i0, H);
    };
    for (uint32_t i0 = 0; i0 < n;) {  // ---- first sweep: sizes ----
        if (in_off[i0 + 1] - in_off[i0] > quarter) { H.status[i0] = KCFL_SIZE; i0++; continue; }
        uint32_t i1 = i0 + 1;
        while (i1 < n && in_off[i1 + 1] - in_off[i0] <= quarter) i1++;
        if ((s = stage(i0, i1)) != KC_OK || (s = (kc_status)kc_fl_size_inputs(dev, H, i0, T)) != KC_OK) return s;
        i0 = i1;
    }
    if (bound) {
        for (uint32_t i = 0; i < n; i++) { bound[i] = H.size[i]; status[i] = H.status[i]; if (consumed) consumed[i] = H.consumed[i]; }
        return KC_OK;
    }
    for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + H.size[i];
    if (out_off[n] > dst_cap) return KC_ERR_DST_TOO_SMALL;
    auto cost = [&](uint32_t a, uint32_t b) { return (in_off[b] - in_off[a]) + (out_off[b] - out_off[a]); };
    std::vector<uint64_t> oo;
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
        if ((s = (kc_status)kc_fl_write_inputs(dev, H, i0, oo.data(), (uint8_t*)c->tmp_dst.p, status + i0, consumed ? consumed + i0 : nullptr, false, T)) != KC_OK) return s;
        if (need) HIPCHK(c, hipMemcpyAsync(dst + out_off[i0], c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        T.batches++;
        i0 = i1;
    }
    return KC_OK;
}

kc_status inflate_host(kc_ctx* c, const kc_flate_ropts* o, uint32_t format, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* out_off, uint32_t* status, uint64_t* consumed, uint64_t* bound) {
    kc_status s = check_inflate_args(c, o, src, in_off, n, dst, dst_cap, out_off, status, bound);
    if (s != KC_OK) return s;
    KcDecTimes T;
    (void)take_outcome(c, T, KC_OK, "");
    if (!bound) out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->fl);
    return take_outcome(c, T, host_sweeps(c, &dev, opts_of(o, format), src, in_off, n, dst, dst_cap, out_off, status, consumed, bound, T),
                        "dst_cap too small for the planned layout");
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
    o->dict_id = kc_fl_adler32(bytes, len);  // zlib's DICTID is that of the whole dictionary (zlib/reader.go:164-165), not of the window's tail
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
    return inflate_dev(c, o, KCFL_FMT_FLATE, d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_flate_inflate(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_host(c, o, KCFL_FMT_FLATE, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_flate_inflate_bound_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                     uint32_t* status, uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_dev(c, o, KCFL_FMT_FLATE, d_src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
kc_status kc_flate_inflate_bound(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status,
                                 uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_host(c, o, KCFL_FMT_FLATE, src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
// io.ReadAll(gzip.NewReader(input)) per input: gzip/gunzip.go:94-124, 183-295
kc_status kc_gzip_inflate_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                              uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_dev(c, o, KCFL_FMT_GZIP, d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_gzip_inflate(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                          uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_host(c, o, KCFL_FMT_GZIP, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_gzip_inflate_bound_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                    uint32_t* status, uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_dev(c, o, KCFL_FMT_GZIP, d_src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
kc_status kc_gzip_inflate_bound(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status,
                                uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_host(c, o, KCFL_FMT_GZIP, src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}

// io.ReadAll(zlib.NewReaderDict(input, dict)) per input, from a fresh reader: zlib/reader.go:84-91, 134-187 (the header, the
// DICTID), :93-121 (the trailer)
kc_status kc_zlib_inflate_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                              uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_dev(c, o, KCFL_FMT_ZLIB, d_src, in_off, n, d_dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_zlib_inflate(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                          uint64_t* out_off, uint32_t* status, uint64_t* consumed) {
    return inflate_host(c, o, KCFL_FMT_ZLIB, src, in_off, n, dst, dst_cap, out_off, status, consumed, nullptr);
}
kc_status kc_zlib_inflate_bound_dev(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                    uint32_t* status, uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_dev(c, o, KCFL_FMT_ZLIB, d_src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}
kc_status kc_zlib_inflate_bound(kc_ctx* c, const kc_flate_ropts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound, uint32_t* status,
                                uint64_t* consumed) {
    if (n && !bound) return KC_ERR_BAD_ARG;
    uint64_t none = 0;
    return inflate_host(c, o, KCFL_FMT_ZLIB, src, in_off, n, nullptr, 0, nullptr, status, consumed, n ? bound : &none);
}

}  // extern "C"
