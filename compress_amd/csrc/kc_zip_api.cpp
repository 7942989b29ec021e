// kc_zip_api.cpp — zip.File.Open / io.ReadAll over a table of archive members: the entry points kc_zip_read_dev / kc_zip_read /
// kc_zip_read_bound of include/kcgpu.h.  The sequence of one device call is kc_zip_host.h's; this file gives it the device
// (HipDevice over kc_ctx::zp), checks the arguments and serves host buffers.  The directory is read elsewhere, without a device
// (kc_zip_dir.cpp).
#include "kc_decdev_hip.h"
#include "kc_zip_host.h"

namespace {

static_assert(ZP_N == sizeof(kc_ctx::zp) / sizeof(DevBuf), "kc_ctx::zp has one slot per ZP_* buffer");

kc_status check_zip_args(kc_ctx* c, const void* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, const void* dst, uint64_t dst_cap,
                         const uint64_t* out_off, const uint32_t* status, bool bound) {
    if (!c || !out_off || (n && (!status || !members)) || (src_len && !src)) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    return !bound && n && !dst && dst_cap ? KC_ERR_BAD_ARG : KC_OK;
}

// Host buffers: the archive is staged whole (the members' offsets are absolute in it), the layout is planned from the local
// headers, the decoded bytes come back in one copy.  The rolling host pipeline is not used.
kc_status read_host(kc_ctx* c, const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                    uint64_t* out_off, uint32_t* status, bool bound) {
    kc_status s = check_zip_args(c, src, src_len, members, n, dst, dst_cap, out_off, status, bound);
    if (s != KC_OK) return s;
    KcDecTimes T;
    (void)take_outcome(c, T, KC_OK, "");
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (src_len > scratch_budget(c)) { c->err = "the archive exceeds the scratch budget"; return KC_ERR_UNSUPPORTED; }
    if ((s = ensure(c, c->tmp_src, (size_t)src_len + 64)) != KC_OK) return s;
    if (src_len) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src, (size_t)src_len, hipMemcpyHostToDevice, c->stream));
    HipDevice dev(c, c->zp);
    const uint8_t* d_src = (const uint8_t*)c->tmp_src.p;
    int r = kc_zp_read(&dev, d_src, src_len, members, n, nullptr, 0, out_off, status, true, T);
    if (r != KC_OK || bound) {
        if (r == KC_OK) HIPCHK(c, hipStreamSynchronize(c->stream));
        return take_outcome(c, T, r, "");
    }
    const uint64_t need = out_off[n];
    if (need > dst_cap) return take_outcome(c, T, KC_ERR_DST_TOO_SMALL, "dst_cap too small for the planned layout");
    if (src_len + need > scratch_budget(c)) { c->err = "the archive and its members exceed the scratch budget"; return KC_ERR_UNSUPPORTED; }
    if ((s = ensure(c, c->tmp_dst, (size_t)need + 64)) != KC_OK) return s;
    T = KcDecTimes();
    r = kc_zp_read(&dev, d_src, src_len, members, n, (uint8_t*)c->tmp_dst.p, need, out_off, status, false, T);
    if (r == KC_OK) {
        if (need) HIPCHK(c, hipMemcpyAsync(dst, c->tmp_dst.p, (size_t)need, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return take_outcome(c, T, r, "dst_cap too small for the planned layout");
}

}  // namespace

extern "C" {

// f.Open(); io.ReadAll; Close per member: zip/reader.go:247-362, 368-381, 566-603
kc_status kc_zip_read_dev(kc_ctx* c, const uint8_t* d_src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* d_dst, uint64_t dst_cap,
                          uint64_t* out_off, uint32_t* status) {
    kc_status s = check_zip_args(c, d_src, src_len, members, n, d_dst, dst_cap, out_off, status, false);
    if (s != KC_OK) return s;
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->zp);
    return take_outcome(c, T, kc_zp_read(&dev, d_src, src_len, members, n, d_dst, dst_cap, out_off, status, false, T),
                        "dst_cap too small for the planned layout");
}
kc_status kc_zip_read(kc_ctx* c, const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                      uint64_t* out_off, uint32_t* status) {
    return read_host(c, src, src_len, members, n, dst, dst_cap, out_off, status, false);
}
kc_status kc_zip_read_bound(kc_ctx* c, const uint8_t* src, uint64_t src_len, const kc_zip_member* members, uint32_t n, uint64_t* out_off, uint32_t* status) {
    return read_host(c, src, src_len, members, n, nullptr, 0, out_off, status, true);
}

}  // extern "C"
