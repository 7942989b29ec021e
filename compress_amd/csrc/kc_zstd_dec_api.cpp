// kc_zstd_dec_api.cpp — zstd.Decoder.DecodeAll over a batch of independent inputs: the decoder options and the entry points
// kc_zstd_decode_all[_dev] / kc_zstd_decode_all_bound[_dev] of include/kcgpu.h.  The sequence of one device call is
// kc_zdec_host.h's; this file gives it the device (HipDevice over kc_ctx::zd), checks the arguments and serves host buffers.
#include "kc_decdev_hip.h"

namespace {

static_assert(ZD_N == sizeof(kc_ctx::zd) / sizeof(DevBuf), "kc_ctx::zd has one slot per ZD_* buffer");

kc_status decode_all_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                         uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    KcDecTimes T;
    if (n) HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->zd);
    return take_outcome(c, T, kc_zd_decode_all(&dev, *o, d_src, in_off, n, d_dst, dst_cap, out_off, status, T), "dst_cap too small for the decoded inputs");
}

}  // namespace

extern "C" {

kc_zstd_dopts* kc_zstd_dopts_default(void) {
    try { return new kc_zstd_dopts(); } catch (...) { return nullptr; }
}
void kc_zstd_dopts_free(kc_zstd_dopts* o) { delete o; }
int kc_zstd_dopts_max_memory(kc_zstd_dopts* o, uint64_t n) {  // WithDecoderMaxMemory, zstd/decoder_options.go:90-101
    if (!o || n == 0 || n > ((uint64_t)1 << 63)) return -1;
    o->max_memory = n;
    return 0;
}
int kc_zstd_dopts_max_window(kc_zstd_dopts* o, uint64_t n) {  // WithDecoderMaxWindow, zstd/decoder_options.go:150-161
    if (!o || n < (uint64_t)KC_ZSTD_MIN_WINDOW_SIZE || n > ((uint64_t)1 << 41) + 7 * ((uint64_t)1 << 38)) return -1;
    o->max_window = n;
    return 0;
}
int kc_zstd_dopts_ignore_checksum(kc_zstd_dopts* o, int b) {  // IgnoreChecksum
    if (!o) return -1;
    o->ignore_checksum = b != 0;
    return 0;
}
int kc_zstd_dopts_dict(kc_zstd_dopts* o, const uint8_t* blob, uint64_t len) {  // WithDecoderDicts, zstd/decoder_options.go:112-126
    if (!o || !blob) return -1;
    KcZdDict D;
    const uint8_t* content = nullptr;
    uint64_t clen = 0;
    if (kc_dict_load_decoder(blob, len, &D, &content, &clen) != 0) return -1;
    return kc_zd_add_dict(*o, D, content, clen);
}
int kc_zstd_dopts_dict_raw(kc_zstd_dopts* o, uint32_t id, const uint8_t* content, uint64_t len) {  // WithDecoderDictRaw, :131-142
    if (!o || (len && !content)) return -1;
    return kc_zd_add_dict_raw(*o, id, content, len);
}

kc_status kc_zstd_decode_all_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                 uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = o ? check_batch_args(c, d_src, in_off, n) : KC_ERR_BAD_ARG;
    if (s != KC_OK) return s;
    if (n && !d_dst && dst_cap) return KC_ERR_BAD_ARG;
    return decode_all_dev(c, o, d_src, in_off, n, d_dst, dst_cap, out_off, status);
}

kc_status kc_zstd_decode_all_bound_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                       uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = o ? check_batch_args(c, d_src, in_off, n) : KC_ERR_BAD_ARG;
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    HipDevice dev(c, c->zd);
    KcDecTimes T;
    KcZdPlan H;
    if ((s = take_outcome(c, T, kc_zd_plan_inputs(&dev, *o, d_src, in_off, n, H, T), "", false)) != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) { bound[i] = H.bound[i]; status[i] = H.status[i]; }
    return KC_OK;
}

// Host buffers: the inputs go to the device in groups of at most a quarter of the scratch budget (input and bound together); a group
// whose decoded bound does not fit is halved, a single input that does not fit gets KC_ZD_SIZE_EXCEEDED.
kc_status kc_zstd_decode_all(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                             uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = o ? check_batch_args(c, src, in_off, n) : KC_ERR_BAD_ARG;
    if (s != KC_OK) return s;
    if (n && !dst && dst_cap) return KC_ERR_BAD_ARG;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GroupSum sum;
    uint64_t pos = 0;
    uint32_t i0 = 0;
    std::vector<uint64_t> rel, bound, oo;
    std::vector<uint32_t> stt;
    while (i0 < n) {
        const uint64_t quarter = scratch_budget(c) / 4;
        uint32_t i1 = i0 + 1;
        while (i1 < n && in_off[i1 + 1] - in_off[i0] <= quarter / 2) i1++;
        for (;;) {  // shrink the group until input + bound fit
            const uint32_t nb = i1 - i0;
            const uint64_t bytes = in_off[i1] - in_off[i0];
            if (bytes > quarter && nb == 1) {
                status[i0] = KC_ZD_SIZE_EXCEEDED;
                out_off[i0 + 1] = pos;
                break;
            }
            if ((s = stage_group(c, src, in_off, i0, i1, rel)) != KC_OK) return s;
            bound.resize(nb); stt.resize(nb); oo.resize(nb + 1);
            if ((s = kc_zstd_decode_all_bound_dev(c, o, (const uint8_t*)c->tmp_src.p, rel.data(), nb, bound.data(), stt.data())) != KC_OK) return s;
            uint64_t need = 0;
            for (uint32_t k = 0; k < nb; k++) need += stt[k] ? 0 : bound[k];
            if (bytes + need > quarter) {
                if (nb > 1) { i1 = i0 + nb / 2; continue; }
                status[i0] = KC_ZD_SIZE_EXCEEDED;
                out_off[i0 + 1] = pos;
                break;
            }
            const uint64_t room = dst_cap - pos;
            const uint64_t cap = need < room ? need : room;  // (what does not fit the caller's buffer need not fit ours)
            if ((s = ensure(c, c->tmp_dst, (size_t)cap + 64)) != KC_OK) return s;
            if ((s = decode_all_dev(c, o, (const uint8_t*)c->tmp_src.p, rel.data(), nb, (uint8_t*)c->tmp_dst.p, cap, oo.data(), stt.data())) != KC_OK) return s;
            if (oo[nb]) HIPCHK(c, hipMemcpyAsync(dst + pos, c->tmp_dst.p, (size_t)oo[nb], hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            for (uint32_t k = 0; k < nb; k++) { status[i0 + k] = stt[k]; out_off[i0 + k + 1] = pos + oo[k + 1]; }
            pos += oo[nb];
            sum.add(c);
            break;
        }
        i0 = i1;
    }
    sum.give(c);
    return KC_OK;
}

kc_status kc_zstd_decode_all_bound(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                   uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = o ? check_batch_args(c, src, in_off, n) : KC_ERR_BAD_ARG;
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> rel;
    uint32_t i0 = 0;
    while (i0 < n) {  // the plan reads headers only, but they are where they are: groups of inputs that fit a quarter of the budget
        const uint64_t quarter = scratch_budget(c) / 4;
        uint32_t i1 = i0 + 1;
        while (i1 < n && in_off[i1 + 1] - in_off[i0] <= quarter) i1++;
        const uint32_t nb = i1 - i0;
        const uint64_t bytes = in_off[i1] - in_off[i0];
        if (bytes > quarter) { status[i0] = KC_ZD_SIZE_EXCEEDED; bound[i0] = 0; i0 = i1; continue; }
        if ((s = stage_group(c, src, in_off, i0, i1, rel)) != KC_OK) return s;
        if ((s = kc_zstd_decode_all_bound_dev(c, o, (const uint8_t*)c->tmp_src.p, rel.data(), nb, bound + i0, status + i0)) != KC_OK) return s;
        i0 = i1;
    }
    return KC_OK;
}

}  // extern "C"
