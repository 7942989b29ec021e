// kc_zstd_dec_api.cpp — zstd.Decoder.DecodeAll over a batch of independent inputs: the decoder options and the entry points
// kc_zstd_decode_all[_dev] / kc_zstd_decode_all_bound[_dev] of include/kcgpu.h.
//
// One call: the plan kernel sizes every input (kc_zstd_plan.hip, first pass); the inputs are cut into batches whose staging fits the
// context's scratch budget; per batch the plan's second pass writes the frame records, the decode kernel decodes one frame per wave
// into its staging slot (kc_zstd_decode_all.hip), XXH64 of every decoded frame is taken, the host settles each input (first error in
// the reference's order, size limit, checksum: kc_zdec_host.h) and kc_compact_kernel moves the frames of the inputs that stand into
// the dense output.  A failing input therefore never reaches dst at all.
#include "kc_host.h"
#include "kc_zdec_host.h"

namespace {

enum { ZD_IN_OFF, ZD_NF, ZD_BOUND, ZD_SLOTB, ZD_EXACT, ZD_STATUS, ZD_FRAME0, ZD_SLOT0, ZD_FRAMES, ZD_STAGE, ZD_LITS, ZD_DICTS, ZD_ARENA,
       ZD_FSIZE, ZD_FSTATUS, ZD_FCRC, ZD_HASHOFF, ZD_HASH, ZD_COFF, ZD_CSIZE };  // c->zd[]: ZD_COFF holds slot offsets then output offsets

int add_dict(kc_zstd_dopts* o, KcZdDict& D, const uint8_t* content, uint64_t len) {
    if (len > ((uint64_t)1 << 31)) return -1;  // dictMaxLength
    try {
        const size_t at = (o->arena.size() + 15) & ~(size_t)15;
        o->arena.resize(at + (size_t)len);
        if (len) memcpy(o->arena.data() + at, content, (size_t)len);
        D.content_off = at;
        D.content_len = (uint32_t)len;
        o->dicts.push_back(D);
    } catch (...) {
        return -1;
    }
    return 0;
}

struct PlanHost {
    std::vector<uint32_t> nf, exact, status;
    std::vector<uint64_t> bound, slotb;
};

// the plan's first pass over all inputs; its results on the host.  The inputs' offsets and the dictionaries stay on the device.
kc_status plan_inputs(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, KcZdPlanParams& P, PlanHost& H) {
    hipStream_t st = c->stream;
    kc_status s;
    DevBuf* z = c->zd;
    if ((s = ensure(c, z[ZD_IN_OFF], (size_t)(n + 1) * 8)) || (s = ensure(c, z[ZD_NF], (size_t)n * 4)) || (s = ensure(c, z[ZD_BOUND], (size_t)n * 8)) ||
        (s = ensure(c, z[ZD_SLOTB], (size_t)n * 8)) || (s = ensure(c, z[ZD_EXACT], (size_t)n * 4)) || (s = ensure(c, z[ZD_STATUS], (size_t)n * 4)) ||
        (s = ensure(c, z[ZD_FRAME0], (size_t)n * 4)) || (s = ensure(c, z[ZD_SLOT0], (size_t)n * 8)))
        return s;
    HIPCHK(c, hipMemcpyAsync(z[ZD_IN_OFF].p, in_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    memset(&P, 0, sizeof(P));
    if (!o->dicts.empty()) {
        if ((s = ensure(c, z[ZD_DICTS], o->dicts.size() * sizeof(KcZdDict))) || (s = ensure(c, z[ZD_ARENA], o->arena.size() + 16))) return s;
        HIPCHK(c, hipMemcpyAsync(z[ZD_DICTS].p, o->dicts.data(), o->dicts.size() * sizeof(KcZdDict), hipMemcpyHostToDevice, st));
        if (!o->arena.empty()) HIPCHK(c, hipMemcpyAsync(z[ZD_ARENA].p, o->arena.data(), o->arena.size(), hipMemcpyHostToDevice, st));
        P.dicts = (const KcZdDict*)z[ZD_DICTS].p;
        P.n_dicts = (uint32_t)o->dicts.size();
    }
    P.src = d_src;
    P.in_off = (const uint64_t*)z[ZD_IN_OFF].p;
    P.n = n;
    P.max_memory = o->max_memory;
    P.max_window = o->max_window;
    P.n_frames = (uint32_t*)z[ZD_NF].p;
    P.bound = (uint64_t*)z[ZD_BOUND].p;
    P.slot_bytes = (uint64_t*)z[ZD_SLOTB].p;
    P.exact = (uint32_t*)z[ZD_EXACT].p;
    P.status = (uint32_t*)z[ZD_STATUS].p;
    HIPCHK(c, hipEventRecord(c->ev[0], st));
    kc_launch_zstd_plan(P, st);
    HIPCHK(c, hipEventRecord(c->ev[1], st));
    H.nf.resize(n); H.exact.resize(n); H.status.resize(n); H.bound.resize(n); H.slotb.resize(n);
    HIPCHK(c, hipMemcpyAsync(H.nf.data(), P.n_frames, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.exact.data(), P.exact, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.status.data(), P.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.bound.data(), P.bound, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(H.slotb.data(), P.slot_bytes, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
    c->last.prep_ms += t;
    return KC_OK;
}

// device scratch one frame takes besides its staging slot: literal scratch, its record and the per-frame result / compaction arrays
const uint64_t kPerFrame = (uint64_t)KC_ZD_LIT_STRIDE + sizeof(KcZdFrame) + 4 * 4 + 8 * 5 + 64;

kc_status check_args(kc_ctx* c, const kc_zstd_dopts* o, const void* src, const uint64_t* in_off, uint32_t n) {
    if (!c || !o || !in_off || (n && !src)) return KC_ERR_BAD_ARG;
    if (c->pend || c->job_active) return KC_ERR_BAD_ARG;
    c->err.clear();
    for (uint32_t i = 0; i < n; i++)
        if (in_off[i + 1] < in_off[i]) { c->err = "in_off not ascending"; return KC_ERR_BAD_ARG; }
    return KC_OK;
}

kc_status decode_all_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                         uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    c->last_batches = 0;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf* z = c->zd;
    KcZdPlanParams P;
    PlanHost H;
    kc_status s = plan_inputs(c, o, d_src, in_off, n, P, H);
    if (s != KC_OK) return s;
    const uint64_t budget = scratch_budget(c);
    auto input_scratch = [&](uint32_t i) { return H.slotb[i] + (uint64_t)H.nf[i] * kPerFrame; };
    std::vector<uint32_t> frame0(n);
    std::vector<uint64_t> slot0(n);
    std::vector<KcZdFrame> fr;
    std::vector<uint32_t> fsize, fstatus, fcrc, csize;
    std::vector<uint64_t> hash, coff;
    uint64_t pos = 0;  // bytes of dst used
    uint32_t i0 = 0;
    while (i0 < n) {
        // ---- cut: inputs i0 .. i1 whose staging and per-frame scratch fit the budget (ensure() over-allocates by 1/8) ----
        uint32_t i1 = i0, nf = 0;
        uint64_t scratch = 0, slots = 0;
        while (i1 < n) {
            if (H.status[i1] == 0 && H.nf[i1]) {
                const uint64_t us = input_scratch(i1);
                if (us + (us >> 3) > budget) {  // cannot be decoded within the budget even alone: the second pass must skip it too
                    H.status[i1] = KCZD_SIZE;
                    HIPCHK(c, hipMemcpy((uint32_t*)z[ZD_STATUS].p + i1, &H.status[i1], 4, hipMemcpyHostToDevice));
                    i1++;
                    continue;
                }
                if (nf && ((scratch + us) + ((scratch + us) >> 3) > budget || (uint64_t)nf + H.nf[i1] > 0x3FFFFFFFu)) break;
                frame0[i1] = nf;
                slot0[i1] = slots;
                scratch += us;
                slots += H.slotb[i1];
                nf += H.nf[i1];
            }
            i1++;
        }
        const uint32_t nb = i1 - i0;
        std::vector<uint64_t> total(nb, 0);
        if (nf) {
            if ((s = ensure(c, z[ZD_FRAMES], (size_t)nf * sizeof(KcZdFrame))) || (s = ensure(c, z[ZD_STAGE], (size_t)slots + 64)) ||
                (s = ensure(c, z[ZD_LITS], (size_t)nf * KC_ZD_LIT_STRIDE)) || (s = ensure(c, z[ZD_FSIZE], (size_t)nf * 4)) ||
                (s = ensure(c, z[ZD_FSTATUS], (size_t)nf * 4)) || (s = ensure(c, z[ZD_FCRC], (size_t)nf * 4)) ||
                (s = ensure(c, z[ZD_HASHOFF], ((size_t)nf * 2 + 1) * 8)) || (s = ensure(c, z[ZD_HASH], (size_t)nf * 2 * 8)) ||
                (s = ensure(c, z[ZD_COFF], (size_t)nf * 2 * 8)) || (s = ensure(c, z[ZD_CSIZE], (size_t)nf * 4)))
                return s;
            HIPCHK(c, hipMemcpyAsync((uint32_t*)z[ZD_FRAME0].p + i0, frame0.data() + i0, (size_t)nb * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync((uint64_t*)z[ZD_SLOT0].p + i0, slot0.data() + i0, (size_t)nb * 8, hipMemcpyHostToDevice, st));
            KcZdPlanParams Q = P;  // second pass over this batch's inputs: the frame records
            Q.in_off = P.in_off + i0;
            Q.n = nb;
            Q.status = P.status + i0;
            Q.frame0 = (const uint32_t*)z[ZD_FRAME0].p + i0;
            Q.slot0 = (const uint64_t*)z[ZD_SLOT0].p + i0;
            Q.frames = (KcZdFrame*)z[ZD_FRAMES].p;
            KcZdDecodeParams D;
            memset(&D, 0, sizeof(D));
            D.src = d_src;
            D.frames = Q.frames;
            D.n_frames = nf;
            D.stage = (uint8_t*)z[ZD_STAGE].p;
            D.lits = (uint8_t*)z[ZD_LITS].p;
            D.dicts = P.dicts;
            D.dict_arena = (const uint8_t*)z[ZD_ARENA].p;
            D.max_memory = o->max_memory;
            D.out_size = (uint32_t*)z[ZD_FSIZE].p;
            D.status = (uint32_t*)z[ZD_FSTATUS].p;
            D.crc_stored = (uint32_t*)z[ZD_FCRC].p;
            D.hash_off = (uint64_t*)z[ZD_HASHOFF].p;
            HIPCHK(c, hipEventRecord(c->ev[0], st));
            kc_launch_zstd_plan(Q, st);
            HIPCHK(c, hipEventRecord(c->ev[1], st));
            kc_launch_zstd_decode_all(D, st);
            HIPCHK(c, hipEventRecord(c->ev[2], st));
            // XXH64 of every decoded frame: the even "units" of hash_off (the odd ones are the unused rests of the slots)
            if (!o->ignore_checksum) kc_launch_xxh64(D.stage, D.hash_off, 2 * nf - 1, (uint64_t*)z[ZD_HASH].p, st);
            HIPCHK(c, hipEventRecord(c->ev[3], st));
            fr.resize(nf); fsize.resize(nf); fstatus.resize(nf); fcrc.resize(nf); csize.resize(nf); hash.assign((size_t)nf * 2, 0); coff.resize((size_t)nf * 2);
            HIPCHK(c, hipMemcpyAsync(fr.data(), Q.frames, (size_t)nf * sizeof(KcZdFrame), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(fsize.data(), D.out_size, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(fstatus.data(), D.status, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(fcrc.data(), D.crc_stored, (size_t)nf * 4, hipMemcpyDeviceToHost, st));
            if (!o->ignore_checksum) HIPCHK(c, hipMemcpyAsync(hash.data(), z[ZD_HASH].p, ((size_t)nf * 2 - 1) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            float t01 = 0, t12 = 0, t23 = 0;
            (void)hipEventElapsedTime(&t01, c->ev[0], c->ev[1]);
            (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
            (void)hipEventElapsedTime(&t23, c->ev[2], c->ev[3]);
            c->last.prep_ms += t01;
            c->last.match_ms += t12;
            c->last.other_ms += t23;
        }
        // ---- settle the inputs; where their frames go ----
        uint64_t need = 0;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t i = i0 + k;
            if (H.status[i] == 0 && H.nf[i]) {
                const uint32_t f0 = frame0[i];
                H.status[i] = kc_zd_settle_input(fr.data() + f0, fstatus.data() + f0, fsize.data() + f0, fcrc.data() + f0, hash.data() + 2 * (size_t)f0,
                                                 H.nf[i], o->max_memory, o->ignore_checksum != 0, &total[k]);
                if (H.status[i]) total[k] = 0;
            }
            need += total[k];
        }
        if (pos + need > dst_cap) { c->err = "dst_cap too small for the decoded inputs"; return KC_ERR_DST_TOO_SMALL; }
        for (uint32_t f = 0; f < nf; f++) { coff[f] = fr[f].slot_off; coff[(size_t)nf + f] = 0; csize[f] = 0; }  // (a failed input's frames stay in their slots)
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t i = i0 + k;
            status[i] = H.status[i];
            if (H.status[i] == 0 && H.nf[i]) {
                uint64_t at = pos;
                for (uint32_t f = frame0[i]; f < frame0[i] + H.nf[i]; f++) { coff[(size_t)nf + f] = at; csize[f] = fsize[f]; at += fsize[f]; }
            }
            pos += total[k];
            out_off[i + 1] = pos;
        }
        if (nf && need) {
            HIPCHK(c, hipMemcpyAsync(z[ZD_COFF].p, coff.data(), (size_t)nf * 2 * 8, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(z[ZD_CSIZE].p, csize.data(), (size_t)nf * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipEventRecord(c->ev[0], st));
            kc_launch_compact((const uint8_t*)z[ZD_STAGE].p, (const uint64_t*)z[ZD_COFF].p, (const uint32_t*)z[ZD_CSIZE].p,
                              (const uint64_t*)z[ZD_COFF].p + nf, d_dst, nf, st);
            HIPCHK(c, hipEventRecord(c->ev[1], st));
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            float t = 0;
            (void)hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
            c->last.other_ms += t;
        }
        c->last_batches++;
        i0 = i1;
    }
    c->last.total_ms = c->last.prep_ms + c->last.match_ms + c->last.other_ms;
    return KC_OK;
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
    if (!o || n < (uint64_t)kMinWindowSize || n > ((uint64_t)1 << 41) + 7 * ((uint64_t)1 << 38)) return -1;
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
    return add_dict(o, D, content, clen);
}
int kc_zstd_dopts_dict_raw(kc_zstd_dopts* o, uint32_t id, const uint8_t* content, uint64_t len) {  // WithDecoderDictRaw, :131-142
    if (!o || (len && !content)) return -1;
    KcZdDict D;
    memset(&D, 0, sizeof(D));
    D.id = id;
    D.rep[0] = 1; D.rep[1] = 4; D.rep[2] = 8;
    return add_dict(o, D, content, len);
}

kc_status kc_zstd_decode_all_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n, uint8_t* d_dst,
                                 uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, d_src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !d_dst && dst_cap) return KC_ERR_BAD_ARG;
    return decode_all_dev(c, o, d_src, in_off, n, d_dst, dst_cap, out_off, status);
}

kc_status kc_zstd_decode_all_bound_dev(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* d_src, const uint64_t* in_off, uint32_t n,
                                       uint64_t* bound, uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, d_src, in_off, n);
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    c->last = kc_timings{0, 0, 0, 0, 0, 0};
    KcZdPlanParams P;
    PlanHost H;
    if ((s = plan_inputs(c, o, d_src, in_off, n, P, H)) != KC_OK) return s;
    for (uint32_t i = 0; i < n; i++) { bound[i] = H.bound[i]; status[i] = H.status[i]; }
    c->last.total_ms = c->last.prep_ms;
    return KC_OK;
}

// Host buffers: the inputs go to the device in groups of at most a quarter of the scratch budget (input and bound together); a group
// whose decoded bound does not fit is halved, a single input that does not fit gets KC_ZD_SIZE_EXCEEDED.
kc_status kc_zstd_decode_all(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint8_t* dst,
                             uint64_t dst_cap, uint64_t* out_off, uint32_t* status) {
    if (!out_off || (n && !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, src, in_off, n);
    if (s != KC_OK) return s;
    if (n && !dst && dst_cap) return KC_ERR_BAD_ARG;
    out_off[0] = 0;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    kc_timings sum = {0, 0, 0, 0, 0, 0};
    int batches = 0;
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
            if ((s = ensure(c, c->tmp_src, (size_t)bytes + 64)) != KC_OK) return s;
            if (bytes) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src + in_off[i0], (size_t)bytes, hipMemcpyHostToDevice, st));
            rel.resize(nb + 1);
            for (uint32_t k = 0; k <= nb; k++) rel[k] = in_off[i0 + k] - in_off[i0];
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
            sum.prep_ms += c->last.prep_ms; sum.match_ms += c->last.match_ms; sum.other_ms += c->last.other_ms; sum.total_ms += c->last.total_ms;
            batches += c->last_batches;
            break;
        }
        i0 = i1;
    }
    c->last = sum;
    c->last_batches = batches;
    return KC_OK;
}

kc_status kc_zstd_decode_all_bound(kc_ctx* c, const kc_zstd_dopts* o, const uint8_t* src, const uint64_t* in_off, uint32_t n, uint64_t* bound,
                                   uint32_t* status) {
    if (n && (!bound || !status)) return KC_ERR_BAD_ARG;
    kc_status s = check_args(c, o, src, in_off, n);
    if (s != KC_OK || n == 0) return s;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<uint64_t> rel;
    uint32_t i0 = 0;
    while (i0 < n) {  // the plan reads headers only, but they are where they are: groups of inputs that fit a quarter of the budget
        const uint64_t quarter = scratch_budget(c) / 4;
        uint32_t i1 = i0 + 1;
        while (i1 < n && in_off[i1 + 1] - in_off[i0] <= quarter) i1++;
        const uint32_t nb = i1 - i0;
        const uint64_t bytes = in_off[i1] - in_off[i0];
        if (bytes > quarter) { status[i0] = KC_ZD_SIZE_EXCEEDED; bound[i0] = 0; i0 = i1; continue; }
        if ((s = ensure(c, c->tmp_src, (size_t)bytes + 64)) != KC_OK) return s;
        if (bytes) HIPCHK(c, hipMemcpyAsync(c->tmp_src.p, src + in_off[i0], (size_t)bytes, hipMemcpyHostToDevice, st));
        rel.resize(nb + 1);
        for (uint32_t k = 0; k <= nb; k++) rel[k] = in_off[i0 + k] - in_off[i0];
        if ((s = kc_zstd_decode_all_bound_dev(c, o, (const uint8_t*)c->tmp_src.p, rel.data(), nb, bound + i0, status + i0)) != KC_OK) return s;
        i0 = i1;
    }
    return KC_OK;
}

}  // extern "C"
