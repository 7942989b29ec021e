// kc_zstd_plan.hip — the plan of zstd.Decoder.DecodeAll over a batch of inputs (zstd/decoder.go:319-410, framedec.go:65-278,
// blockdec.go:122-212): one lane per input walks the input the way the reference's frame decoder does — skippable frames, frame
// magic, header descriptor, window descriptor, dictionary id, content size, the chain of 3-byte block headers, the optional
// checksum — until the input is used up, without touching a block's payload.  The first pass sizes the batch (frames, decoded size
// or its bound, staging bytes, first header-level error); the second pass, given where each input's records and staging start,
// writes one KcZdFrame per frame for the decode kernel (kc_zstd_decode_all.hip).  Every read is checked against the input's end.
#include "kc_dev.h"
#include "kc_kernels.h"

namespace {

__device__ __forceinline__ uint32_t zp_ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

__global__ __launch_bounds__(64) void kc_zstd_plan_kernel(KcZdPlanParams P) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= P.n) return;
    const bool emit = P.frames != nullptr;
    if (emit && P.status[u] != 0u) return;  // nothing of a refused input is decoded
    const uint8_t* __restrict__ in = P.src;
    uint64_t pos = P.in_off[u];
    const uint64_t end = P.in_off[u + 1];
    uint32_t nf = 0, st = KCZD_OK;
    uint64_t produced = 0;   // decoded bytes of the frames so far: exact while every frame carried its size, else the bound
    uint64_t known = 0;      // ... counting only the frames that carried their size: what the input has produced AT LEAST (the
                             // exact running total of an input with frames of unknown size is checked by the host after the decode)
    uint64_t slots = 0;      // staging bytes so far (every slot 16-byte aligned)
    bool exact = true;
    while (pos < end) {  // (nothing left: io.EOF from the first read of a frame, which ends DecodeAll without an error)
        if (end - pos < 4) { st = KCZD_EOF; break; }
        const uint32_t magic = zp_ld32(in + pos);
        pos += 4;
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {  // skippable frame: 4-byte length, then that many bytes
            if (end - pos < 4) { st = KCZD_EOF; break; }
            const uint64_t n = zp_ld32(in + pos);
            pos += 4;
            if (end - pos < n) { st = KCZD_EOF; break; }
            pos += n;
            continue;
        }
        if (magic != 0xFD2FB528u) { st = KCZD_MAGIC; break; }
        if (pos >= end) { st = KCZD_EOF; break; }
        const uint32_t fhd = in[pos++];
        const bool single = ((fhd >> 5) & 1u) != 0u;
        if (fhd & 8u) { st = KCZD_CORRUPT; break; }  // reserved bit
        uint64_t window = 0;
        if (!single) {
            if (pos >= end) { st = KCZD_EOF; break; }
            const uint32_t wd = in[pos++];
            const uint64_t base = (uint64_t)1 << (10 + (wd >> 3));
            window = base + (base / 8) * (wd & 7u);
        }
        uint32_t did = 0;
        {
            const uint32_t dsz = (fhd & 3u) == 3u ? 4u : (fhd & 3u);
            if (end - pos < dsz) { st = KCZD_EOF; break; }
            for (uint32_t k = 0; k < dsz; k++) did |= (uint32_t)in[pos + k] << (8 * k);
            pos += dsz;
        }
        uint64_t fcs = KC_ZD_NO_SIZE;
        {
            const uint32_t v = fhd >> 6;
            const uint32_t fsz = v == 0 ? (single ? 1u : 0u) : (1u << v);
            if (end - pos < fsz) { st = KCZD_EOF; break; }
            if (fsz) {
                fcs = 0;
                for (uint32_t k = 0; k < fsz; k++) fcs |= (uint64_t)in[pos + k] << (8 * k);
                if (fsz == 2) fcs += 256;
                pos += fsz;
            }
        }
        const uint32_t checksum = (fhd >> 2) & 1u;
        if (window > P.max_window) { st = KCZD_WINDOW; break; }
        if (window == 0 && single) {
            window = fcs > 1024 ? fcs : 1024;
            if (window > P.max_memory) { st = KCZD_SIZE; break; }
        }
        if (window < 1024) { st = KCZD_CORRUPT; break; }
        // the dictionary is chosen by the frame's id; an id nobody registered is an error unless it is 0 (decoder.go:942-957)
        uint32_t dict = 0;
        for (uint32_t k = 0; k < P.n_dicts; k++) if (P.dicts[k].id == did) dict = k + 1;  // (a later registration replaces an earlier one)
        if (dict == 0 && did != 0) { st = KCZD_UNKNOWN_DICT; break; }
        if (fcs != KC_ZD_NO_SIZE) {
            if (known > P.max_memory || fcs > P.max_memory - known) { st = KCZD_SIZE; break; }
            if (fcs > KC_ZD_MAX_FRAME) { st = KCZD_SIZE; break; }  // (a limit of this path, not of the format: include/kcgpu.h)
        }
        // the chain of block headers
        const uint64_t blk_begin = pos;
        const uint64_t blockMax = window < (128u << 10) ? window : (uint64_t)(128u << 10);
        uint64_t bound = 0;
        for (;;) {
            if (end - pos < 3) { st = KCZD_EOF; break; }
            const uint32_t bh = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16);
            pos += 3;
            const uint32_t type = (bh >> 1) & 3u;
            uint64_t size = bh >> 3;
            if (type == 3) { st = KCZD_CORRUPT; break; }
            if (type == 2) {
                if (size > (128u << 10) || size > window || size < 2) { st = KCZD_CORRUPT; break; }
                bound += blockMax;
            } else {
                if (size > (128u << 10) || size > window) { st = KCZD_WINDOW; break; }
                bound += size;
                if (type == 1) size = 1;
            }
            if (end - pos < size) { st = KCZD_EOF; break; }
            pos += size;
            if (bh & 1u) break;
        }
        if (st) break;
        const uint64_t blk_end = pos;
        if (checksum) {
            if (end - pos < 4) { st = KCZD_EOF; break; }
            pos += 4;
        }
        uint64_t cap = fcs;
        if (fcs == KC_ZD_NO_SIZE) {
            exact = false;
            cap = bound < P.max_memory ? bound : P.max_memory;
            if (cap > KC_ZD_MAX_FRAME) { st = KCZD_SIZE; break; }
        }
        if (emit) {
            KcZdFrame F;
            F.blk_begin = blk_begin; F.blk_end = blk_end; F.window = window; F.fcs = fcs;
            F.slot_off = P.slot0[u] + slots; F.slot_cap = (uint32_t)cap; F.dict = dict; F.checksum = checksum; F.input = u;
            P.frames[P.frame0[u] + nf] = F;
        }
        nf++;
        produced += cap;
        if (fcs != KC_ZD_NO_SIZE) known += fcs;
        slots += (cap + 15) & ~(uint64_t)15;
    }
    if (emit) return;
    if (!exact && produced > P.max_memory) produced = P.max_memory;  // (more than the limit is never returned)
    P.n_frames[u] = st ? 0u : nf;
    P.bound[u] = st ? 0 : produced;
    P.slot_bytes[u] = st ? 0 : slots;
    P.exact[u] = exact ? 1u : 0u;
    P.status[u] = st;
}

void kc_launch_zstd_plan(const KcZdPlanParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_zstd_plan_kernel, dim3((P.n + 63) / 64), dim3(64), 0, st, P);
}
