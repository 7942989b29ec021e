// kc_s2_plan.hip — the plan of s2.Reader / s2.Decode over a batch of inputs: one lane per input runs the chunk walk of
// kc_s2_plan_dev.h (s2/reader.go:259-404; bare blocks: s2.DecodedLen, s2/decode.go:29-47).  The first pass sizes the batch (data
// chunks, decoded bytes, first header-level error per input); the second pass, given where each input's records and output range
// start, writes one KcS2Chunk per data chunk for the decode kernel (kc_s2_decode_all.hip).  S2 sizes are exact before any byte is
// decoded, so the records carry the chunks' final places in dst.
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_s2_plan_dev.h"

__global__ __launch_bounds__(64) void kc_s2_plan_kernel(KcS2PlanParams P) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= P.n) return;
    const bool fill = P.chunks != nullptr;
    const uint8_t* __restrict__ in = P.src;
    const uint64_t pos = P.in_off[u], end = P.in_off[u + 1];
    KcS2Chunk* out = fill ? P.chunks + P.chunk0[u] : nullptr;
    const uint64_t out0 = fill ? P.out0[u] : 0;
    auto emit = [&](uint32_t index, uint64_t body_off, uint32_t body_len, uint32_t kind, uint64_t out_rel, uint32_t dlen, uint32_t crc) {
        if (!fill) return;
        KcS2Chunk C;
        C.body_off = body_off; C.out_off = out0 + out_rel; C.body_len = body_len; C.dlen = dlen; C.crc = crc; C.kind = kind;
        C.stream = u; C.index = index;
        out[index] = C;
    };
    KcS2Walk W;
    if (P.blocks) {  // N x s2.Decode(nil, block): the input is one block
        W.status = KCS2D_OK; W.n_chunks = 0; W.total = 0;
        uint32_t dl = 0, hdr = 0;
        if (end - pos > 0xffffffffull) W.status = KCS2D_SIZE;  // (sizes inside a block are 32-bit here)
        else if (!kc_s2_decoded_len(in, pos, end, &dl, &hdr)) W.status = KCS2D_CORRUPT;
        else {
            emit(0, pos, (uint32_t)(end - pos), KC_S2C_NOCRC, 0, dl, 0);
            W.n_chunks = 1;
            W.total = dl;
        }
    } else {
        W = kc_s2_walk(in, pos, end, P.max_block, P.max_buf, P.ignore_id != 0, emit);
    }
    if (fill) return;
    P.n_chunks[u] = W.n_chunks;
    P.bound[u] = W.total;
    P.status[u] = W.status;
}

void kc_launch_s2_plan(const KcS2PlanParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_s2_plan_kernel, dim3((P.n + 63) / 64), dim3(64), 0, st, P);
}
