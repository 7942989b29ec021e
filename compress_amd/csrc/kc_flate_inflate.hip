// kc_flate_inflate.hip — flate.NewReader / gzip.NewReader over a batch of independent inputs: ONE WAVE PER INPUT, two launches.
//
// The sizing pass walks every input as the write pass will — block headers, tables, every symbol, every rule the reference checks,
// for gzip the headers, the trailers and the ISIZE compare — and writes nothing: it yields the decoded size, the verdict short of
// the CRC-32 and the bytes read.  The host's exclusive scan of the sizes is the output layout; the write pass then decodes every
// input that has something to write straight to its final place, checks each gzip member's CRC-32 wave-wide (s2_crc32c_wave over
// IEEE tables) and zero-fills the range of an input that failed.  Walking the symbols twice is the price of a dense layout
// without a staging copy.  zlib.NewReaderDict has two kernels of its own over the same passes (below): the flate and gzip
// kernels are not touched by it.
//
// No launch can spin on hostile bytes: every loop of kc_flate_dev.h either consumes at least one input bit (byte) per round or
// ends the input, as the comment at each loop says.
#include "kc_flate_dev.h"

__global__ __launch_bounds__(64) void kc_flate_size_kernel(KcFlateParams P) {
    __shared__ FlLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    uint64_t size, used;
    uint32_t members;
    const uint32_t e = fl_input<false>(P, P.in_off[i], P.in_off[i + 1], nullptr, 0, 0, L, &size, &used, &members, lane);
    if (lane == 0) {
        P.size[i] = size;
        P.status[i] = e;
        P.consumed[i] = e ? 0 : used;
        P.members[i] = members;
    }
}

__global__ __launch_bounds__(64) void kc_flate_write_kernel(KcFlateParams P) {
    __shared__ FlLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    const uint32_t members = P.members[i];
    if (members == 0) return;  // nothing planned: the sizing pass's verdict stands
    const uint64_t cap = P.size[i];
    uint8_t* dst = P.dst + P.out0[i];
    uint64_t size, used;
    uint32_t got;
    uint32_t e = fl_input<true>(P, P.in_off[i], P.in_off[i + 1], dst, cap, members, L, &size, &used, &got, lane);
    if (!e && (size != cap || got != members)) e = KCFL_CORRUPT;  // (the two passes disagree: never on the same bytes)
    if (!e) e = P.status[i];  // an error behind the complete members
    if (e) {                   // no byte decoded from a failed input stays
        KC_WAVE_SYNC();
        for (uint64_t k = (uint64_t)lane; k < cap; k += 64) dst[k] = 0;
    }
    if (lane == 0) P.wstatus[i] = e;
}

// zlib.NewReaderDict over the same batch, with the same grid and the same two passes (fl_zlib_input): the sizing pass gives every
// verdict short of the Adler-32; the write pass decodes, sums what it wrote wave-wide (fl_adler32_wave) and zero-fills the planned
// range of an input whose checksum fails.  `members` is 1 for an input that stands so far, else 0.
__global__ __launch_bounds__(64) void kc_zlib_size_kernel(KcFlateParams P) {
    __shared__ FlLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    uint64_t size, used;
    const uint32_t e = fl_zlib_input<false>(P, P.in_off[i], P.in_off[i + 1], nullptr, 0, L, &size, &used, lane);
    if (lane == 0) {
        P.size[i] = size;
        P.status[i] = e;
        P.consumed[i] = e ? 0 : used;
        P.members[i] = e ? 0u : 1u;
    }
}

__global__ __launch_bounds__(64) void kc_zlib_write_kernel(KcFlateParams P) {
    __shared__ FlLds L;
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= P.n) return;
    if (P.members[i] == 0) return;  // nothing planned: the sizing pass's verdict stands
    const uint64_t cap = P.size[i];
    uint8_t* dst = P.dst + P.out0[i];
    uint64_t size, used;
    uint32_t e = fl_zlib_input<true>(P, P.in_off[i], P.in_off[i + 1], dst, cap, L, &size, &used, lane);
    if (!e && size != cap) e = KCFL_CORRUPT;  // (the two passes disagree: never on the same bytes)
    if (e) {                                   // no byte decoded from a failed input stays
        KC_WAVE_SYNC();
        for (uint64_t k = (uint64_t)lane; k < cap; k += 64) dst[k] = 0;
    }
    if (lane == 0) P.wstatus[i] = e;
}

void kc_launch_flate_size(const KcFlateParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_flate_size_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_flate_write(const KcFlateParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_flate_write_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_zlib_size(const KcFlateParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_zlib_size_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_zlib_write(const KcFlateParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_zlib_write_kernel, dim3(P.n), dim3(64), 0, st, P);
}
