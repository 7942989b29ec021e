// kc_zip.hip — zip.File.Open / io.ReadAll over a batch of archive members: four launches, one wave per unit of work.
//
//   locate   one lane per member: the local header, where the body starts and ends inside the buffer, the data descriptor's verdict.
//            The host plans the layout from these and the table (kc_zip_host.h): n small copies of a device-resident archive to
//            the host never happen.
//   inflate  one wave per deflated member: fl_inflate of kc_flate_dev.h in a single pass, the room it may fill being the size the
//            directory states; the CRC-32 of what it wrote wave-wide.  A member whose stated size DEFLATE cannot reach is walked
//            without writing, to learn which error it is (the walk kernel: launched only where the plan has such a member).
//   store    one wave per 64 KiB chunk of every stored member that stands: a large stored member runs at the rate of the whole
//            chip, not of one wave.
//   finish   one wave per member: the stored members' CRC-32 combined from their chunks, the descriptor and CRC rules, the final
//            status, and the range of a failed member zero-filled.
//
// No launch can spin on hostile bytes: the loops of kc_flate_dev.h consume input in every round, the others run over counts the
// host's plan fixed.
#include "kc_zip_dev.h"

__global__ __launch_bounds__(64) void kc_zip_locate_kernel(KcZipParams P) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t < P.n) zp_locate(P, t);
}

__global__ __launch_bounds__(64) void kc_zip_inflate_kernel(KcZipParams P) {
    __shared__ FlLds L;
    if (blockIdx.x < P.n) zp_inflate<true>(P, blockIdx.x, L, (int)threadIdx.x);
}

__global__ __launch_bounds__(64) void kc_zip_walk_kernel(KcZipParams P) {
    __shared__ FlLds L;
    if (blockIdx.x < P.n) zp_inflate<false>(P, blockIdx.x, L, (int)threadIdx.x);
}

__global__ __launch_bounds__(64) void kc_zip_store_kernel(KcZipParams P) {
    __shared__ ZpCrcLds L;
    if (blockIdx.x < P.n_chunks) zp_store(P, blockIdx.x, L, (int)threadIdx.x);
}

__global__ __launch_bounds__(64) void kc_zip_finish_kernel(KcZipParams P) {
    __shared__ ZpPowLds L;
    if (blockIdx.x < P.n) zp_finish(P, blockIdx.x, L, (int)threadIdx.x);
}

void kc_launch_zip_locate(const KcZipParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_zip_locate_kernel, dim3((P.n + 63) / 64), dim3(64), 0, st, P);
}
void kc_launch_zip_inflate(const KcZipParams& P, bool write, hipStream_t st) {
    if (P.n == 0) return;
    if (write) hipLaunchKernelGGL(kc_zip_inflate_kernel, dim3(P.n), dim3(64), 0, st, P);
    else hipLaunchKernelGGL(kc_zip_walk_kernel, dim3(P.n), dim3(64), 0, st, P);
}
void kc_launch_zip_store(const KcZipParams& P, hipStream_t st) {
    if (P.n_chunks == 0) return;
    hipLaunchKernelGGL(kc_zip_store_kernel, dim3(P.n_chunks), dim3(64), 0, st, P);
}
void kc_launch_zip_finish(const KcZipParams& P, hipStream_t st) {
    if (P.n == 0) return;
    hipLaunchKernelGGL(kc_zip_finish_kernel, dim3(P.n), dim3(64), 0, st, P);
}
