// kc_zstd_first.hip — SpeedFastest: the first-occurrence bits of a batch's units (KcFirstParams in kc_kernels.h has the
// definition and the layout).  One wave per unit, 64 consecutive source positions per step, in position order:
//   * `seen` (2^15 bits in LDS, all the kernel keeps: 4 KiB per wave, so that its waves find room beside a match finder that
//     fills the CU's LDS) holds the hashes of all earlier steps; a lane whose hash is in it is no first occurrence;
//   * the lanes that remain ("candidates") set their bits with atomicOr.  When every candidate finds its bit clear, no two of
//     them share a hash, and every candidate is the first occurrence of its hash: the usual step;
//   * else some candidates of the step share a hash (a 6-byte repetition within 64 bytes, or two hashes that collide): the
//     candidates compare their hashes lane by lane, and the lowest lane of each hash is the first occurrence.  This is exact
//     too, so the kernel marks every first occurrence that has 8 source bytes behind it;
//   * the 64 verdicts of the step are one ballot, stored as one 8-byte word.
// The source bytes of the next ZF1_U steps are loaded while this group of steps works in LDS (the positions are known up front):
// with one step in flight the kernel ran at the latency of a global load per step (9.5 ms per 4 GiB on its own).
#include "kc_dev.h"
#include "kc_kernels.h"
#include "kc_zfast_dev.h"

#define ZF1_U 8  // steps per group: 8 x 8 source bytes per lane in flight

__global__ __launch_bounds__(64) void kc_zfast_first_kernel(KcFirstParams P) {
    __shared__ uint32_t seen[(1u << ZF_TABLE_BITS) / 32];
    const int lane = (int)threadIdx.x;
    const uint32_t u = blockIdx.x;
    if (u >= P.n_units) return;
    const int ulen = (int)(P.unit_off[u + 1] - P.unit_off[u]);
    if (ulen == 0) return;  // (no position, no word)
    const uint8_t* __restrict__ base = P.src + P.unit_off[u];
    const uint64_t rb = (uint64_t)((uintptr_t)P.src & 15) + P.unit_off[u];  // the unit's distance from the bits' origin
    const uint64_t w0 = rb >> 6;
    const int nstep = (int)(((rb + (uint64_t)ulen + 63) >> 6) - w0);
    uint64_t* __restrict__ out = P.bits + w0 + u;
    for (int i = lane; i < (int)((1u << ZF_TABLE_BITS) / 32); i += 64) seen[i] = 0u;
    KC_WAVE_SYNC();
    const int p0 = lane - (int)(rb & 63);  // this lane's position in step 0 (negative: in front of the unit)
    auto inside = [&](int p) -> bool { return p >= 0 && p + 8 <= ulen; };
    uint64_t nxt[ZF1_U];
#pragma unroll
    for (int j = 0; j < ZF1_U; j++) {
        const int p = p0 + 64 * j;
        nxt[j] = inside(p) ? ld64(base + p) : 0;
    }
    for (int k0 = 0; k0 < nstep; k0 += ZF1_U) {  // wave-uniform trip counts throughout
        uint64_t cur[ZF1_U];
#pragma unroll
        for (int j = 0; j < ZF1_U; j++) {
            cur[j] = nxt[j];
            const int p = p0 + 64 * (k0 + ZF1_U + j);
            nxt[j] = inside(p) ? ld64(base + p) : 0;  // (false behind the unit's last step as well)
        }
#pragma unroll
        for (int j = 0; j < ZF1_U; j++) {
            const int k = k0 + j;
            if (k >= nstep) break;
            const bool in = inside(p0 + 64 * k);
            const uint32_t h = hash6(cur[j], ZF_TABLE_BITS);
            const uint32_t bit = 1u << (h & 31u);
            const bool cand = in && (seen[h >> 5] & bit) == 0u;
            KC_WAVE_SYNC();  // every lane has read the state the earlier steps left
            bool win = false;
            if (cand) win = (atomicOr(&seen[h >> 5], bit) & bit) == 0u;
            uint64_t m = ballot64(win);
            if (m != ballot64(cand)) {  // candidates that share a hash: the lowest lane of each is the first occurrence
                const uint32_t hx = cand ? h : 0xFFFFFFFFu;
                bool lower = false;
                for (int d = 1; d < 64; d++) {
                    const uint32_t a = (uint32_t)__shfl_up((int)hx, d, 64);
                    if (lane >= d && a == h) lower = true;
                }
                m = ballot64(cand && !lower);
            }
            if (lane == 0) out[k] = m;
        }
    }
}

void kc_launch_zfast_first(const KcFirstParams& P, hipStream_t st) {
    if (P.n_units == 0) return;
    hipLaunchKernelGGL(kc_zfast_first_kernel, dim3(P.n_units), dim3(64), 0, st, P);
}
