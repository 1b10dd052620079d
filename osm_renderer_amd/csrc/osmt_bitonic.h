/* osmt_bitonic.h — the one-direction bitonic network of the per-tile sorts (k_styled_sort: 16-byte keys, k_tq_sort: 32-bit ids). */
#ifndef OSMT_BITONIC_H
#define OSMT_BITONIC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

template <typename K, typename Less>
__device__ __forceinline__ void osmt_cmpx(K* k, uint32_t i, uint32_t l, Less less) {
    const K a = k[i], b = k[l];
    if (less(b, a)) {
        k[i] = b;
        k[l] = a;
    }
}

/* k[0 .. n) ascending under the total order `less`, by a workgroup of WG lanes; N = the power of two >= n.  First step of a
 * merge mirrors, the others shift.  Slots n .. N - 1 are +inf and exist only in the index arithmetic: every exchange puts the
 * smaller key at the smaller index, so a pair that reaches into them is a no-op.  k may be LDS or device memory (a workgroup
 * sees its own global stores behind a barrier).  Every block size is a power of two: shifts and masks, no division. */
template <uint32_t WG, typename K, typename Less>
__device__ __forceinline__ void osmt_bitonic(K* k, uint32_t n, uint32_t N, Less less) {
    for (uint32_t lk = 1u; (1u << lk) <= N; ++lk) { /* merges of 2^lk keys */
        const uint32_t k2 = 1u << lk, lh = lk - 1u, h = 1u << lh;
        for (uint32_t p = threadIdx.x; p < (N >> 1); p += WG) { /* mirror step */
            const uint32_t blk = p >> lh, w = p & (h - 1u);
            const uint32_t i = blk * k2 + w, l = blk * k2 + (k2 - 1u - w);
            if (l < n) osmt_cmpx(k, i, l, less);
        }
        __syncthreads();
        for (uint32_t lj = lh; lj-- > 0u;) { /* j = 2^lj = k2 / 4 .. 1 */
            const uint32_t j = 1u << lj;
            for (uint32_t p = threadIdx.x; p < (N >> 1); p += WG) {
                const uint32_t blk = p >> lj, w = p & (j - 1u);
                const uint32_t i = blk * 2u * j + w, l = i + j;
                if (l < n) osmt_cmpx(k, i, l, less);
            }
            __syncthreads();
        }
    }
}

#endif
