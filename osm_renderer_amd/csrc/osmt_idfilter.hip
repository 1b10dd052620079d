/*
 * osmt_idfilter.hip — the osm_ids filter of GeodataReader::get_entities_in_tile_with_neighbors (reader.rs:60,95-99,254-262:
 * filter_entities_by_ids keeps an entity iff its global_id() is in the set) as bit-planes: one bit per node, way and
 * multipolygon of a registered geodata file, built once when the set is registered (osmt_register_id_filter) and consulted
 * by the mark kernels of osmt_tilequery.hip and osmt_tilelabels.hip.  gfx950 only.
 *
 *   k_idf_plane   one lane per entity of a kind: a lower-bound bisection of its 64-bit global id in the set, which the host
 *                 sorted and made unique; __ballot of "found" is the wave's 64 bits of the plane, and the wave's first lane
 *                 stores them.  The grid covers the plane's 64-bit words exactly: every word is written here, and the bits
 *                 past the entity count are 0 because their lanes vote 0 — the plane is never cleared beforehand.
 *
 * No LDS, no scratch.  A lane reads gid[e] only for e < n and ids[mid] only for mid < n_ids; a wave stores word e / 64 only
 * while that word is below the n_words the plane was sized with.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t WG = 256u;

/* plane: [n_words] 64-bit words, n_words = ceil(n / 64) */
__global__ __launch_bounds__(256) void k_idf_plane(const uint64_t* __restrict__ gid, uint32_t n, const uint64_t* __restrict__ ids, uint32_t n_ids,
                                                   unsigned long long* __restrict__ plane, uint32_t n_words) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if ((e >> 6) >= n_words) return; /* the waves of the last workgroup behind the plane: uniform over a wave */
    bool found = false;
    if (e < n) {
        const uint64_t g = gid[e];
        uint32_t lo = 0u, hi = n_ids;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (ids[mid] < g)
                lo = mid + 1u;
            else
                hi = mid;
        }
        found = lo < n_ids && ids[lo] == g;
    }
    const unsigned long long m = __ballot(found);
    if ((threadIdx.x & 63u) == 0u) plane[e >> 6] = m;
}

}  // namespace

hipError_t osmt_launch_idf_plane(const uint64_t* gid, uint32_t n, const uint64_t* ids, uint32_t n_ids, uint32_t* plane, hipStream_t st) {
    if (!n) return hipSuccess; /* no entity of the kind: a plane of no words */
    const uint32_t n_words = (n + 63u) / 64u; /* n + 63 does not wrap: n < 2^32 - 64 (osmt_register_id_filter) */
    hipLaunchKernelGGL(k_idf_plane, dim3((n_words + WG / 64u - 1u) / (WG / 64u)), dim3(WG), 0, st, gid, n, ids, n_ids, (unsigned long long*)plane, n_words);
    return hipGetLastError();
}
