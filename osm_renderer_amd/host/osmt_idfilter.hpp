/*
 * osmt_idfilter.hpp — host side of the osm_ids filter (include/osmtile.h, osmt_register_id_filter):
 *
 *   id_filter_set    the one host step of a registration: the caller's ids, sorted and made unique — what the device bisects;
 *   id_filter_plane  the host twin of k_idf_plane (csrc/osmt_idfilter.hip): one bit per entity, whole 64-bit words, the bits
 *                    past the entity count 0.  The yardstick of the kernel's tests next to np.isin.
 *
 * The filter itself — filter_entities_by_ids (reader.rs:254-262) — is the osm_ids argument of
 * GeodataReader::get_entities_in_tile_with_neighbors (host/osmt_geodata.hpp).  Host only, no HIP.
 */
#ifndef OSMT_IDFILTER_HPP
#define OSMT_IDFILTER_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace osmt {

inline std::vector<uint64_t> id_filter_set(const uint64_t* ids, size_t n) {
    std::vector<uint64_t> set(ids, ids + n); /* n == 0: an empty range, ids is not read */
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    return set;
}

/* bit e % 32 of word e / 32 = gids[e] is in `set` (ascending, unique); 2 * ceil(n / 64) words */
inline std::vector<uint32_t> id_filter_plane(const uint64_t* gids, size_t n, const std::vector<uint64_t>& set) {
    std::vector<uint32_t> plane((n + 63) / 64 * 2, 0u);
    for (size_t e = 0; e < n; ++e)
        if (std::binary_search(set.begin(), set.end(), gids[e])) plane[e >> 5] |= 1u << (e & 31);
    return plane;
}

}  // namespace osmt
#endif
