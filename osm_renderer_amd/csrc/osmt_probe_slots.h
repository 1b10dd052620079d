/*
 * osmt_probe_slots.h — where a key's probe starts, and how many slots its table has, in the two open-addressing tables of
 * the importer: the pair table of the way dedup (k_res_short, osmt_resolve.hip: one table in LDS per way) and the vertex
 * table of the multipolygon assembly (k_mpa_vertices, k_mpa_canon, osmt_polygons.hip: one table in device memory per call,
 * sized by osmt_host_polygons.cpp).
 *
 * Both tables probe linearly, (slot + 1) & mask, and both hold at most half as many keys as they have slots.  Which keys'
 * probes cross from the last slot to slot 0 follows from this arithmetic and the keys alone, whatever order the lanes arrive
 * in, so a host test can count them for a world before the device sees it.
 *
 * Shared with a host test (tests/probe_slots_shim.cpp).
 */
#ifndef OSMT_PROBE_SLOTS_H
#define OSMT_PROBE_SLOTS_H

#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

/* ---- the pair table: keyed by the unordered pair of two node indices ---- */

/* min << 32 | max; never all ones: an index is below 2^32 - 1 */
OSMT_HD unsigned long long osmt_pair_key(uint32_t a, uint32_t b) {
    return a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
}

OSMT_HD uint32_t osmt_pair_hash(unsigned long long k) {
    k *= 0x9E3779B97F4A7C15ull;
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    return (uint32_t)(k >> 32);
}

/* slots of the table of a way of len >= 1 resolved references (len - 1 pairs): 64, doubled until >= 2 * (len - 1) */
OSMT_HD uint32_t osmt_pair_slots(uint32_t len) {
    uint32_t slots = 64u;
    while (slots < 2u * (len - 1u)) slots <<= 1;
    return slots;
}

/* ---- the vertex table: keyed by (relation, lat bits, lon bits) ---- */

OSMT_HD uint32_t osmt_vertex_hash(unsigned long long lat_bits, unsigned long long lon_bits, uint32_t rel) {
    unsigned long long h = lat_bits * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h = (h + lon_bits) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    h = (h + rel) * 0x94D049BB133111EBull;
    return (uint32_t)(h >> 32);
}

/* hash_bits: 32, or fewer to make chains long (osmt_debug_vertex_hash_bits); table_mask: slots - 1 */
OSMT_HD uint32_t osmt_vertex_first_slot(unsigned long long lat_bits, unsigned long long lon_bits, uint32_t rel, uint32_t hash_bits, uint32_t table_mask) {
    const uint32_t keep = hash_bits >= 32u ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
    return osmt_vertex_hash(lat_bits, lon_bits, rel) & keep & table_mask;
}

/* slots of the table of `endpoints` endpoints: 64, doubled until >= 2 * endpoints, 2^32 at the most (endpoints < 2^32: then
 * still more slots than endpoints) */
OSMT_HD uint64_t osmt_vertex_slots(uint64_t endpoints) {
    uint64_t slots = 64;
    while (slots < 2 * endpoints && slots < (1ull << 32)) slots <<= 1;
    return slots;
}

#endif
