// Host build of the slot arithmetic of the importer's two open-addressing tables (osmt_probe_slots.h) for
// tests/_probe_slots.py: the header's six functions one by one and over arrays, and the two tables filled sequentially with
// the header's own slots, counting the probe steps that go from the last slot to slot 0.
#include "../osm_renderer_amd/csrc/osmt_probe_slots.h"

#include <stddef.h>

#include <vector>

namespace {

// One probe as a kernel's loop walks it: from `slot` on until same(resident) or an empty slot; counts its steps and whether it
// stepped from the last slot to slot 0.
struct probe_stats {
    uint64_t crossings = 0;  // probe steps from the last slot to slot 0, over all probes
    uint32_t longest = 0;    // the steps of the longest probe that took such a step
    void probe_done(uint32_t steps, bool crossed) {
        if (crossed && steps > longest) longest = steps;
    }
};

}  // namespace

extern "C" {

unsigned long long shim_pair_key(uint32_t a, uint32_t b) { return osmt_pair_key(a, b); }
uint32_t shim_pair_hash(unsigned long long k) { return osmt_pair_hash(k); }
uint32_t shim_pair_slots(uint32_t len) { return osmt_pair_slots(len); }
uint32_t shim_vertex_hash(unsigned long long lat, unsigned long long lon, uint32_t rel) { return osmt_vertex_hash(lat, lon, rel); }
uint32_t shim_vertex_first_slot(unsigned long long lat, unsigned long long lon, uint32_t rel, uint32_t hash_bits, uint32_t table_mask) {
    return osmt_vertex_first_slot(lat, lon, rel, hash_bits, table_mask);
}
uint64_t shim_vertex_slots(uint64_t endpoints) { return osmt_vertex_slots(endpoints); }

// the home slot of the pair (a, b[i]) in a table of mask + 1 slots, for every i
void shim_pair_homes(uint32_t a, const uint32_t* b, size_t n, uint32_t mask, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = osmt_pair_hash(osmt_pair_key(a, b[i])) & mask;
}

// the home slot of every position bits[2 i], bits[2 i + 1] under relation rel
void shim_vertex_homes(const unsigned long long* bits, size_t n, uint32_t rel, uint32_t hash_bits, uint32_t mask, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = osmt_vertex_first_slot(bits[2 * i], bits[2 * i + 1], rel, hash_bits, mask);
}

// k_res_short's table, way by way, over RESOLVED references (off [n_ways + 1], refs): positions 1 .. len - 1 enter in order.
// per_way[2 w] = the way's crossing steps, per_way[2 w + 1] = its longest crossing probe; ways of fewer than 3 references or
// more than short_max have no table.  Returns the number of ways with at least one crossing step.
uint64_t shim_pair_crossings(const uint32_t* off, const uint32_t* refs, size_t n_ways, uint32_t short_max, uint32_t* per_way) {
    const unsigned long long EMPTY = ~0ull;
    uint64_t ways_crossing = 0;
    std::vector<unsigned long long> tkey;
    for (size_t w = 0; w < n_ways; ++w) {
        const uint32_t b = off[w], len = off[w + 1] - b;
        per_way[2 * w] = per_way[2 * w + 1] = 0u;
        if (len <= 2u || len > short_max) continue;
        const uint32_t slots = osmt_pair_slots(len), mask = slots - 1u;
        tkey.assign(slots, EMPTY);
        probe_stats st;
        for (uint32_t i = 1u; i < len; ++i) {
            const unsigned long long k = osmt_pair_key(refs[b + i - 1u], refs[b + i]);
            uint32_t slot = osmt_pair_hash(k) & mask, steps = 0u;
            bool crossed = false;
            while (tkey[slot] != EMPTY && tkey[slot] != k) {
                if (slot == mask) crossed = true, ++st.crossings;
                slot = (slot + 1u) & mask;
                ++steps;
            }
            tkey[slot] = k;
            st.probe_done(steps, crossed);
        }
        per_way[2 * w] = (uint32_t)st.crossings, per_way[2 * w + 1] = st.longest;
        if (st.crossings) ++ways_crossing;
    }
    return ways_crossing;
}

// k_mpa_vertices' table over the relations' segments as k_mpa_segments lays them out: endpoint e = 2 * segment + side enters
// in order, a resident of the same relation and position bits is its own vertex.  out[0] = crossing steps, out[1] = the
// longest crossing probe, out[2] = the table's slots, out[3] = endpoints.
void shim_vertex_crossings(const unsigned long long* node_bits, const uint32_t* way_off, const uint32_t* way_nodes, const uint32_t* rel_way_off,
                           const uint32_t* rel_ways, size_t n_rels, uint32_t hash_bits, uint64_t* out) {
    std::vector<uint32_t> seg_node, seg_rel;  // per endpoint, per segment
    for (size_t r = 0; r < n_rels; ++r)
        for (uint32_t j = rel_way_off[r]; j < rel_way_off[r + 1]; ++j) {
            const uint32_t w = rel_ways[j];
            for (uint32_t at = way_off[w]; at + 1u < way_off[w + 1]; ++at) {
                seg_node.push_back(way_nodes[at]), seg_node.push_back(way_nodes[at + 1u]);
                seg_rel.push_back((uint32_t)r);
            }
        }
    const uint64_t E = seg_node.size(), slots = osmt_vertex_slots(E);
    const uint32_t mask = (uint32_t)(slots - 1), NONE = 0xFFFFFFFFu;
    std::vector<uint32_t> table(E ? slots : 0, NONE);
    probe_stats st;
    for (uint64_t e = 0; e < E; ++e) {
        const uint32_t rel = seg_rel[e >> 1];
        const unsigned long long lat = node_bits[2 * (size_t)seg_node[e]], lon = node_bits[2 * (size_t)seg_node[e] + 1];
        uint32_t slot = osmt_vertex_first_slot(lat, lon, rel, hash_bits, mask), steps = 0u;
        bool crossed = false;
        for (;;) {
            const uint32_t cur = table[slot];
            if (cur == NONE) {
                table[slot] = (uint32_t)e;
                break;
            }
            if (seg_rel[cur >> 1] == rel && node_bits[2 * (size_t)seg_node[cur]] == lat && node_bits[2 * (size_t)seg_node[cur] + 1] == lon) break;
            if (slot == mask) crossed = true, ++st.crossings;
            slot = (slot + 1u) & mask;
            ++steps;
        }
        st.probe_done(steps, crossed);
    }
    out[0] = st.crossings, out[1] = st.longest, out[2] = E ? slots : 0, out[3] = E;
}
}
