/*
 * osmt_resolve.hpp — OSM ids resolved on the host: osmt::RawOsmDesc builds the arrays osmt_resolve_refs takes,
 * osmt::resolve_refs_host is the host twin of that call — a plain restatement of OsmEntityStorage::translate_id
 * (importer.rs:45-71), the silent drop of references that do not resolve (importer.rs:365-400) and postprocess_node_refs
 * (importer.rs:334-353), with a hash map and a hash set as the importer has them — and the yardstick of the GPU tests.
 * Host only: no HIP, no device.
 */
#ifndef OSMT_RESOLVE_HPP
#define OSMT_RESOLVE_HPP

#include <cstdint>
#include <set>
#include <stdexcept>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"

namespace osmt {

/* The arrays of an osmt_raw_osm_desc with owning vectors, filled in file order.  view() points into them: valid until the
 * next add_*.  With track_seen every way (relation) records how many nodes (ways) were added before it; without, the
 * *_seen arrays stay NULL: every element is visible to every reference. */
struct RawOsmDesc {
    std::vector<uint64_t> node_ids, way_ids, way_refs, relation_refs;
    std::vector<uint32_t> way_ref_off{0u}, relation_ref_off{0u}, way_nodes_seen, relation_ways_seen;
    std::vector<uint8_t> relation_ref_inner;
    bool track_seen = false;

    void add_node(uint64_t global_id) { node_ids.push_back(global_id); }
    void add_way(uint64_t global_id, const std::vector<uint64_t>& node_refs) {
        way_ids.push_back(global_id);
        way_refs.insert(way_refs.end(), node_refs.begin(), node_refs.end());
        if (way_refs.size() >= 0xFFFFFFFFull || node_ids.size() >= 0xFFFFFFFFull) throw std::runtime_error("raw OSM data too large for 32-bit offsets");
        way_ref_off.push_back((uint32_t)way_refs.size());
        if (track_seen) way_nodes_seen.push_back((uint32_t)node_ids.size());
    }
    /* members: (way id, is_inner) of the type="way" members in the relation's order */
    void add_relation(const std::vector<std::pair<uint64_t, bool>>& members) {
        for (const auto& m : members) relation_refs.push_back(m.first), relation_ref_inner.push_back(m.second ? 1u : 0u);
        if (relation_refs.size() >= 0xFFFFFFFFull || way_ids.size() >= 0xFFFFFFFFull) throw std::runtime_error("raw OSM data too large for 32-bit offsets");
        relation_ref_off.push_back((uint32_t)relation_refs.size());
        if (track_seen) relation_ways_seen.push_back((uint32_t)way_ids.size());
    }
    osmt_raw_osm_desc view() const {
        osmt_raw_osm_desc d{};
        d.node_ids = node_ids.data(), d.n_nodes = node_ids.size();
        d.way_ids = way_ids.data(), d.way_ref_off = way_ref_off.data(), d.n_ways = way_ids.size();
        d.way_refs = way_refs.data(), d.n_way_refs = way_refs.size();
        d.relation_ref_off = relation_ref_off.data(), d.n_relations = relation_ref_off.size() - 1;
        d.relation_refs = relation_refs.data(), d.relation_ref_inner = relation_ref_inner.data(), d.n_relation_refs = relation_refs.size();
        d.way_nodes_seen = track_seen ? way_nodes_seen.data() : nullptr;
        d.relation_ways_seen = track_seen ? relation_ways_seen.data() : nullptr;
        return d;
    }
};

/* What a resolution gives: the way and relation arrays of osmt_relations_desc / osmt_geodata_desc, and the five counts of
 * osmt_resolved_counts. */
struct ResolvedRefs {
    std::vector<uint32_t> way_node_off{0u}, way_nodes, relation_way_off{0u}, relation_ways;
    std::vector<uint8_t> relation_way_inner;
    size_t counts[5] = {0, 0, 0, 0, 0};
};

namespace resolve_detail {

/* OsmEntityStorage as the reader has filled it after `seen` elements: add() inserts, so a later element of an id wins.
 * `seen` usually only grows from one owner to the next; where it does not, the map starts over. */
struct Storage {
    const uint64_t* ids;
    std::unordered_map<uint64_t, uint32_t> global_id_to_local_id;
    size_t added = 0;
    explicit Storage(const uint64_t* ids_) : ids(ids_) {}
    void read_up_to(size_t seen) {
        if (seen < added) global_id_to_local_id.clear(), added = 0;
        for (; added < seen; ++added) global_id_to_local_id[ids[added]] = (uint32_t)added;
    }
    bool translate_id(uint64_t g, uint32_t* out) const {
        const auto it = global_id_to_local_id.find(g);
        if (it == global_id_to_local_id.end()) return false;
        *out = it->second;
        return true;
    }
};

/* postprocess_node_refs, line for line */
inline std::vector<uint32_t> postprocess_node_refs(const std::vector<uint32_t>& refs) {
    if (refs.empty()) return refs;
    std::set<std::pair<uint32_t, uint32_t>> seen_node_pairs;
    std::vector<uint32_t> refs_without_duplicates{refs[0]};
    for (size_t idx = 1; idx < refs.size(); ++idx) {
        const uint32_t cur = refs[idx], prev = refs[idx - 1];
        if (!seen_node_pairs.count({cur, prev}) && !seen_node_pairs.count({prev, cur})) {
            seen_node_pairs.insert({cur, prev});
            refs_without_duplicates.push_back(cur);
        }
    }
    return refs_without_duplicates;
}

}  // namespace resolve_detail

/* The host twin of osmt_resolve_refs.  `d` is what osmt_validate_resolve accepts. */
inline ResolvedRefs resolve_refs_host(const osmt_raw_osm_desc& d) {
    ResolvedRefs out;
    resolve_detail::Storage nodes(d.node_ids), ways(d.way_ids);
    for (size_t w = 0; w < d.n_ways; ++w) {
        nodes.read_up_to(d.way_nodes_seen ? d.way_nodes_seen[w] : d.n_nodes);
        std::vector<uint32_t> refs;
        for (uint32_t r = d.way_ref_off[w]; r < d.way_ref_off[w + 1]; ++r) {
            uint32_t local;
            if (nodes.translate_id(d.way_refs[r], &local))
                refs.push_back(local);
            else
                ++out.counts[2];
        }
        const std::vector<uint32_t> kept = resolve_detail::postprocess_node_refs(refs);
        out.counts[3] += refs.size() - kept.size();
        out.way_nodes.insert(out.way_nodes.end(), kept.begin(), kept.end());
        out.way_node_off.push_back((uint32_t)out.way_nodes.size());
    }
    for (size_t r = 0; r < d.n_relations; ++r) {
        ways.read_up_to(d.relation_ways_seen ? d.relation_ways_seen[r] : d.n_ways);
        for (uint32_t m = d.relation_ref_off[r]; m < d.relation_ref_off[r + 1]; ++m) {
            uint32_t local;
            if (ways.translate_id(d.relation_refs[m], &local))
                out.relation_ways.push_back(local), out.relation_way_inner.push_back(d.relation_ref_inner[m]);
            else
                ++out.counts[4];
        }
        out.relation_way_off.push_back((uint32_t)out.relation_ways.size());
    }
    out.counts[0] = out.way_nodes.size(), out.counts[1] = out.relation_ways.size();
    return out;
}
inline ResolvedRefs resolve_refs_host(const RawOsmDesc& raw) { return resolve_refs_host(raw.view()); }

}  // namespace osmt

#endif /* OSMT_RESOLVE_HPP */
