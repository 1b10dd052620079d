/*
 * osmt_polygons.hpp — multipolygon rings from relations' member ways on the host: osmt::RelationsDesc builds the arrays
 * osmt_assemble_multipolygons takes, osmt::assemble_multipolygons_host is the host twin of that call — a plain restatement of
 * find_polygons_in_multipolygon (find_polygons.rs) over RawRelation::to_segments (importer.rs:516-537), with maps and sets as
 * the importer has them — and the yardstick of the GPU tests.  Host only: no HIP, no device.
 */
#ifndef OSMT_POLYGONS_HPP
#define OSMT_POLYGONS_HPP

#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_geodata.hpp"

namespace osmt {

/* The arrays of an osmt_relations_desc with owning vectors.  view() points into them: valid until the next add_*. */
struct RelationsDesc {
    std::vector<double> nodes;
    std::vector<uint32_t> way_node_off{0u}, way_nodes, relation_way_off{0u}, relation_ways;
    std::vector<uint64_t> relation_ids;
    std::vector<uint8_t> relation_way_inner;

    uint32_t add_node(double lat, double lon) {
        nodes.push_back(lat), nodes.push_back(lon);
        return (uint32_t)(nodes.size() / 2 - 1);
    }
    uint32_t add_way(const std::vector<uint32_t>& node_indices) {
        way_nodes.insert(way_nodes.end(), node_indices.begin(), node_indices.end());
        if (way_nodes.size() >= 0xFFFFFFFFull) throw std::runtime_error("relations too large for 32-bit offsets");
        way_node_off.push_back((uint32_t)way_nodes.size());
        return (uint32_t)(way_node_off.size() - 2);
    }
    /* members: (way index, is_inner) in the relation's order */
    void add_relation(uint64_t global_id, const std::vector<std::pair<uint32_t, bool>>& members) {
        relation_ids.push_back(global_id);
        for (const auto& m : members) relation_ways.push_back(m.first), relation_way_inner.push_back(m.second ? 1u : 0u);
        if (relation_ways.size() >= 0xFFFFFFFFull) throw std::runtime_error("relations too large for 32-bit offsets");
        relation_way_off.push_back((uint32_t)relation_ways.size());
    }
    osmt_relations_desc view() const {
        osmt_relations_desc d{};
        d.nodes = nodes.data(), d.n_nodes = nodes.size() / 2;
        d.way_node_off = way_node_off.data(), d.n_ways = way_node_off.size() - 1, d.way_nodes = way_nodes.data(), d.n_way_nodes = way_nodes.size();
        d.relation_ids = relation_ids.data(), d.relation_way_off = relation_way_off.data(), d.n_relations = relation_ids.size();
        d.relation_ways = relation_ways.data(), d.relation_way_inner = relation_way_inner.data(), d.n_relation_ways = relation_ways.size();
        return d;
    }
};

/* What an assembly gives: the polygon and multipolygon arrays of osmt_geodata_desc, every relation's status, and the relation
 * of every multipolygon. */
struct AssembledPolygons {
    std::vector<uint32_t> polygon_node_off{0u}, polygon_nodes, multipolygon_polygon_off{0u}, multipolygon_polygons, multipolygon_relation;
    std::vector<uint64_t> multipolygon_ids;
    std::vector<osmt_relation_status> status;

    /* the arrays into a GeodataDesc, whose nodes and ways stay as they are */
    void into(GeodataDesc& g) const {
        g.polygon_node_off = polygon_node_off, g.polygon_nodes = polygon_nodes;
        g.multipolygon_ids = multipolygon_ids, g.multipolygon_polygon_off = multipolygon_polygon_off, g.multipolygon_polygons = multipolygon_polygons;
        g.repoint();
    }
};

/* The host twin of osmt_assemble_multipolygons.  `d` is what osmt_validate_relations accepts; an index out of range throws. */
inline AssembledPolygons assemble_multipolygons_host(const osmt_relations_desc& d) {
    typedef std::pair<uint64_t, uint64_t> Pos;
    struct Node {
        size_t id;
        Pos pos;
    };
    struct Segment {
        Node node1, node2;
        bool is_inner;
    };
    struct Connected {
        Pos other_side;
        size_t segment_index;
        bool is_inner;
    };
    auto node_of = [&](uint32_t i) {
        if (i >= d.n_nodes) throw std::out_of_range("assemble_multipolygons_host: a node index out of range");
        Node n;
        n.id = i;
        std::memcpy(&n.pos.first, &d.nodes[2 * (size_t)i], 8); /* f64::to_bits */
        std::memcpy(&n.pos.second, &d.nodes[2 * (size_t)i + 1], 8);
        return n;
    };
    AssembledPolygons out;
    for (size_t r = 0; r < d.n_relations; ++r) {
        /* 1: RawRelation::to_segments */
        std::vector<Segment> segments;
        for (uint32_t j = d.relation_way_off[r]; j < d.relation_way_off[r + 1]; ++j) {
            const uint32_t w = d.relation_ways[j];
            if (w >= d.n_ways) throw std::out_of_range("assemble_multipolygons_host: a way index out of range");
            for (uint32_t k = d.way_node_off[w] + 1; k < d.way_node_off[w + 1]; ++k)
                segments.push_back(Segment{node_of(d.way_nodes[k - 1]), node_of(d.way_nodes[k]), d.relation_way_inner[j] != 0});
        }
        /* 2: get_connections */
        std::map<Pos, std::vector<Connected>> connections;
        for (size_t idx = 0; idx < segments.size(); ++idx) {
            const Segment& s = segments[idx];
            connections[s.node1.pos].push_back(Connected{s.node2.pos, idx, s.is_inner});
            connections[s.node2.pos].push_back(Connected{s.node1.pos, idx, s.is_inner});
        }
        /* 3: find_rings */
        std::vector<bool> available(segments.size(), true);
        std::vector<std::vector<size_t>> rings;
        size_t unmatched = segments.size();
        bool accepted = true;
        for (size_t start = 0; start < segments.size() && accepted; ++start) {
            if (!available[start]) continue;
            available[start] = false;
            std::vector<size_t> used{start};
            std::set<Pos> used_vertices{segments[start].node1.pos, segments[start].node2.pos};
            const Pos first = segments[start].node1.pos;
            const bool is_inner = segments[start].is_inner;
            Pos at = segments[start].node2.pos;
            bool found_ring = false;
            for (;;) { /* find_ring_from */
                const Connected* next = nullptr;
                const auto list = connections.find(at);
                if (list != connections.end())
                    for (const Connected& c : list->second) { /* find_next_segment */
                        const bool can_use = c.is_inner == is_inner && available[c.segment_index];
                        const bool is_duplicate = used_vertices.count(c.other_side) && c.other_side != first;
                        if (can_use && !is_duplicate) {
                            next = &c;
                            break;
                        }
                    }
                if (!next) break;
                available[next->segment_index] = false;
                used.push_back(next->segment_index);
                used_vertices.insert(next->other_side);
                if (next->other_side == first) {
                    found_ring = used.size() >= 3;
                    break;
                }
                at = next->other_side;
            }
            if (!found_ring) {
                accepted = false;
                break;
            }
            unmatched -= used.size();
            rings.push_back(used);
        }
        osmt_relation_status st;
        st.accepted = accepted ? 1u : 0u, st.rings_built = (uint32_t)rings.size(), st.unmatched = (uint32_t)unmatched;
        out.status.push_back(st);
        if (!accepted) continue;
        /* 4, 5: the polygons, appended to the storage; one multipolygon */
        for (const std::vector<size_t>& ring : rings) {
            std::vector<size_t> polygon;
            for (size_t idx = 0; idx < ring.size(); ++idx) {
                const Segment& s = segments[ring[idx]];
                if (idx == 0) polygon.push_back(s.node1.id);
                const size_t last = polygon.back();
                polygon.push_back(last == s.node1.id ? s.node2.id : s.node1.id);
            }
            out.multipolygon_polygons.push_back((uint32_t)(out.polygon_node_off.size() - 1));
            for (size_t id : polygon) out.polygon_nodes.push_back((uint32_t)id);
            out.polygon_node_off.push_back((uint32_t)out.polygon_nodes.size());
        }
        out.multipolygon_ids.push_back(d.relation_ids[r]);
        out.multipolygon_relation.push_back((uint32_t)r);
        out.multipolygon_polygon_off.push_back((uint32_t)out.multipolygon_polygons.size());
    }
    return out;
}

inline AssembledPolygons assemble_multipolygons_host(const RelationsDesc& r) { return assemble_multipolygons_host(r.view()); }

}  // namespace osmt

#endif /* OSMT_POLYGONS_HPP */
