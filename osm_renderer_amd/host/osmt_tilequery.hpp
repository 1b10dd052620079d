/*
 * osmt_tilequery.hpp — host side of scenes built from tile coordinates (include/osmtile.h, osmt_scene_build_tiles):
 *
 *   TileIndexDesc        the z18 tile storage of a geodata file (reader.rs:217-229) as osmt_register_tile_index takes it;
 *   StyleBindings        a CSR builder for osmt_register_style_bindings: per entity the style ids Styler::style_entities
 *                        pushes for it (styler.rs:128-160 memoises exactly this per (entity, zoom)), in push order;
 *   styled_areas_of_tile the host mirror of the device query: the (entity, style) pairs of one tile, written over
 *                        GeodataReader::get_entities_in_tile_with_neighbors (reader.rs:60-133) — it shares no code with the
 *                        kernels' rectangle arithmetic and is the yardstick of their tests;
 *   tile_pyramid_level   a level of the tile index pyramid (osmt_register_tile_pyramid) from its definition, a std::map of
 *                        std::sets; TilePyramid and entities_of_tile are the mirror query over such levels.
 */
#ifndef OSMT_TILEQUERY_HPP
#define OSMT_TILEQUERY_HPP

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_geodata.hpp"

namespace osmt {

/* `desc` points into the vectors: valid as long as this object lives and is not copied from. */
struct TileIndexDesc {
    std::vector<uint32_t> tile_xy, way_off{0u}, ways, multipolygon_off{0u}, multipolygons;
    osmt_tile_index_desc desc{};

    explicit TileIndexDesc(const GeodataReader& r) {
        auto append = [](std::vector<uint32_t>& off, std::vector<uint32_t>& flat, std::pair<const uint32_t*, size_t> ids) {
            flat.insert(flat.end(), ids.first, ids.first + ids.second);
            if (flat.size() >= 0xFFFFFFFFull) throw std::runtime_error("tile index too large for 32-bit offsets");
            off.push_back((uint32_t)flat.size());
        };
        for (size_t i = 0; i < r.tile_count(); ++i) {
            const auto xy = r.tile_xy(i);
            tile_xy.push_back(xy.first);
            tile_xy.push_back(xy.second);
            append(way_off, ways, r.tile_way_ids(i));
            append(multipolygon_off, multipolygons, r.tile_multipolygon_ids(i));
        }
        desc.tile_xy = tile_xy.data(), desc.n_tiles = tile_xy.size() / 2;
        desc.way_off = way_off.data(), desc.ways = ways.data(), desc.n_way_refs = ways.size();
        desc.multipolygon_off = multipolygon_off.data(), desc.multipolygons = multipolygons.data(), desc.n_multipolygon_refs = multipolygons.size();
    }
    TileIndexDesc(const TileIndexDesc&) = delete;
    TileIndexDesc& operator=(const TileIndexDesc&) = delete;
};

/* Entities are bound in ascending id, the ways first: bind_way(i, ...) for i = 0 .. n_ways - 1, each at most once (an
 * entity that is skipped has no style), then the multipolygons likewise; desc() closes both tables. */
class StyleBindings {
  public:
    StyleBindings(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_ways, size_t n_multipolygons)
        : n_ways_(n_ways), n_mps_(n_multipolygons) {
        desc_.geodata_id = geodata_id, desc_.zoom_lo = zoom_lo, desc_.zoom_hi = zoom_hi;
    }
    void bind_way(size_t way, const std::vector<uint32_t>& styles) { bind(way_off_, way_styles_, n_ways_, way, styles); }
    void bind_multipolygon(size_t mp, const std::vector<uint32_t>& styles) { bind(mp_off_, mp_styles_, n_mps_, mp, styles); }
    /* valid until the next bind_* call or the end of this object */
    const osmt_style_bindings_desc& desc() {
        way_off_.resize(n_ways_ + 1, (uint32_t)way_styles_.size());
        mp_off_.resize(n_mps_ + 1, (uint32_t)mp_styles_.size());
        desc_.way_style_off = way_off_.data(), desc_.way_styles = way_styles_.data(), desc_.n_way_styles = way_styles_.size();
        desc_.multipolygon_style_off = mp_off_.data(), desc_.multipolygon_styles = mp_styles_.data(), desc_.n_multipolygon_styles = mp_styles_.size();
        return desc_;
    }
    /* the styles of an entity, as (first, count) into the pool */
    std::pair<const uint32_t*, size_t> way(size_t i) const { return of(way_off_, way_styles_, i); }
    std::pair<const uint32_t*, size_t> multipolygon(size_t i) const { return of(mp_off_, mp_styles_, i); }

  private:
    static void bind(std::vector<uint32_t>& off, std::vector<uint32_t>& pool, size_t n, size_t id, const std::vector<uint32_t>& styles) {
        if (id >= n) throw std::out_of_range("StyleBindings: entity id out of range");
        if (off.size() > id + 1) throw std::logic_error("StyleBindings: entities are bound in ascending id, each once");
        off.resize(id + 1, (uint32_t)pool.size()); /* the entities skipped since the last call have no style */
        pool.insert(pool.end(), styles.begin(), styles.end());
        if (pool.size() >= 0xFFFFFFFFull) throw std::runtime_error("StyleBindings: too many styles for 32-bit offsets");
        off.push_back((uint32_t)pool.size());
    }
    static std::pair<const uint32_t*, size_t> of(const std::vector<uint32_t>& off, const std::vector<uint32_t>& pool, size_t i) {
        if (i + 1 >= off.size()) return {nullptr, 0}; /* behind the last bound entity */
        return {pool.data() + off[i], off[i + 1] - off[i]};
    }
    size_t n_ways_, n_mps_;
    std::vector<uint32_t> way_off_{0u}, way_styles_, mp_off_{0u}, mp_styles_;
    osmt_style_bindings_desc desc_{};
};

/* One level of a tile index pyramid (osmt_register_tile_pyramid), in the layout osmt_read_tile_pyramid copies back. */
struct TilePyramidLevel {
    uint32_t level = 0;
    bool has_nodes = false;
    std::vector<uint32_t> tile_xy, way_off{0u}, ways, mp_off{0u}, mps, node_off{0u}, nodes;
    size_t tile_count() const { return tile_xy.size() / 2; }
};

/* Level `level` of `index` from its definition: the tiles are the distinct (x >> s, y >> s), s = 18 - level, over ALL tiles of
 * the index (a tile with empty lists still gives its parent a tile), ascending by (x, y); per tile and kind the union of its
 * z18 children's lists, ascending and without repeats.  node_off / nodes: the node lists of the index's tiles
 * (osmt_node_index_desc), nullptr: a level without node lists.  The yardstick of the device build. */
inline TilePyramidLevel tile_pyramid_level(const osmt_tile_index_desc& index, uint32_t level, const uint32_t* node_off = nullptr,
                                           const uint32_t* nodes = nullptr) {
    if (level > OSMT_MAX_ZOOM) throw std::out_of_range("tile_pyramid_level: level above 18");
    const uint32_t s = OSMT_MAX_ZOOM - level;
    struct Lists {
        std::set<uint32_t> kind[3];
    };
    std::map<std::pair<uint32_t, uint32_t>, Lists> tiles;
    for (size_t i = 0; i < index.n_tiles; ++i) {
        Lists& t = tiles[{index.tile_xy[2 * i] >> s, index.tile_xy[2 * i + 1] >> s}];
        t.kind[0].insert(index.ways + index.way_off[i], index.ways + index.way_off[i + 1]);
        t.kind[1].insert(index.multipolygons + index.multipolygon_off[i], index.multipolygons + index.multipolygon_off[i + 1]);
        if (node_off) t.kind[2].insert(nodes + node_off[i], nodes + node_off[i + 1]);
    }
    TilePyramidLevel out;
    out.level = level, out.has_nodes = node_off != nullptr;
    for (const auto& kv : tiles) {
        out.tile_xy.push_back(kv.first.first);
        out.tile_xy.push_back(kv.first.second);
        out.ways.insert(out.ways.end(), kv.second.kind[0].begin(), kv.second.kind[0].end());
        out.mps.insert(out.mps.end(), kv.second.kind[1].begin(), kv.second.kind[1].end());
        out.nodes.insert(out.nodes.end(), kv.second.kind[2].begin(), kv.second.kind[2].end());
        out.way_off.push_back((uint32_t)out.ways.size());
        out.mp_off.push_back((uint32_t)out.mps.size());
        out.node_off.push_back((uint32_t)out.nodes.size());
    }
    return out;
}

/* The z18 tile index of a geodata file from its definition (get_tile_references, saver.rs:167-226, with max_zoom_tile of
 * tile.rs:30-38 over the registered Mercator factors): the host twin and yardstick of osmt_build_tile_index.  The vectors are
 * what an osmt_tile_index_desc and an osmt_node_index_desc point to (index_desc, node_desc: valid as long as this object lives
 * and is not copied from; node_desc.node_ids is the caller's). */
struct BuiltTileIndex {
    std::vector<uint32_t> tile_xy, way_off{0u}, ways, mp_off{0u}, mps, node_off{0u}, nodes;
    /* a factor of exactly 1.0 (coordinate 2^18): the build is refused and the arrays are empty */
    bool refused = false;
    size_t refused_node = 0;
    int refused_axis = 0; /* 0: x, 1: y */
    size_t tile_count() const { return tile_xy.size() / 2; }
    osmt_tile_index_desc index_desc() const {
        osmt_tile_index_desc d{};
        d.tile_xy = tile_xy.data(), d.n_tiles = tile_count();
        d.way_off = way_off.data(), d.ways = ways.data(), d.n_way_refs = ways.size();
        d.multipolygon_off = mp_off.data(), d.multipolygons = mps.data(), d.n_multipolygon_refs = mps.size();
        return d;
    }
    osmt_node_index_desc node_desc(const uint64_t* node_ids, size_t n_nodes) const {
        osmt_node_index_desc d{};
        d.node_ids = node_ids, d.n_nodes = n_nodes;
        d.node_off = node_off.data(), d.nodes = nodes.data(), d.n_node_refs = nodes.size();
        return d;
    }
};

/* the z18 tile coordinate of a Mercator factor in [0, 1]: (u32)(f * 2^26) / 256 — the product is exact, the conversion truncates */
inline uint32_t max_zoom_coordinate(double factor) {
    if (!(factor >= 0.0) || !(factor <= 1.0)) throw std::out_of_range("max_zoom_coordinate: factor is not finite or outside [0, 1]"); /* what osmt_register_node_mercator refuses */
    return (uint32_t)(factor * 67108864.0) >> 8;
}

/* factors: [n_nodes][2] as osmt_register_node_mercator takes them (osmt::mercator_factors) */
inline BuiltTileIndex tile_index_of(const osmt_geodata_desc& g, const double* factors) {
    BuiltTileIndex out;
    const uint32_t world = 1u << OSMT_MAX_ZOOM;
    std::vector<std::pair<uint32_t, uint32_t>> tile(g.n_nodes);
    for (size_t i = 0; i < g.n_nodes; ++i) {
        tile[i] = {max_zoom_coordinate(factors[2 * i]), max_zoom_coordinate(factors[2 * i + 1])};
        if (tile[i].first >= world || tile[i].second >= world) {
            out.refused = true, out.refused_node = i, out.refused_axis = tile[i].first >= world ? 0 : 1;
            return out;
        }
    }
    struct Lists {
        std::set<uint32_t> kind[3]; /* ways, multipolygons, nodes */
    };
    std::map<std::pair<uint32_t, uint32_t>, Lists> tiles;
    for (size_t i = 0; i < g.n_nodes; ++i) tiles[tile[i]].kind[2].insert((uint32_t)i);
    struct Box {
        uint32_t x0 = ~0u, x1 = 0u, y0 = ~0u, y1 = 0u;
        bool any = false;
        void add(const std::pair<uint32_t, uint32_t>& t) {
            x0 = std::min(x0, t.first), x1 = std::max(x1, t.first), y0 = std::min(y0, t.second), y1 = std::max(y1, t.second), any = true;
        }
    };
    auto spread = [&](const Box& b, int kind, uint32_t id) {
        if (!b.any) return;
        for (uint32_t x = b.x0; x <= b.x1; ++x)
            for (uint32_t y = b.y0; y <= b.y1; ++y) tiles[{x, y}].kind[kind].insert(id);
    };
    for (size_t w = 0; w < g.n_ways; ++w) {
        Box b;
        for (uint32_t k = g.way_node_off[w]; k < g.way_node_off[w + 1]; ++k) b.add(tile[g.way_nodes[k]]);
        spread(b, 0, (uint32_t)w);
    }
    for (size_t m = 0; m < g.n_multipolygons; ++m) {
        Box b;
        for (uint32_t k = g.multipolygon_polygon_off[m]; k < g.multipolygon_polygon_off[m + 1]; ++k) {
            const uint32_t p = g.multipolygon_polygons[k];
            for (uint32_t q = g.polygon_node_off[p]; q < g.polygon_node_off[p + 1]; ++q) b.add(tile[g.polygon_nodes[q]]);
        }
        spread(b, 1, (uint32_t)m);
    }
    for (const auto& kv : tiles) {
        out.tile_xy.push_back(kv.first.first);
        out.tile_xy.push_back(kv.first.second);
        out.ways.insert(out.ways.end(), kv.second.kind[0].begin(), kv.second.kind[0].end());
        out.mps.insert(out.mps.end(), kv.second.kind[1].begin(), kv.second.kind[1].end());
        out.nodes.insert(out.nodes.end(), kv.second.kind[2].begin(), kv.second.kind[2].end());
        if (out.ways.size() >= 0xFFFFFFFFull || out.mps.size() >= 0xFFFFFFFFull) throw std::runtime_error("tile_index_of: too large for 32-bit offsets");
        out.way_off.push_back((uint32_t)out.ways.size());
        out.mp_off.push_back((uint32_t)out.mps.size());
        out.node_off.push_back((uint32_t)out.nodes.size());
    }
    return out;
}

inline BuiltTileIndex tile_index_of(const GeodataDesc& g, const double* factors) { return tile_index_of(g.desc, factors); }

/* The registered levels of one geodata file, by level. */
struct TilePyramid {
    std::map<uint32_t, TilePyramidLevel> levels;
    /* the level a tile of `zoom` reads: the smallest registered one >= zoom; nullptr: none, the z18 index */
    const TilePyramidLevel* level_for(uint32_t zoom) const {
        const auto it = levels.lower_bound(zoom);
        return it == levels.end() ? nullptr : &it->second;
    }
};

/* get_entities_in_tile_with_neighbors as the device runs it with a pyramid: ways and multipolygons gathered from the level the
 * tile reads, nodes too where that level has node lists (else from the z18 index), then the reference's sort, dedup, drop of
 * multipolygons without polygons and id filter.  A level's tile belongs to the neighbourhood iff its ancestor at `zoom` is one
 * of the 3 x 3 tiles around (x, y).  pyramid == nullptr, or no level >= zoom: the reader's own walk. */
inline OsmEntityIds entities_of_tile(const GeodataReader& reader, uint8_t zoom, uint32_t x, uint32_t y, const std::unordered_set<uint64_t>* osm_ids = nullptr,
                                     const TilePyramid* pyramid = nullptr) {
    const TilePyramidLevel* lv = pyramid ? pyramid->level_for(zoom) : nullptr;
    if (!lv) return reader.get_entities_in_tile_with_neighbors(zoom, x, y, osm_ids);
    OsmEntityIds ids;
    const uint32_t sh = lv->level - zoom;
    for (size_t i = 0; i < lv->tile_count(); ++i) {
        const int64_t ax = lv->tile_xy[2 * i] >> sh, ay = lv->tile_xy[2 * i + 1] >> sh;
        if (ax < (int64_t)x - 1 || ax > (int64_t)x + 1 || ay < (int64_t)y - 1 || ay > (int64_t)y + 1) continue;
        ids.ways.insert(ids.ways.end(), lv->ways.begin() + lv->way_off[i], lv->ways.begin() + lv->way_off[i + 1]);
        ids.multipolygons.insert(ids.multipolygons.end(), lv->mps.begin() + lv->mp_off[i], lv->mps.begin() + lv->mp_off[i + 1]);
        if (lv->has_nodes) ids.nodes.insert(ids.nodes.end(), lv->nodes.begin() + lv->node_off[i], lv->nodes.begin() + lv->node_off[i + 1]);
    }
    auto uniq = [](std::vector<uint32_t>& v) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    };
    uniq(ids.ways), uniq(ids.multipolygons), uniq(ids.nodes);
    ids.multipolygons.erase(std::remove_if(ids.multipolygons.begin(), ids.multipolygons.end(),
                                           [&](uint32_t m) { return reader.multipolygon_polygon_ids(m).second == 0; }),
                            ids.multipolygons.end());
    if (osm_ids) {
        auto keep = [&](std::vector<uint32_t>& v, auto global_id) {
            v.erase(std::remove_if(v.begin(), v.end(), [&](uint32_t e) { return osm_ids->count(global_id(e)) == 0; }), v.end());
        };
        keep(ids.nodes, [&](uint32_t e) { return reader.node_global_id(e); });
        keep(ids.ways, [&](uint32_t e) { return reader.way_global_id(e); });
        keep(ids.multipolygons, [&](uint32_t e) { return reader.multipolygon_global_id(e); });
    }
    if (!lv->has_nodes) ids.nodes = reader.get_entities_in_tile_with_neighbors(zoom, x, y, osm_ids).nodes;
    return ids;
}

/* What osmt_scene_build_tiles derives for tile (zoom, x, y): every way of get_entities_in_tile_with_neighbors in ascending
 * local id, then every multipolygon (those without polygons are dropped there), each repeated once per bound style in
 * binding order.  An entity without a bound style contributes nothing.  osm_ids: the filter of
 * osmt_scene_build_tiles_filtered (nullptr: none), applied where the reference applies it: last, inside the query.
 * pyramid: the levels registered for the file (nullptr: none) — the result does not depend on it. */
inline std::vector<osmt_styled_area> styled_areas_of_tile(const GeodataReader& reader, const StyleBindings& bindings, uint8_t zoom, uint32_t x, uint32_t y,
                                                          const std::unordered_set<uint64_t>* osm_ids = nullptr, const TilePyramid* pyramid = nullptr) {
    const OsmEntityIds ids = entities_of_tile(reader, zoom, x, y, osm_ids, pyramid);
    std::vector<osmt_styled_area> out;
    for (uint32_t w : ids.ways) {
        const auto st = bindings.way(w);
        for (size_t k = 0; k < st.second; ++k) out.push_back(osmt_styled_area{w, st.first[k]});
    }
    for (uint32_t m : ids.multipolygons) {
        const auto st = bindings.multipolygon(m);
        for (size_t k = 0; k < st.second; ++k) out.push_back(osmt_styled_area{m | OSMT_STYLED_MULTIPOLYGON, st.first[k]});
    }
    return out;
}

}  // namespace osmt
#endif
