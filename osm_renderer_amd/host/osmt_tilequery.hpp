/*
 * osmt_tilequery.hpp — host side of scenes built from tile coordinates (include/osmtile.h, osmt_scene_build_tiles):
 *
 *   TileIndexDesc        the z18 tile storage of a geodata file (reader.rs:217-229) as osmt_register_tile_index takes it;
 *   StyleBindings        a CSR builder for osmt_register_style_bindings: per entity the style ids Styler::style_entities
 *                        pushes for it (styler.rs:128-160 memoises exactly this per (entity, zoom)), in push order;
 *   styled_areas_of_tile the host mirror of the device query: the (entity, style) pairs of one tile, written over
 *                        GeodataReader::get_entities_in_tile_with_neighbors (reader.rs:60-133) — it shares no code with the
 *                        kernels' rectangle arithmetic and is the yardstick of their tests.
 */
#ifndef OSMT_TILEQUERY_HPP
#define OSMT_TILEQUERY_HPP

#include <cstdint>
#include <stdexcept>
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

/* What osmt_scene_build_tiles derives for tile (zoom, x, y): every way of get_entities_in_tile_with_neighbors in ascending
 * local id, then every multipolygon (those without polygons are dropped there), each repeated once per bound style in
 * binding order.  An entity without a bound style contributes nothing.  osm_ids: the filter of
 * osmt_scene_build_tiles_filtered (nullptr: none), applied where the reference applies it: last, inside the query. */
inline std::vector<osmt_styled_area> styled_areas_of_tile(const GeodataReader& reader, const StyleBindings& bindings, uint8_t zoom, uint32_t x, uint32_t y,
                                                          const std::unordered_set<uint64_t>* osm_ids = nullptr) {
    const OsmEntityIds ids = reader.get_entities_in_tile_with_neighbors(zoom, x, y, osm_ids);
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
