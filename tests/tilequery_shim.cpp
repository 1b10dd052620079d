// C entry points over host/osmt_tilequery.hpp for tests/_tilequery.py (ctypes): osmt::TileIndexDesc, osmt::StyleBindings and
// the host mirror osmt::styled_areas_of_tile.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

extern "C" {
void* tq_index_new(void* reader) { return new TileIndexDesc(*(const GeodataReader*)reader); }
const osmt_tile_index_desc* tq_index_get(void* d) { return &((TileIndexDesc*)d)->desc; }
void tq_index_free(void* d) { delete (TileIndexDesc*)d; }

// per entity the styles way_styles[way_off[i] .. way_off[i + 1]); entities with an empty range are skipped, as a caller would
void* tq_bindings_new(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_ways, const uint32_t* way_off, const uint32_t* way_styles,
                      size_t n_mps, const uint32_t* mp_off, const uint32_t* mp_styles) {
    StyleBindings* b = new StyleBindings(geodata_id, zoom_lo, zoom_hi, n_ways, n_mps);
    for (size_t i = 0; i < n_ways; ++i)
        if (way_off[i + 1] > way_off[i]) b->bind_way(i, std::vector<uint32_t>(way_styles + way_off[i], way_styles + way_off[i + 1]));
    for (size_t i = 0; i < n_mps; ++i)
        if (mp_off[i + 1] > mp_off[i]) b->bind_multipolygon(i, std::vector<uint32_t>(mp_styles + mp_off[i], mp_styles + mp_off[i + 1]));
    return b;
}
const osmt_style_bindings_desc* tq_bindings_get(void* b) { return &((StyleBindings*)b)->desc(); }
void tq_bindings_free(void* b) { delete (StyleBindings*)b; }

// the areas of one tile; returns their number (nothing is written beyond cap)
size_t tq_areas(void* reader, void* bindings, uint8_t zoom, uint32_t x, uint32_t y, osmt_styled_area* out, size_t cap) {
    const std::vector<osmt_styled_area> a = styled_areas_of_tile(*(const GeodataReader*)reader, *(const StyleBindings*)bindings, zoom, x, y);
    if (!a.empty()) memcpy(out, a.data(), (a.size() < cap ? a.size() : cap) * sizeof(osmt_styled_area));
    return a.size();
}

// the styled batch of n tiles (zxy: n x {zoom, x, y}): tiles[i].area_off / n_areas and the areas back to back; returns the
// number of areas (nothing is written beyond cap).  The per-tile host loop a server runs without osmt_scene_build_tiles.
size_t tq_batch(void* reader, void* bindings, const uint32_t* zxy, size_t n, osmt_styled_tile* tiles, osmt_styled_area* out, size_t cap) {
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const std::vector<osmt_styled_area> a =
            styled_areas_of_tile(*(const GeodataReader*)reader, *(const StyleBindings*)bindings, (uint8_t)zxy[3 * i], zxy[3 * i + 1], zxy[3 * i + 2]);
        tiles[i].area_off = (uint32_t)total;
        tiles[i].n_areas = (uint32_t)a.size();
        if (total + a.size() <= cap && !a.empty()) memcpy(out + total, a.data(), a.size() * sizeof(osmt_styled_area));
        total += a.size();
    }
    return total;
}

size_t tq_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_tile_index_desc);
        case 1: return sizeof(osmt_style_bindings_desc);
        case 2: return sizeof(osmt_query_tile);
        case 3: return sizeof(osmt_tile_batch);
        case 10: return offsetof(osmt_tile_index_desc, n_multipolygon_refs);
        case 11: return offsetof(osmt_style_bindings_desc, way_style_off);
        case 12: return offsetof(osmt_style_bindings_desc, n_multipolygon_styles);
        case 13: return offsetof(osmt_query_tile, canvas_rgb);
        case 14: return offsetof(osmt_tile_batch, bindings_of_zoom);
    }
    return 0;
}
}
