// C entry points over host/osmt_tilequery.hpp for tests/_tilepyramid.py (ctypes): osmt::tile_pyramid_level, the host twin of
// the device-built levels, and the mirror queries with a pyramid (osmt::TilePyramid, osmt::entities_of_tile,
// osmt::styled_areas_of_tile).  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

namespace {
size_t put(const std::vector<uint32_t>& v, uint32_t* out, size_t cap) {
    if (out && !v.empty()) memcpy(out, v.data(), (v.size() < cap ? v.size() : cap) * 4);
    return v.size();
}
std::unordered_set<uint64_t> set_of(const uint64_t* ids, size_t n) { return std::unordered_set<uint64_t>(ids, ids + n); }
}  // namespace

extern "C" {
// node_off == NULL: a level without node lists
void* tp_level_new(const osmt_tile_index_desc* index, uint32_t level, const uint32_t* node_off, const uint32_t* nodes) {
    return new TilePyramidLevel(tile_pyramid_level(*index, level, node_off, nodes));
}
void tp_level_free(void* l) { delete (TilePyramidLevel*)l; }
// which: 0 tile_xy, 1 way_off, 2 ways, 3 mp_off, 4 mps, 5 node_off, 6 nodes; returns the array's length (nothing is written beyond cap)
size_t tp_level_get(void* l, int which, uint32_t* out, size_t cap) {
    const TilePyramidLevel& v = *(const TilePyramidLevel*)l;
    const std::vector<uint32_t>* a[7] = {&v.tile_xy, &v.way_off, &v.ways, &v.mp_off, &v.mps, &v.node_off, &v.nodes};
    return which >= 0 && which < 7 ? put(*a[which], out, cap) : 0;
}

void* tp_pyramid_new() { return new TilePyramid(); }
void tp_pyramid_add(void* p, const osmt_tile_index_desc* index, uint32_t level, const uint32_t* node_off, const uint32_t* nodes) {
    ((TilePyramid*)p)->levels[level] = tile_pyramid_level(*index, level, node_off, nodes);
}
void tp_pyramid_free(void* p) { delete (TilePyramid*)p; }
// the level a tile of `zoom` reads, -1: none
int tp_pyramid_level_for(void* p, uint32_t zoom) {
    const TilePyramidLevel* l = ((const TilePyramid*)p)->level_for(zoom);
    return l ? (int)l->level : -1;
}

// kind: 0 nodes, 1 ways, 2 multipolygons of osmt::entities_of_tile; pyramid may be NULL; has_filter: ids[0 .. n_ids) is the osm_ids set
size_t tp_entities(void* reader, void* pyramid, uint8_t zoom, uint32_t x, uint32_t y, const uint64_t* ids, size_t n_ids, int has_filter, int kind, uint32_t* out,
                   size_t cap) {
    const std::unordered_set<uint64_t> s = set_of(ids, n_ids);
    const OsmEntityIds e = entities_of_tile(*(const GeodataReader*)reader, zoom, x, y, has_filter ? &s : nullptr, (const TilePyramid*)pyramid);
    return put(kind == 0 ? e.nodes : kind == 1 ? e.ways : e.multipolygons, out, cap);
}

// the areas of one tile through the pyramid; returns their number (nothing is written beyond cap)
size_t tp_areas(void* reader, void* bindings, void* pyramid, uint8_t zoom, uint32_t x, uint32_t y, const uint64_t* ids, size_t n_ids, int has_filter,
                osmt_styled_area* out, size_t cap) {
    const std::unordered_set<uint64_t> s = set_of(ids, n_ids);
    const std::vector<osmt_styled_area> a = styled_areas_of_tile(*(const GeodataReader*)reader, *(const StyleBindings*)bindings, zoom, x, y,
                                                                 has_filter ? &s : nullptr, (const TilePyramid*)pyramid);
    if (!a.empty()) memcpy(out, a.data(), (a.size() < cap ? a.size() : cap) * sizeof(osmt_styled_area));
    return a.size();
}
}
