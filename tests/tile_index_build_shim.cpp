// C entry points over host/osmt_tilequery.hpp for tests/_tileindexbuild.py (ctypes): osmt::tile_index_of, the host twin of
// osmt_build_tile_index, osmt::max_zoom_coordinate and osmt::mercator_factors.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

extern "C" {
// NULL: the twin threw (a factor outside [0, 1])
void* tib_new(const osmt_geodata_desc* g, const double* factors) {
    try {
        return new BuiltTileIndex(tile_index_of(*g, factors));
    } catch (const std::exception&) {
        return nullptr;
    }
}
void tib_free(void* h) { delete (BuiltTileIndex*)h; }
// which: 0 tile_xy, 1 way_off, 2 ways, 3 mp_off, 4 mps, 5 node_off, 6 nodes; returns the array's length (nothing is written beyond cap)
size_t tib_get(void* h, int which, uint32_t* out, size_t cap) {
    const BuiltTileIndex& v = *(const BuiltTileIndex*)h;
    const std::vector<uint32_t>* a[7] = {&v.tile_xy, &v.way_off, &v.ways, &v.mp_off, &v.mps, &v.node_off, &v.nodes};
    if (which < 0 || which >= 7) return 0;
    if (out && !a[which]->empty()) memcpy(out, a[which]->data(), (a[which]->size() < cap ? a[which]->size() : cap) * 4);
    return a[which]->size();
}
// 1: the build is refused for a factor of 1.0; *node, *axis (0: x, 1: y) name it
int tib_refused(void* h, size_t* node, int* axis) {
    const BuiltTileIndex& v = *(const BuiltTileIndex*)h;
    *node = v.refused_node, *axis = v.refused_axis;
    return v.refused ? 1 : 0;
}
// the z18 tile of every node of factors[n][2] into out[n][2]
void tib_node_tiles(const double* factors, size_t n, uint32_t* out) {
    for (size_t i = 0; i < 2 * n; ++i) out[i] = max_zoom_coordinate(factors[i]);
}
void tib_mercator_factors(const double* latlon, size_t n, double* out) {
    const std::vector<double> f = mercator_factors(latlon, n);
    if (n) memcpy(out, f.data(), 2 * n * sizeof(double));
}
}
