// Host build of the tile-coordinate half of osm_renderer_amd/host/osmt_labelable.hpp (osmt::project_factors,
// osmt::label_rings_of) and of osmt::mercator_factors (host/osmt_geodata.hpp) for the CPU tests and as the yardstick of the
// GPU tests.  Compiled with -ffp-contract=off.
#include <cstring>

#include "../osm_renderer_amd/host/osmt_geodata.hpp"
#include "../osm_renderer_amd/host/osmt_labelable.hpp"

extern "C" {

void an_mercator_factors(const double* latlon, size_t n, double* out) {
    const std::vector<double> f = osmt::mercator_factors(latlon, n);
    if (n) std::memcpy(out, f.data(), f.size() * sizeof(double));
}

static osmt_query_tile tile_of(uint8_t zoom, uint32_t x, uint32_t y) {
    osmt_query_tile t{};
    t.x = x, t.y = y, t.zoom = zoom;
    return t;
}

// counts[0] = rings, counts[1] = points; ring_n[k] = points of ring k, pts = the rings' points one after the other.
// Returns 0, 1 when a capacity is too small (counts are set), 2 for an id the geodata does not have.
int an_label_rings(const osmt_geodata_desc* g, const double* factors, uint32_t entity, uint8_t zoom, uint32_t x, uint32_t y, uint32_t scale,
                   uint32_t* ring_n, size_t ring_cap, double* pts, size_t pts_cap, size_t* counts) {
    std::vector<osmt::LabelRing> rings;
    try {
        rings = osmt::label_rings_of(*g, factors, entity, tile_of(zoom, x, y), scale);
    } catch (const std::out_of_range&) {
        return 2;
    }
    size_t n = 0;
    for (const auto& r : rings) n += r.size();
    counts[0] = rings.size(), counts[1] = n;
    if (rings.size() > ring_cap || n > pts_cap) return 1;
    size_t at = 0;
    for (size_t k = 0; k < rings.size(); ++k) {
        ring_n[k] = (uint32_t)rings[k].size();
        for (const auto& p : rings[k]) {
            pts[2 * at] = p[0];
            pts[2 * at + 1] = p[1];
            ++at;
        }
    }
    return 0;
}

// get_label_position over label_rings_of: what osmt::TileLabelPositions computes for a request the device declines (capped = 0)
int an_position(const osmt_geodata_desc* g, const double* factors, uint32_t entity, uint8_t zoom, uint32_t x, uint32_t y, uint32_t scale, int capped,
                osmt_label_position* out) {
    try {
        const osmt::LabelPosition r = osmt::get_label_position(osmt::label_rings_of(*g, factors, entity, tile_of(zoom, x, y), scale), (double)scale, capped != 0);
        out->x = r.x, out->y = r.y, out->status = r.status, out->_pad = 0;
    } catch (const std::out_of_range&) {
        return 2;
    }
    return 0;
}

size_t an_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_label_tile_request);
        case 1: return sizeof(osmt_label_tile_batch);
        case 2: return sizeof(osmt_query_tile);
        default: return 0;
    }
}
}
