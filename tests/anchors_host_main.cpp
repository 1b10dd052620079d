// Stand-alone host program over osmt::mercator_factors and osmt::label_rings_of (built with -fsanitize=address,undefined by
// tests/_anchors.py): a small geodata with an empty way, an empty polygon at the start of a multipolygon and a one-node polygon
// in the middle of another; every projected point is compared, bit for bit, with the reference's whole formula
// (tile.rs:88-106, labelable.rs:61-68) written out here with the same libm.  Prints "ok <points>" and exits 0.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_geodata.hpp"
#include "../osm_renderer_amd/host/osmt_labelable.hpp"

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

static void reference_point(double lat, double lon, uint8_t zoom, uint32_t tx, uint32_t ty, double scale, double* ox, double* oy) {
    const double PI = 3.14159265358979323846264338327950288;
    const double lat_rad = lat * (PI / 180.0), lon_rad = lon * (PI / 180.0);
    const double x = lon_rad + PI;
    const double y = PI - std::log(std::tan((PI / 4.0) + (lat_rad / 2.0)));
    const double dim = (double)(256u * (1u << zoom));
    const double px = (x / (2.0 * PI)) * dim, py = (y / (2.0 * PI)) * dim;
    const double rx = px - (double)(uint32_t)(tx * 256u), ry = py - (double)(uint32_t)(ty * 256u);
    *ox = rx * scale;
    *oy = ry * scale;
}

int main() {
    std::vector<double> nodes;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    const size_t n_nodes = 500;
    for (size_t i = 0; i < n_nodes; ++i) {
        nodes.push_back(-85.0 + 170.0 * rnd());
        nodes.push_back(-180.0 + 360.0 * rnd());
    }
    const std::vector<double> f = osmt::mercator_factors(nodes.data(), n_nodes);
    // ways: 0 nodes, 1, 2, 65, 300; polygons: empty, 5 nodes, 1 node, 70 nodes; multipolygons: {0, 1}, {1, 2, 3}, {}
    std::vector<uint32_t> way_off{0}, way_nodes, poly_off{0}, poly_nodes;
    uint32_t at = 0;
    for (uint32_t n : {0u, 1u, 2u, 65u, 300u}) {
        for (uint32_t i = 0; i < n; ++i) way_nodes.push_back(at++ % n_nodes);
        way_off.push_back((uint32_t)way_nodes.size());
    }
    for (uint32_t n : {0u, 5u, 1u, 70u}) {
        for (uint32_t i = 0; i < n; ++i) poly_nodes.push_back(at++ % n_nodes);
        poly_off.push_back((uint32_t)poly_nodes.size());
    }
    const std::vector<uint32_t> mp_off{0, 2, 5, 5}, mp_polys{0, 1, 1, 2, 3};
    const std::vector<uint64_t> way_ids{1, 2, 3, 4, 5}, mp_ids{7, 8, 9};
    osmt_geodata_desc g{};
    g.nodes = nodes.data(), g.n_nodes = n_nodes;
    g.way_ids = way_ids.data(), g.way_node_off = way_off.data(), g.n_ways = way_ids.size();
    g.way_nodes = way_nodes.data(), g.n_way_nodes = way_nodes.size();
    g.polygon_node_off = poly_off.data(), g.n_polygons = poly_off.size() - 1;
    g.polygon_nodes = poly_nodes.data(), g.n_polygon_nodes = poly_nodes.size();
    g.multipolygon_ids = mp_ids.data(), g.multipolygon_polygon_off = mp_off.data(), g.n_multipolygons = mp_ids.size();
    g.multipolygon_polygons = mp_polys.data(), g.n_multipolygon_polygons = mp_polys.size();

    struct tile {
        uint8_t z;
        uint32_t x, y;
    };
    const tile tiles[] = {{0, 0, 0}, {10, 512, 340}, {15, 19805, 10244}, {18, 0, 0}, {18, 262143, 262143}};
    size_t checked = 0;
    for (const tile& t : tiles)
        for (uint32_t scale = 1; scale <= OSMT_MAX_SCALE; scale *= 2) {
            osmt_query_tile q{};
            q.zoom = t.z, q.x = t.x, q.y = t.y;
            for (uint32_t e = 0; e < 8; ++e) {
                const bool mp = e >= 5;
                const uint32_t id = mp ? e - 5 : e;
                const auto rings = osmt::label_rings_of(g, f.data(), id | (mp ? OSMT_STYLED_MULTIPOLYGON : 0u), q, scale);
                const size_t want_rings = mp ? mp_off[id + 1] - mp_off[id] : 1;
                if (rings.size() != want_rings) return std::printf("entity %u: %zu rings, expected %zu\n", e, rings.size(), want_rings), 1;
                for (size_t k = 0; k < rings.size(); ++k) {
                    const uint32_t* src = mp ? poly_nodes.data() + poly_off[mp_polys[mp_off[id] + k]] : way_nodes.data() + way_off[id];
                    const size_t n = mp ? poly_off[mp_polys[mp_off[id] + k] + 1] - poly_off[mp_polys[mp_off[id] + k]] : way_off[id + 1] - way_off[id];
                    if (rings[k].size() != n) return std::printf("entity %u ring %zu: %zu points, expected %zu\n", e, k, rings[k].size(), n), 1;
                    for (size_t i = 0; i < n; ++i) {
                        double wx, wy;
                        reference_point(nodes[2 * src[i]], nodes[2 * src[i] + 1], t.z, t.x, t.y, (double)scale, &wx, &wy);
                        if (bits(wx) != bits(rings[k][i][0]) || bits(wy) != bits(rings[k][i][1]))
                            return std::printf("entity %u ring %zu point %zu: %a %a, expected %a %a\n", e, k, i, rings[k][i][0], rings[k][i][1], wx, wy), 1;
                        if (!(std::fabs(wx) <= 268435456.0) || !(std::fabs(wy) <= 268435456.0)) return std::printf("point beyond 2^28\n"), 1;
                        ++checked;
                    }
                }
                if (e < 3 || e == 5) (void)osmt::get_label_position(rings, (double)scale, true); /* the small ones: NONE, a point, a segment, a pentagon */
            }
            bool threw = false;
            try {
                (void)osmt::label_rings_of(g, f.data(), 5u, q, scale);
            } catch (const std::out_of_range&) {
                threw = true;
            }
            if (!threw) return std::printf("way 5 was accepted\n"), 1;
        }
    std::printf("ok %zu\n", checked);
    return 0;
}
