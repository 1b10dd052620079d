// osmt::TileLabelPositions (osm_renderer_amd/host/osmt_labelable.hpp) against libosmtile.so: a geodata file of three closed ways
// stated in degrees — a square, a 5000 x 0.01 pixel strip (its initial grid alone is 500 000 cells: the device declines it) and
// an L — registered with its Mercator factors, asked for under two tiles.  Prints, per request, the collector's answer and the
// host mirror's (uncapped, from the same factors) as hex bit patterns, and how many requests fell back to the CPU.
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

int main() {
    const uint32_t TX = 158455, TY = 81980; /* a z18 tile */
    const double PI = 3.14159265358979323846, dim = 256.0 * 262144.0;
    std::vector<double> nodes;
    std::vector<uint32_t> way_off{0}, way_nodes;
    auto way = [&](std::initializer_list<std::array<double, 2>> px) {
        for (const auto& p : px) {
            const double wx = TX * 256.0 + p[0], wy = TY * 256.0 + p[1];
            nodes.push_back(std::atan(std::sinh(PI * (1.0 - 2.0 * wy / dim))) * 180.0 / PI);
            nodes.push_back(wx / dim * 360.0 - 180.0);
            way_nodes.push_back((uint32_t)(nodes.size() / 2 - 1));
        }
        way_off.push_back((uint32_t)way_nodes.size());
    };
    way({{10.5, 20.25}, {50.5, 20.25}, {50.5, 60.25}, {10.5, 60.25}, {10.5, 20.25}});
    way({{0.0, 0.0}, {5000.0, 0.0}, {5000.0, 0.01}, {0.0, 0.01}, {0.0, 0.0}});
    way({{1.5, 2.5}, {81.5, 2.5}, {81.5, 32.25}, {31.75, 32.25}, {31.75, 92.5}, {1.5, 92.5}, {1.5, 2.5}});
    const std::vector<uint64_t> way_ids{1, 2, 3};
    const uint32_t zero = 0;
    osmt_geodata_desc g{};
    g.nodes = nodes.data(), g.n_nodes = nodes.size() / 2;
    g.way_ids = way_ids.data(), g.way_node_off = way_off.data(), g.n_ways = 3;
    g.way_nodes = way_nodes.data(), g.n_way_nodes = way_nodes.size();
    g.polygon_node_off = &zero, g.multipolygon_polygon_off = &zero;
    const std::vector<double> f = osmt::mercator_factors(nodes.data(), g.n_nodes);

    osmt_ctx* ctx = nullptr;
    if (osmt_create(nullptr, &ctx) != OSMT_OK) {
        std::fprintf(stderr, "osmt_create: %s\n", osmt_last_error());
        return 2;
    }
    uint32_t gid = 0;
    if (osmt_register_geodata(ctx, &g, &gid) != OSMT_OK || osmt_register_node_mercator(ctx, gid, f.data()) != OSMT_OK) {
        std::fprintf(stderr, "registration: %s\n", osmt_last_error());
        return 2;
    }
    const uint32_t scale = 2;
    osmt::TileLabelPositions lp(g, f.data(), gid, scale);
    const uint32_t t0 = lp.add_tile(18, TX, TY), t1 = lp.add_tile(15, TX >> 3, TY >> 3);
    struct rq {
        uint32_t way, tile;
    };
    const rq reqs[] = {{0, t0}, {1, t0}, {2, t1}, {1, t1}, {0, t1}};
    for (const rq& r : reqs) lp.add_way(r.way, r.tile);
    std::vector<osmt_label_position> got;
    try {
        got = lp.run(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (size_t i = 0; i < got.size(); ++i) {
        osmt_query_tile t{};
        t.zoom = reqs[i].tile == t0 ? 18 : 15;
        t.x = reqs[i].tile == t0 ? TX : TX >> 3, t.y = reqs[i].tile == t0 ? TY : TY >> 3;
        const osmt::LabelPosition want = osmt::get_label_position(osmt::label_rings_of(g, f.data(), reqs[i].way, t, scale), (double)scale);
        std::printf("%zu %u %016" PRIx64 " %016" PRIx64 " %u %016" PRIx64 " %016" PRIx64 "\n", i, got[i].status, bits(got[i].x), bits(got[i].y), want.status,
                    bits(want.x), bits(want.y));
    }
    std::printf("fallbacks %zu\n", lp.cpu_fallbacks());
    osmt_destroy(ctx);
    return 0;
}
