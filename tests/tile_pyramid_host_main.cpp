// A host program of its own over host/osmt_tilequery.hpp: reads a geodata file, makes the levels named on the command line
// with osmt::tile_pyramid_level (node lists included) and prints, per level, its counts and a checksum of its arrays; then runs
// osmt::entities_of_tile with and without the pyramid over a list of tiles and prints, per tile, the three entity counts, a
// checksum and whether both forms agree.  tests/test_tile_pyramid_cpu.py builds it with -fsanitize=address,undefined and
// compares its output with the Python restatement.
// usage: tile_pyramid_host_main FILE N_LEVELS LEVEL ... [ZOOM X Y ...]
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

static unsigned long long mix(unsigned long long h, const std::vector<uint32_t>& v) {
    for (uint32_t x : v) h = h * 1000003ull + x;
    return h * 1000003ull + v.size();
}

int main(int argc, char** argv) {
    const int n_levels = argc > 2 ? atoi(argv[2]) : -1;
    if (n_levels < 0 || argc < 3 + n_levels || (argc - 3 - n_levels) % 3 != 0) {
        fprintf(stderr, "usage: %s FILE N_LEVELS LEVEL ... [ZOOM X Y ...]\n", argv[0]);
        return 2;
    }
    try {
        osmt::GeodataReader r(argv[1]);
        osmt::TileIndexDesc index(r);
        std::vector<uint32_t> node_off{0u}, nodes;
        for (size_t i = 0; i < r.tile_count(); ++i) {
            const auto ids = r.tile_node_ids(i);
            nodes.insert(nodes.end(), ids.first, ids.first + ids.second);
            node_off.push_back((uint32_t)nodes.size());
        }
        osmt::TilePyramid pyramid;
        for (int k = 0; k < n_levels; ++k) {
            const uint32_t level = (uint32_t)strtoul(argv[3 + k], nullptr, 10);
            const osmt::TilePyramidLevel& l = pyramid.levels[level] = osmt::tile_pyramid_level(index.desc, level, node_off.data(), nodes.data());
            unsigned long long h = 0;
            for (const std::vector<uint32_t>* a : {&l.tile_xy, &l.way_off, &l.ways, &l.mp_off, &l.mps, &l.node_off, &l.nodes}) h = mix(h, *a);
            printf("level %u %zu %zu %zu %zu %llu\n", level, l.tile_count(), l.ways.size(), l.mps.size(), l.nodes.size(), h);
        }
        for (int a = 3 + n_levels; a + 2 < argc; a += 3) {
            const uint8_t zoom = (uint8_t)atoi(argv[a]);
            const uint32_t x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
            const osmt::OsmEntityIds with = osmt::entities_of_tile(r, zoom, x, y, nullptr, &pyramid), without = osmt::entities_of_tile(r, zoom, x, y);
            const bool same = with.nodes == without.nodes && with.ways == without.ways && with.multipolygons == without.multipolygons;
            printf("%zu %zu %zu %llu %s\n", with.nodes.size(), with.ways.size(), with.multipolygons.size(), mix(mix(mix(0, with.nodes), with.ways), with.multipolygons),
                   same ? "same" : "DIFFERENT");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
