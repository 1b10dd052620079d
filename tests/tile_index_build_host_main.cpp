// A host program of its own over osmt::tile_index_of (host/osmt_tilequery.hpp): reads a world in the text form
// tests/_tileindexbuild.py writes (counts, factors as hex floats, the three reference lists), builds its z18 tile index and
// prints the counts and a checksum of its arrays, or the refusal.  tests/test_tile_index_build_cpu.py builds it with
// -fsanitize=address,undefined and compares its output with the Python restatement.
// usage: tile_index_build_host_main FILE
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

static unsigned long long mix(unsigned long long h, const std::vector<uint32_t>& v) {
    for (uint32_t x : v) h = h * 1000003ull + x;
    return h * 1000003ull + v.size();
}

static bool read_list(FILE* f, std::vector<uint32_t>& off, std::vector<uint32_t>& flat) {
    size_t n = 0;
    if (fscanf(f, "%zu", &n) != 1) return false;
    off.assign(1, 0u);
    for (size_t i = 0; i < n; ++i) {
        size_t k = 0;
        if (fscanf(f, "%zu", &k) != 1) return false;
        for (size_t j = 0; j < k; ++j) {
            unsigned v = 0;
            if (fscanf(f, "%u", &v) != 1) return false;
            flat.push_back(v);
        }
        off.push_back((uint32_t)flat.size());
    }
    return true;
}

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    size_t n_nodes = 0;
    if (fscanf(f, "%zu", &n_nodes) != 1) return 2;
    std::vector<double> factors(2 * n_nodes), nodes(2 * n_nodes, 0.0);
    for (double& v : factors) {
        char word[64];
        if (fscanf(f, "%63s", word) != 1) return 2;
        v = strtod(word, nullptr); /* hex floats: exact */
    }
    std::vector<uint32_t> way_off, way_nodes, poly_off, poly_nodes, mp_off, mp_polys;
    if (!read_list(f, way_off, way_nodes) || !read_list(f, poly_off, poly_nodes) || !read_list(f, mp_off, mp_polys)) return 2;
    fclose(f);
    std::vector<uint64_t> way_ids(way_off.size() - 1, 0), mp_ids(mp_off.size() - 1, 0);
    osmt_geodata_desc g{};
    g.nodes = nodes.data(), g.n_nodes = n_nodes;
    g.way_ids = way_ids.data(), g.way_node_off = way_off.data(), g.n_ways = way_ids.size(), g.way_nodes = way_nodes.data(), g.n_way_nodes = way_nodes.size();
    g.polygon_node_off = poly_off.data(), g.n_polygons = poly_off.size() - 1, g.polygon_nodes = poly_nodes.data(), g.n_polygon_nodes = poly_nodes.size();
    g.multipolygon_ids = mp_ids.data(), g.multipolygon_polygon_off = mp_off.data(), g.n_multipolygons = mp_ids.size();
    g.multipolygon_polygons = mp_polys.data(), g.n_multipolygon_polygons = mp_polys.size();
    try {
        const osmt::BuiltTileIndex x = osmt::tile_index_of(g, factors.data());
        if (x.refused) {
            printf("refused %zu %c\n", x.refused_node, x.refused_axis ? 'y' : 'x');
            return 0;
        }
        unsigned long long h = 0;
        for (const std::vector<uint32_t>* a : {&x.tile_xy, &x.way_off, &x.ways, &x.mp_off, &x.mps, &x.node_off, &x.nodes}) h = mix(h, *a);
        printf("index %zu %zu %zu %zu %llu\n", x.tile_count(), x.ways.size(), x.mps.size(), x.nodes.size(), h);
        /* the descs point at the arrays */
        const osmt_tile_index_desc d = x.index_desc();
        const osmt_node_index_desc nd = x.node_desc(nullptr, n_nodes);
        if (d.n_tiles != x.tile_count() || d.n_way_refs != x.ways.size() || nd.n_node_refs != x.nodes.size() || nd.n_nodes != n_nodes) return 3;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
