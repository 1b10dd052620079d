// A host program of its own over osmt::assemble_multipolygons_host (host/osmt_polygons.hpp): reads a world in the text form
// tests/_polygons.py writes (positions as the hex bits of lat and lon, the ways, the relations with their roles), builds it with
// osmt::RelationsDesc, assembles it and prints the counts and a checksum of the arrays.  tests/test_polygons_cpu.py builds it
// with -fsanitize=address,undefined and compares its output with the Python restatement.
// usage: polygons_host_main FILE
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_polygons.hpp"

template <class T>
static unsigned long long mix(unsigned long long h, const std::vector<T>& v) {
    for (T x : v) h = h * 1000003ull + (unsigned long long)x;
    return h * 1000003ull + v.size();
}

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    osmt::RelationsDesc rel;
    size_t n_nodes = 0, n_ways = 0, n_rels = 0;
    if (fscanf(f, "%zu", &n_nodes) != 1) return 2;
    for (size_t i = 0; i < n_nodes; ++i) {
        unsigned long long bits[2];
        double v[2];
        if (fscanf(f, "%llx %llx", &bits[0], &bits[1]) != 2) return 2;
        memcpy(v, bits, 16); /* any bit pattern: NaNs keep their payload */
        rel.nodes.push_back(0.0), rel.nodes.push_back(0.0);
        memcpy(&rel.nodes[2 * i], v, 16);
    }
    if (fscanf(f, "%zu", &n_ways) != 1) return 2;
    for (size_t i = 0; i < n_ways; ++i) {
        size_t k = 0;
        if (fscanf(f, "%zu", &k) != 1) return 2;
        std::vector<uint32_t> way(k);
        for (uint32_t& v : way)
            if (fscanf(f, "%u", &v) != 1) return 2;
        rel.add_way(way);
    }
    if (fscanf(f, "%zu", &n_rels) != 1) return 2;
    for (size_t i = 0; i < n_rels; ++i) {
        unsigned long long gid = 0;
        size_t k = 0;
        if (fscanf(f, "%llu %zu", &gid, &k) != 2) return 2;
        std::vector<std::pair<uint32_t, bool>> members(k);
        for (auto& m : members) {
            unsigned w = 0, inner = 0;
            if (fscanf(f, "%u %u", &w, &inner) != 2) return 2;
            m = {w, inner != 0};
        }
        rel.add_relation(gid, members);
    }
    fclose(f);
    try {
        const osmt::AssembledPolygons x = osmt::assemble_multipolygons_host(rel);
        std::vector<uint32_t> status;
        for (const osmt_relation_status& s : x.status) status.push_back(s.accepted), status.push_back(s.rings_built), status.push_back(s.unmatched);
        unsigned long long h = 0;
        h = mix(h, x.polygon_node_off), h = mix(h, x.polygon_nodes), h = mix(h, x.multipolygon_ids), h = mix(h, x.multipolygon_polygon_off);
        h = mix(h, x.multipolygon_polygons), h = mix(h, x.multipolygon_relation), h = mix(h, status);
        printf("polygons %zu %zu %zu %llu\n", x.polygon_node_off.size() - 1, x.polygon_nodes.size(), x.multipolygon_ids.size(), h);
        /* the helper writes the arrays into a GeodataDesc, whose desc then points at them */
        osmt::GeodataDesc g;
        g.nodes = rel.nodes;
        x.into(g);
        if (g.desc.n_polygons != x.polygon_node_off.size() - 1 || g.desc.n_polygon_nodes != x.polygon_nodes.size() || g.desc.n_multipolygons != x.multipolygon_ids.size() ||
            g.desc.n_multipolygon_polygons != x.multipolygon_polygons.size() || g.desc.n_nodes != n_nodes || g.desc.polygon_nodes != g.polygon_nodes.data())
            return 3;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
