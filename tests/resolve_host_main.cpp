// A host program of its own over osmt::resolve_refs_host (host/osmt_resolve.hpp): reads a raw world in the text form
// tests/_resolve.py writes (the nodes' ids, the ways with their `seen` and node references, the relations with their `seen`,
// member ids and roles), builds it with osmt::RawOsmDesc, resolves it and prints the counts and a checksum of the arrays.
// tests/test_resolve_cpu.py builds it with -fsanitize=address,undefined and compares its output with the Python model.
// usage: resolve_host_main FILE
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_resolve.hpp"

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
    osmt::RawOsmDesc raw;
    size_t n_nodes = 0, n_ways = 0, n_rels = 0;
    int with_seen = 0;
    if (fscanf(f, "%d %zu", &with_seen, &n_nodes) != 2) return 2;
    /* the file lists the elements per kind; `seen` says where in the file each way and relation stood */
    std::vector<unsigned long long> node_ids(n_nodes);
    for (auto& g : node_ids)
        if (fscanf(f, "%llu", &g) != 1) return 2;
    for (unsigned long long g : node_ids) raw.add_node(g);
    if (fscanf(f, "%zu", &n_ways) != 1) return 2;
    for (size_t i = 0; i < n_ways; ++i) {
        unsigned long long gid = 0;
        unsigned seen = 0;
        size_t k = 0;
        if (fscanf(f, "%llu %u %zu", &gid, &seen, &k) != 3) return 2;
        std::vector<uint64_t> refs(k);
        for (uint64_t& v : refs) {
            unsigned long long g = 0;
            if (fscanf(f, "%llu", &g) != 1) return 2;
            v = g;
        }
        raw.add_way(gid, refs);
        raw.way_nodes_seen.push_back(seen);
    }
    if (fscanf(f, "%zu", &n_rels) != 1) return 2;
    for (size_t i = 0; i < n_rels; ++i) {
        unsigned seen = 0;
        size_t k = 0;
        if (fscanf(f, "%u %zu", &seen, &k) != 2) return 2;
        std::vector<std::pair<uint64_t, bool>> members(k);
        for (auto& m : members) {
            unsigned long long g = 0;
            unsigned inner = 0;
            if (fscanf(f, "%llu %u", &g, &inner) != 2) return 2;
            m = {g, inner != 0};
        }
        raw.add_relation(members);
        raw.relation_ways_seen.push_back(seen);
    }
    fclose(f);
    try {
        osmt_raw_osm_desc d = raw.view(); /* track_seen is off: the file's own values go in, or none */
        if (with_seen) d.way_nodes_seen = raw.way_nodes_seen.data(), d.relation_ways_seen = raw.relation_ways_seen.data();
        const osmt::ResolvedRefs x = osmt::resolve_refs_host(d);
        unsigned long long h = 0;
        h = mix(h, x.way_node_off), h = mix(h, x.way_nodes), h = mix(h, x.relation_way_off), h = mix(h, x.relation_ways), h = mix(h, x.relation_way_inner);
        printf("resolved %zu %zu %zu %zu %zu %llu\n", x.counts[0], x.counts[1], x.counts[2], x.counts[3], x.counts[4], h);
        if (x.way_node_off.size() != n_ways + 1 || x.relation_way_off.size() != n_rels + 1 || x.way_nodes.size() != x.counts[0]) return 3;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
