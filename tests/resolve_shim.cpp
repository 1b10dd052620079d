// C entry points over host/osmt_resolve.hpp for tests/_resolve.py (ctypes): osmt::resolve_refs_host, the host twin of
// osmt_resolve_refs.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_resolve.hpp"

using namespace osmt;

extern "C" {
// NULL: the twin threw
void* res_new(const osmt_raw_osm_desc* d) {
    try {
        return new ResolvedRefs(resolve_refs_host(*d));
    } catch (const std::exception&) {
        return nullptr;
    }
}
void res_free(void* h) { delete (ResolvedRefs*)h; }
// which: 0 way_node_off, 1 way_nodes, 2 relation_way_off, 3 relation_ways, 4 relation_way_inner (u8), 5 counts (five u64);
// returns the array's length in elements (nothing is written beyond cap)
size_t res_get(void* h, int which, void* out, size_t cap) {
    const ResolvedRefs& v = *(const ResolvedRefs*)h;
    unsigned long long counts[5];
    for (int i = 0; i < 5; ++i) counts[i] = v.counts[i];
    const void* p[6] = {v.way_node_off.data(), v.way_nodes.data(), v.relation_way_off.data(), v.relation_ways.data(), v.relation_way_inner.data(), counts};
    const size_t n[6] = {v.way_node_off.size(), v.way_nodes.size(), v.relation_way_off.size(), v.relation_ways.size(), v.relation_way_inner.size(), 5};
    const size_t sz[6] = {4, 4, 4, 4, 1, 8};
    if (which < 0 || which >= 6) return 0;
    if (out && n[which]) memcpy(out, p[which], (n[which] < cap ? n[which] : cap) * sz[which]);
    return n[which];
}
}
