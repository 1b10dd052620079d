// Stand-alone host program over the osm_ids filter of the host twins, built with -fsanitize=address,undefined by
// tests/_idfilter.py and run directly by tests/test_idfilter_cpu.py:
//   idfilter_host_main <geodata file> <scale> <n ids, or -1 for no filter> <id>... {<zoom> <x> <y>}...
// The ids go through osmt::id_filter_set (the sort and dedup of a registration) and osmt::id_filter_plane (the host twin of
// the kernel) over the file's ways, multipolygons and nodes; then osmt::styled_areas_of_tile, osmt::node_labels_of_tile and
// osmt::area_labels_of_tile run over every tile with the ids AS GIVEN (any order, repeats) as their osm_ids.  The binding
// rules are those of tests/tilequery_host_main.cpp, tests/tilelabels_host_main.cpp and tests/arealabels_host_main.cpp.
#include <cstdio>
#include <cstdlib>
#include <unordered_set>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"
#include "../osm_renderer_amd/host/osmt_idfilter.hpp"
#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

static void print_plane(const char* name, const std::vector<uint64_t>& gids, const std::vector<uint64_t>& set) {
    const std::vector<uint32_t> p = id_filter_plane(gids.data(), gids.size(), set);
    printf("plane %s %zu", name, p.size());
    for (uint32_t w : p) printf(" %08x", w);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const GeodataReader r(argv[1]);
    const uint32_t scale = (uint32_t)atoi(argv[2]);
    const long n_ids = atol(argv[3]);
    const bool filtered = n_ids >= 0;
    int a = 4;
    std::vector<uint64_t> ids;
    for (long i = 0; i < n_ids && a < argc; ++i, ++a) ids.push_back(strtoull(argv[a], nullptr, 10));
    if ((filtered && (long)ids.size() != n_ids) || (argc - a) % 3) return 2;
    const std::unordered_set<uint64_t> osm_ids(ids.begin(), ids.end());
    const std::unordered_set<uint64_t>* flt = filtered ? &osm_ids : nullptr;
    // the registration's host step and the kernel's twin
    const std::vector<uint64_t> set = id_filter_set(ids.data(), ids.size());
    printf("set %zu", set.size());
    for (uint64_t v : set) printf(" %llu", (unsigned long long)v);
    printf("\n");
    std::vector<uint64_t> wg, mg, ng;
    for (size_t i = 0; i < r.way_count(); ++i) wg.push_back(r.way_global_id(i));
    for (size_t i = 0; i < r.multipolygon_count(); ++i) mg.push_back(r.multipolygon_global_id(i));
    for (size_t i = 0; i < r.node_count(); ++i) ng.push_back(r.node_global_id(i));
    print_plane("ways", wg, set);
    print_plane("multipolygons", mg, set);
    print_plane("nodes", ng, set);
    // draw styles: way i: i % 3 styles, falling ids; multipolygon m: (m + 1) % 3 styles
    StyleBindings sb(0, 0, 18, r.way_count(), r.multipolygon_count());
    for (size_t i = 0; i < r.way_count(); ++i) {
        std::vector<uint32_t> st;
        for (size_t k = 0; k < i % 3; ++k) st.push_back((uint32_t)(7 * i + 5 - k));
        if (!st.empty()) sb.bind_way(i, st);
    }
    for (size_t m = 0; m < r.multipolygon_count(); ++m) {
        std::vector<uint32_t> st;
        for (size_t k = 0; k < (m + 1) % 3; ++k) st.push_back((uint32_t)(11 * m + 9 - k));
        if (!st.empty()) sb.bind_multipolygon(m, st);
    }
    (void)sb.desc();
    // label styles: 0 a text, 1 an icon, 2 a text along the line, 3 a centred text, 4 icon + text
    std::vector<LabelStyle> st(5);
    st[0].rec.has_text_style = st[0].rec.has_font_size = 1, st[0].rec.font_size = 11.5;
    st[1].rec.has_layer = 1, st[1].rec.z_index = -0.0, st[1].rec.has_icon = 1, st[1].rec.icon_image = 3, st[1].icon_height = 7;
    st[2].rec.has_layer = 1, st[2].rec.layer = -1, st[2].rec.has_text_style = st[2].rec.has_font_size = 1, st[2].rec.font_size = 9.0;
    st[2].rec.text_position = OSMT_LABEL_POSITION_LINE;
    st[3].rec.z_index = 2.5, st[3].rec.has_text_style = st[3].rec.has_font_size = 1, st[3].rec.font_size = 14.0;
    st[3].rec.text_position = OSMT_LABEL_POSITION_CENTER;
    st[4].rec.has_icon = 1, st[4].rec.icon_image = 1, st[4].icon_height = 16, st[4].rec.has_text_style = st[4].rec.has_font_size = 1, st[4].rec.font_size = 8.0;
    // node i: i % 4 bindings, binding k: style (i + k) % 4, text none for odd k, else i % 2
    LabelBindings lb(0, 0, 18, r.node_count());
    lb.add_text({0x41, 0x42, 0x43});
    lb.add_text({});
    for (size_t i = 0; i < r.node_count(); ++i) {
        std::vector<osmt_label_binding> b;
        for (uint32_t k = 0; k < i % 4; ++k) b.push_back(osmt_label_binding{(uint32_t)((i + k) % 4), k % 2 ? OSMT_TEXT_NONE : (uint32_t)(i % 2)});
        if (!b.empty()) lb.bind_node(i, b);
    }
    (void)lb.desc();
    // entity i of either kind: i % 4 bindings, binding k: style (i + k) % 5, text none for odd k, else i % 2
    AreaLabelBindings ab(0, 0, 18, r.way_count(), r.multipolygon_count());
    ab.add_text({0x41, 0x42, 0x43});
    ab.add_text({});
    for (int kind = 0; kind < 2; ++kind)
        for (size_t i = 0; i < (kind ? r.multipolygon_count() : r.way_count()); ++i) {
            std::vector<osmt_label_binding> v;
            for (size_t k = 0; k < i % 4; ++k) v.push_back(osmt_label_binding{(uint32_t)((i + k) % 5), k % 2 ? OSMT_TEXT_NONE : (uint32_t)(i % 2)});
            if (v.empty()) continue;
            if (kind)
                ab.bind_multipolygon(i, v);
            else
                ab.bind_way(i, v);
        }
    (void)ab.desc();
    const GeodataDesc g(r);
    const std::vector<double> f = mercator_factors(g.nodes.data(), g.nodes.size() / 2);
    for (; a + 2 < argc; a += 3) {
        osmt_query_tile t{};
        t.zoom = (uint8_t)atoi(argv[a]), t.x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), t.y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
        auto project = [&](uint32_t, double lat, double lon) { return project_libm(lat, lon, t.zoom, t.x, t.y, (double)scale); };
        const std::vector<osmt_styled_area> areas = styled_areas_of_tile(r, sb, t.zoom, t.x, t.y, flt);
        printf("areas %zu", areas.size());
        for (const osmt_styled_area& e : areas) printf(" %u:%u", e.entity, e.style);
        printf("\n");
        NodeLabels nl;
        node_labels_of_tile(r, t.zoom, t.x, t.y, scale, st, lb, project, nl, flt);
        printf("nodes %zu %zu\n", nl.labels.size(), nl.chars.size());
        const HostAnchors host{&g.desc, f.data(), &t, scale};
        size_t asked = 0;
        AreaLabels al;
        area_labels_of_tile(
            r, t.zoom, t.x, t.y, scale, st, ab, project,
            [&](uint32_t e) {
                ++asked;
                return host(0, e);
            },
            al, flt);
        printf("arealabels %zu %zu %zu %zu\n", al.labels.size(), al.chars.size(), al.way_pts.size() / 2, asked);
    }
    return 0;
}
