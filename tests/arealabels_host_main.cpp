// Stand-alone host program over host/osmt_arealabels.hpp, built with -fsanitize=address,undefined by
// tests/test_area_labels_cpu.py: osmt::AreaLabelBindings and the mirror osmt::area_labels_of_tile with the host's libm
// projection and osmt::HostAnchors, over a geodata file, with a fixed set of styles and a fixed binding rule the test restates.
//   arealabels_host_main <geodata file> <scale> {<zoom> <x> <y>}...
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"

using namespace osmt;

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 3) % 3) return 2;
    const GeodataReader r(argv[1]);
    const uint32_t scale = (uint32_t)atoi(argv[2]);
    std::vector<LabelStyle> st(5);
    st[0].rec.has_text_style = st[0].rec.has_font_size = 1, st[0].rec.font_size = 11.5;
    st[1].rec.has_layer = 1, st[1].rec.z_index = -0.0, st[1].rec.has_icon = 1, st[1].rec.icon_image = 3, st[1].icon_height = 7;
    st[2].rec.has_layer = 1, st[2].rec.layer = -1, st[2].rec.has_text_style = st[2].rec.has_font_size = 1, st[2].rec.font_size = 9.0;
    st[2].rec.text_position = OSMT_LABEL_POSITION_LINE;
    st[3].rec.z_index = 2.5, st[3].rec.has_text_style = st[3].rec.has_font_size = 1, st[3].rec.font_size = 14.0, st[3].rec.has_text_color = 1;
    st[3].rec.text_color[0] = 200, st[3].rec.text_color[1] = 10, st[3].rec.text_color[2] = 30, st[3].rec.text_position = OSMT_LABEL_POSITION_CENTER;
    st[4].rec.has_icon = 1, st[4].rec.icon_image = 1, st[4].icon_height = 16, st[4].rec.has_text_style = st[4].rec.has_font_size = 1, st[4].rec.font_size = 8.0;
    AreaLabelBindings b(0, 0, 18, r.way_count(), r.multipolygon_count());
    b.add_text({0x41, 0x42, 0x43});
    b.add_text({});
    // entity i of either kind gets i % 4 bindings; binding k: style (i + k) % 5, text none for odd k, else i % 2
    for (int kind = 0; kind < 2; ++kind)
        for (size_t i = 0; i < (kind ? r.multipolygon_count() : r.way_count()); ++i) {
            std::vector<osmt_label_binding> v;
            for (size_t k = 0; k < i % 4; ++k) v.push_back(osmt_label_binding{(uint32_t)((i + k) % 5), k % 2 ? OSMT_TEXT_NONE : (uint32_t)(i % 2)});
            if (v.empty()) continue;
            if (kind)
                b.bind_multipolygon(i, v);
            else
                b.bind_way(i, v);
        }
    const osmt_area_label_bindings_desc& d = b.desc();
    printf("bindings %zu %zu %zu %zu\n", d.n_way_bindings, d.n_multipolygon_bindings, d.n_texts, d.n_chars);
    const GeodataDesc g(r);
    const std::vector<double> f = mercator_factors(g.nodes.data(), g.nodes.size() / 2);
    for (int a = 3; a + 2 < argc; a += 3) {
        osmt_query_tile t{};
        t.zoom = (uint8_t)atoi(argv[a]), t.x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), t.y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
        const HostAnchors host{&g.desc, f.data(), &t, scale};
        AreaLabels out;
        area_labels_of_tile(
            r, t.zoom, t.x, t.y, scale, st, b, [&](uint32_t, double lat, double lon) { return project_libm(lat, lon, t.zoom, t.x, t.y, (double)scale); },
            [&](uint32_t e) { return host(0, e); }, out);
        printf("tile %u %u %u %zu %zu %zu\n", t.zoom, t.x, t.y, out.labels.size(), out.chars.size(), out.way_pts.size() / 2);
        for (size_t i = 0; i < out.labels.size(); ++i) {
            const osmt_label& l = out.labels[i];
            const osmt_string_run& s = out.runs[i];
            printf("%u %u %u %u %u %u %u %u %u %.17g %.17g %.17g %u %u %u\n", l.has_icon, l.has_text, l.image_id, l.seg_off, l.n_segs, s.y_offset, s.position,
                   s.pt_off, s.n_pts, s.font_size, l.icon_center_x, l.icon_center_y, l.text_color[0], l.text_color[1], l.text_color[2]);
        }
        for (size_t i = 0; i < out.way_pts.size() / 2; ++i)
            printf("pt %d %d %.17g %.17g\n", out.way_pts[2 * i], out.way_pts[2 * i + 1], out.way_sincos[2 * i], out.way_sincos[2 * i + 1]);
    }
    return 0;
}
