// Stand-alone host program over host/osmt_tilelabels.hpp (built with AddressSanitizer and UBSan by tests/_tilelabels.py):
//   tilelabels_host_main <geodata file> <scale> <zoom> <x> <y> [<zoom> <x> <y> ...]
// Four fixed label styles and a fixed binding rule (node i: i % 4 bindings, binding k: style (i + k) % 4, text k % 2 ? none : i % 2),
// the same in tests/test_tile_labels_cpu.py.  Prints NodeIndexDesc's sizes, then one line per label of every tile.
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_tilelabels.hpp"

using namespace osmt;

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 3) % 3 != 0) return 2;
    GeodataReader r(argv[1]);
    const uint32_t scale = (uint32_t)atoi(argv[2]);
    NodeIndexDesc ix(r);
    printf("index %zu %zu %zu\n", ix.desc.n_nodes, ix.node_off.size() - 1, ix.desc.n_node_refs);
    std::vector<LabelStyle> st(4);
    st[0].rec.has_text_style = st[0].rec.has_font_size = 1, st[0].rec.font_size = 11.5;
    st[1].rec.has_layer = 1, st[1].rec.layer = 0, st[1].rec.z_index = -0.0, st[1].rec.has_icon = 1, st[1].rec.icon_image = 3, st[1].icon_height = 7;
    st[2].rec.has_layer = 1, st[2].rec.layer = -1, st[2].rec.has_text_style = st[2].rec.has_font_size = 1, st[2].rec.font_size = 9.0;
    st[2].rec.text_position = OSMT_LABEL_POSITION_LINE;
    st[3].rec.z_index = 2.5, st[3].rec.has_text_style = st[3].rec.has_font_size = st[3].rec.has_text_color = 1, st[3].rec.font_size = 14.0;
    st[3].rec.text_color[0] = 200, st[3].rec.text_color[1] = 10, st[3].rec.text_color[2] = 30, st[3].rec.text_position = OSMT_LABEL_POSITION_CENTER;
    LabelBindings lb(0, 0, 18, r.node_count());
    lb.add_text({0x41, 0x42, 0x43});
    lb.add_text({});
    for (size_t i = 0; i < r.node_count(); ++i) {
        std::vector<osmt_label_binding> b;
        for (uint32_t k = 0; k < i % 4; ++k) b.push_back(osmt_label_binding{(uint32_t)((i + k) % 4), k % 2 ? OSMT_TEXT_NONE : (uint32_t)(i % 2)});
        if (!b.empty()) lb.bind_node(i, b);
    }
    const osmt_label_bindings_desc& d = lb.desc();
    printf("bindings %zu %zu %zu\n", d.n_bindings, d.n_texts, d.n_chars);
    for (int a = 3; a + 2 < argc; a += 3) {
        const uint8_t zoom = (uint8_t)atoi(argv[a]);
        const uint32_t x = (uint32_t)strtoul(argv[a + 1], nullptr, 10), y = (uint32_t)strtoul(argv[a + 2], nullptr, 10);
        NodeLabels out;
        const size_t n = node_labels_of_tile(r, zoom, x, y, scale, st, lb, [&](uint32_t, double lat, double lon) { return project_libm(lat, lon, zoom, x, y, (double)scale); }, out);
        printf("tile %u %u %u %zu %zu\n", zoom, x, y, n, out.chars.size());
        for (size_t l = 0; l < n; ++l) {
            const osmt_label& q = out.labels[l];
            const osmt_string_run& s = out.runs[l];
            printf("%u %u %u %u %u %u %.17g %.17g %.17g %u %u %u\n", q.has_icon, q.has_text, q.image_id, q.seg_off, q.n_segs, s.y_offset, s.font_size, q.icon_center_x,
                   q.icon_center_y, q.text_color[0], q.text_color[1], q.text_color[2]);
        }
    }
    return 0;
}
