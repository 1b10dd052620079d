// C entry points over host/osmt_arealabels.hpp for tests/_arealabels.py (ctypes): osmt::AreaLabelBindings and the host mirror
// osmt::area_labels_of_tile.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"

using namespace osmt;

extern "C" {
// a table from its CSR arrays; entities with an empty range are skipped, as a caller would
void* al_bindings_new(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_ways, const uint32_t* way_off, const osmt_label_binding* wb,
                      size_t n_mps, const uint32_t* mp_off, const osmt_label_binding* mb, size_t n_texts, const uint32_t* text_off, const uint32_t* chars) {
    AreaLabelBindings* lb = new AreaLabelBindings(geodata_id, zoom_lo, zoom_hi, n_ways, n_mps);
    for (size_t t = 0; t < n_texts; ++t) lb->add_text(std::vector<uint32_t>(chars + text_off[t], chars + text_off[t + 1]));
    for (size_t i = 0; i < n_ways; ++i)
        if (way_off[i + 1] > way_off[i]) lb->bind_way(i, std::vector<osmt_label_binding>(wb + way_off[i], wb + way_off[i + 1]));
    for (size_t i = 0; i < n_mps; ++i)
        if (mp_off[i + 1] > mp_off[i]) lb->bind_multipolygon(i, std::vector<osmt_label_binding>(mb + mp_off[i], mb + mp_off[i + 1]));
    return lb;
}
const osmt_area_label_bindings_desc* al_bindings_get(void* b) { return &((AreaLabelBindings*)b)->desc(); }
void al_bindings_free(void* b) { delete (AreaLabelBindings*)b; }

// The area labels of one tile.  pts: NULL = the host's libm projection, else [n_nodes][2] = the point of every node for this tile
// and scale.  way_pos / mp_pos: NULL = get_label_position on the host from the host's Mercator factors, else the anchor of every
// way / multipolygon under this tile.  counts = { labels, chars, way points }; nothing is written beyond caps.
void al_labels(void* reader, void* bindings, const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n_styles, uint8_t zoom, uint32_t x,
               uint32_t y, uint32_t scale, const int32_t* pts, const osmt_label_position* way_pos, const osmt_label_position* mp_pos, osmt_label* labels,
               osmt_string_run* runs, uint32_t* chars, int32_t* way_pts, double* way_sincos, const size_t* caps, size_t* counts) {
    const GeodataReader& r = *(const GeodataReader*)reader;
    std::vector<LabelStyle> st(n_styles);
    for (size_t i = 0; i < n_styles; ++i) st[i].rec = styles[i], st[i].icon_height = icon_h[i];
    AreaLabels out;
    auto project = [&](uint32_t node, double lat, double lon) {
        if (pts) return std::pair<int32_t, int32_t>(pts[2 * node], pts[2 * node + 1]);
        return project_libm(lat, lon, zoom, x, y, (double)scale);
    };
    if (way_pos && mp_pos) {
        auto anchor = [&](uint32_t e) { return (e & OSMT_STYLED_MULTIPOLYGON) ? mp_pos[e & ~OSMT_STYLED_MULTIPOLYGON] : way_pos[e]; };
        area_labels_of_tile(r, zoom, x, y, scale, st, *(const AreaLabelBindings*)bindings, project, anchor, out);
    } else {
        const GeodataDesc g(r);
        const std::vector<double> f = mercator_factors(g.nodes.data(), g.nodes.size() / 2);
        osmt_query_tile t{};
        t.x = x, t.y = y, t.zoom = zoom;
        const HostAnchors host{&g.desc, f.data(), &t, scale};
        area_labels_of_tile(r, zoom, x, y, scale, st, *(const AreaLabelBindings*)bindings, project, [&](uint32_t e) { return host(0, e); }, out);
    }
    counts[0] = out.labels.size(), counts[1] = out.chars.size(), counts[2] = out.way_pts.size() / 2;
    if (counts[0] <= caps[0] && counts[1] <= caps[1] && counts[2] <= caps[2]) {
        if (counts[0]) memcpy(labels, out.labels.data(), counts[0] * sizeof(osmt_label)), memcpy(runs, out.runs.data(), counts[0] * sizeof(osmt_string_run));
        if (counts[1]) memcpy(chars, out.chars.data(), counts[1] * 4);
        if (counts[2]) memcpy(way_pts, out.way_pts.data(), counts[2] * 8), memcpy(way_sincos, out.way_sincos.data(), counts[2] * 16);
    }
}

size_t al_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_area_label_bindings_desc);
        case 1: return sizeof(osmt_area_anchor);
        case 10: return offsetof(osmt_area_label_bindings_desc, way_off);
        case 11: return offsetof(osmt_area_label_bindings_desc, n_chars);
        case 12: return offsetof(osmt_area_anchor, status);
    }
    return 0;
}
}
