// C entry points over host/osmt_tilelabels.hpp for tests/_tilelabels.py (ctypes): osmt::NodeIndexDesc, osmt::LabelBindings and
// the host mirror osmt::node_labels_of_tile.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_tilelabels.hpp"

using namespace osmt;

extern "C" {
void* tl_index_new(void* reader) { return new NodeIndexDesc(*(const GeodataReader*)reader); }
const osmt_node_index_desc* tl_index_get(void* d) { return &((NodeIndexDesc*)d)->desc; }
void tl_index_free(void* d) { delete (NodeIndexDesc*)d; }

// a table from its CSR arrays; nodes with an empty range are skipped, as a caller would
void* tl_bindings_new(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_nodes, const uint32_t* node_off, const osmt_label_binding* b,
                      size_t n_texts, const uint32_t* text_off, const uint32_t* chars) {
    LabelBindings* lb = new LabelBindings(geodata_id, zoom_lo, zoom_hi, n_nodes);
    for (size_t t = 0; t < n_texts; ++t) lb->add_text(std::vector<uint32_t>(chars + text_off[t], chars + text_off[t + 1]));
    for (size_t i = 0; i < n_nodes; ++i)
        if (node_off[i + 1] > node_off[i]) lb->bind_node(i, std::vector<osmt_label_binding>(b + node_off[i], b + node_off[i + 1]));
    return lb;
}
const osmt_label_bindings_desc* tl_bindings_get(void* b) { return &((LabelBindings*)b)->desc(); }
void tl_bindings_free(void* b) { delete (LabelBindings*)b; }

// The node labels of one tile.  pts: NULL = the host's libm projection, else [n_nodes][2] = the point of every node for this
// tile and scale.  counts = { labels, chars }; nothing is written beyond caps = { labels, chars }.
void tl_labels(void* reader, void* bindings, const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n_styles, uint8_t zoom, uint32_t x,
               uint32_t y, uint32_t scale, const int32_t* pts, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, const size_t* caps, size_t* counts) {
    std::vector<LabelStyle> st(n_styles);
    for (size_t i = 0; i < n_styles; ++i) st[i].rec = styles[i], st[i].icon_height = icon_h[i];
    NodeLabels out;
    auto project = [&](uint32_t node, double lat, double lon) {
        if (pts) return std::pair<int32_t, int32_t>(pts[2 * node], pts[2 * node + 1]);
        return project_libm(lat, lon, zoom, x, y, (double)scale);
    };
    node_labels_of_tile(*(const GeodataReader*)reader, zoom, x, y, scale, st, *(const LabelBindings*)bindings, project, out);
    counts[0] = out.labels.size(), counts[1] = out.chars.size();
    if (counts[0] <= caps[0] && counts[1] <= caps[1]) {
        if (counts[0]) memcpy(labels, out.labels.data(), counts[0] * sizeof(osmt_label)), memcpy(runs, out.runs.data(), counts[0] * sizeof(osmt_string_run));
        if (counts[1]) memcpy(chars, out.chars.data(), counts[1] * 4);
    }
}

// The node labels of n tiles (zxy: n x {zoom, x, y}) with the host's libm projection, tile behind tile: job_off[n + 1], seg_off
// running over the chars.  counts = { labels, chars }; nothing is written beyond caps.  The per-tile host loop a server runs
// without osmt_scene_build_tile_labels.
void tl_batch(void* reader, void* bindings, const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n_styles, const uint32_t* zxy, size_t n,
              uint32_t scale, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, uint32_t* job_off, const size_t* caps, size_t* counts) {
    std::vector<LabelStyle> st(n_styles);
    for (size_t i = 0; i < n_styles; ++i) st[i].rec = styles[i], st[i].icon_height = icon_h[i];
    NodeLabels out;
    job_off[0] = 0;
    for (size_t t = 0; t < n; ++t) {
        const uint8_t zoom = (uint8_t)zxy[3 * t];
        const uint32_t x = zxy[3 * t + 1], y = zxy[3 * t + 2];
        node_labels_of_tile(*(const GeodataReader*)reader, zoom, x, y, scale, st, *(const LabelBindings*)bindings,
                            [&](uint32_t, double lat, double lon) { return project_libm(lat, lon, zoom, x, y, (double)scale); }, out);
        job_off[t + 1] = (uint32_t)out.labels.size();
    }
    counts[0] = out.labels.size(), counts[1] = out.chars.size();
    if (counts[0] <= caps[0] && counts[1] <= caps[1]) {
        if (counts[0]) memcpy(labels, out.labels.data(), counts[0] * sizeof(osmt_label)), memcpy(runs, out.runs.data(), counts[0] * sizeof(osmt_string_run));
        if (counts[1]) memcpy(chars, out.chars.data(), counts[1] * 4);
    }
}

void tl_project(double lat, double lon, uint8_t zoom, uint32_t x, uint32_t y, double scale, int32_t* xy) {
    const auto p = project_libm(lat, lon, zoom, x, y, scale);
    xy[0] = p.first, xy[1] = p.second;
}

size_t tl_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_node_index_desc);
        case 1: return sizeof(osmt_label_style_rec);
        case 2: return sizeof(osmt_label_binding);
        case 3: return sizeof(osmt_label_bindings_desc);
        case 10: return offsetof(osmt_node_index_desc, n_node_refs);
        case 11: return offsetof(osmt_label_style_rec, has_layer);
        case 12: return offsetof(osmt_label_style_rec, text_position);
        case 13: return offsetof(osmt_label_bindings_desc, node_off);
        case 14: return offsetof(osmt_label_bindings_desc, n_chars);
    }
    return 0;
}
}
