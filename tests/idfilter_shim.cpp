// C entry points for tests/_idfilter.py (ctypes): the three host twins with their osm_ids argument — osmt::styled_areas_of_tile,
// osmt::node_labels_of_tile, osmt::area_labels_of_tile — over the handles of the other shims (a GeodataReader, a StyleBindings,
// a LabelBindings, an AreaLabelBindings: the same classes of the same headers), and host/osmt_idfilter.hpp.  Host only.
#include <cstddef>
#include <cstring>
#include <unordered_set>

#include "../osm_renderer_amd/host/osmt_arealabels.hpp"
#include "../osm_renderer_amd/host/osmt_idfilter.hpp"
#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

using namespace osmt;

namespace {
typedef std::unordered_set<uint64_t> id_set;
// has_filter 0: None; else Some(the n ids, in the caller's order, repeats and all)
const id_set* set_of(id_set& store, const uint64_t* ids, size_t n, int has_filter) {
    if (!has_filter) return nullptr;
    store.insert(ids, ids + n);
    return &store;
}
std::vector<LabelStyle> styles_of(const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n) {
    std::vector<LabelStyle> st(n);
    for (size_t i = 0; i < n; ++i) st[i].rec = styles[i], st[i].icon_height = icon_h[i];
    return st;
}
}  // namespace

extern "C" {
// osmt::id_filter_set: out gets the sorted unique ids (at most n); returns their number
size_t idf_set(const uint64_t* ids, size_t n, uint64_t* out) {
    const std::vector<uint64_t> s = id_filter_set(ids, n);
    if (!s.empty()) memcpy(out, s.data(), s.size() * 8);
    return s.size();
}
// osmt::id_filter_plane over the set of `ids`: out gets 2 * ceil(n_gids / 64) words; returns their number
size_t idf_plane(const uint64_t* gids, size_t n_gids, const uint64_t* ids, size_t n, uint32_t* out) {
    const std::vector<uint32_t> p = id_filter_plane(gids, n_gids, id_filter_set(ids, n));
    if (!p.empty()) memcpy(out, p.data(), p.size() * 4);
    return p.size();
}

// the areas of one tile; returns their number, nothing is written beyond cap
size_t idf_areas(void* reader, void* bindings, uint8_t zoom, uint32_t x, uint32_t y, const uint64_t* ids, size_t n, int has_filter, osmt_styled_area* out,
                 size_t cap) {
    id_set store;
    const std::vector<osmt_styled_area> a =
        styled_areas_of_tile(*(const GeodataReader*)reader, *(const StyleBindings*)bindings, zoom, x, y, set_of(store, ids, n, has_filter));
    if (a.size() <= cap && !a.empty()) memcpy(out, a.data(), a.size() * sizeof(osmt_styled_area));
    return a.size();
}

// tl_labels of tests/tilelabels_shim.cpp with the filter
void idf_node_labels(void* reader, void* bindings, const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n_styles, uint8_t zoom, uint32_t x,
                     uint32_t y, uint32_t scale, const int32_t* pts, const uint64_t* ids, size_t n, int has_filter, osmt_label* labels, osmt_string_run* runs,
                     uint32_t* chars, const size_t* caps, size_t* counts) {
    const std::vector<LabelStyle> st = styles_of(styles, icon_h, n_styles);
    id_set store;
    NodeLabels out;
    auto project = [&](uint32_t node, double lat, double lon) {
        if (pts) return std::pair<int32_t, int32_t>(pts[2 * node], pts[2 * node + 1]);
        return project_libm(lat, lon, zoom, x, y, (double)scale);
    };
    node_labels_of_tile(*(const GeodataReader*)reader, zoom, x, y, scale, st, *(const LabelBindings*)bindings, project, out, set_of(store, ids, n, has_filter));
    counts[0] = out.labels.size(), counts[1] = out.chars.size();
    if (counts[0] <= caps[0] && counts[1] <= caps[1]) {
        if (counts[0]) memcpy(labels, out.labels.data(), counts[0] * sizeof(osmt_label)), memcpy(runs, out.runs.data(), counts[0] * sizeof(osmt_string_run));
        if (counts[1]) memcpy(chars, out.chars.data(), counts[1] * 4);
    }
}

// al_labels of tests/arealabels_shim.cpp with the filter; asked[0] (may be NULL) gets the number of anchors the twin asked for
void idf_area_labels(void* reader, void* bindings, const osmt_label_style_rec* styles, const uint32_t* icon_h, size_t n_styles, uint8_t zoom, uint32_t x,
                     uint32_t y, uint32_t scale, const int32_t* pts, const osmt_label_position* way_pos, const osmt_label_position* mp_pos, const uint64_t* ids,
                     size_t n, int has_filter, osmt_label* labels, osmt_string_run* runs, uint32_t* chars, int32_t* way_pts, double* way_sincos,
                     const size_t* caps, size_t* counts, size_t* asked) {
    const GeodataReader& r = *(const GeodataReader*)reader;
    const std::vector<LabelStyle> st = styles_of(styles, icon_h, n_styles);
    id_set store;
    const id_set* set = set_of(store, ids, n, has_filter);
    AreaLabels out;
    size_t n_asked = 0;
    auto project = [&](uint32_t node, double lat, double lon) {
        if (pts) return std::pair<int32_t, int32_t>(pts[2 * node], pts[2 * node + 1]);
        return project_libm(lat, lon, zoom, x, y, (double)scale);
    };
    if (way_pos && mp_pos) {
        auto anchor = [&](uint32_t e) {
            ++n_asked;
            return (e & OSMT_STYLED_MULTIPOLYGON) ? mp_pos[e & ~OSMT_STYLED_MULTIPOLYGON] : way_pos[e];
        };
        area_labels_of_tile(r, zoom, x, y, scale, st, *(const AreaLabelBindings*)bindings, project, anchor, out, set);
    } else {
        const GeodataDesc g(r);
        const std::vector<double> f = mercator_factors(g.nodes.data(), g.nodes.size() / 2);
        osmt_query_tile t{};
        t.x = x, t.y = y, t.zoom = zoom;
        const HostAnchors host{&g.desc, f.data(), &t, scale};
        auto anchor = [&](uint32_t e) {
            ++n_asked;
            return host(0, e);
        };
        area_labels_of_tile(r, zoom, x, y, scale, st, *(const AreaLabelBindings*)bindings, project, anchor, out, set);
    }
    if (asked) *asked = n_asked;
    counts[0] = out.labels.size(), counts[1] = out.chars.size(), counts[2] = out.way_pts.size() / 2;
    if (counts[0] <= caps[0] && counts[1] <= caps[1] && counts[2] <= caps[2]) {
        if (counts[0]) memcpy(labels, out.labels.data(), counts[0] * sizeof(osmt_label)), memcpy(runs, out.runs.data(), counts[0] * sizeof(osmt_string_run));
        if (counts[1]) memcpy(chars, out.chars.data(), counts[1] * 4);
        if (counts[2]) memcpy(way_pts, out.way_pts.data(), counts[2] * 8), memcpy(way_sincos, out.way_sincos.data(), counts[2] * 16);
    }
}
}
