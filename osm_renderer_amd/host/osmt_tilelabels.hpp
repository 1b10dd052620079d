/*
 * osmt_tilelabels.hpp — host side of the node labels of tile-built scenes (include/osmtile.h, osmt_scene_build_tile_labels):
 *
 *   NodeIndexDesc       the node half of the z18 tile storage of a geodata file (reader.rs:217-229) and the nodes' global
 *                       ids, as osmt_register_node_index takes them;
 *   LabelStyle          the label half of mapcss::styler::Style (styler.rs:42-72) as osmt_register_label_styles takes it,
 *                       with the height of its icon (what the library looks up in its image registry);
 *   LabelBindings       a CSR builder for osmt_register_label_bindings: per node the (label style, text) pairs
 *                       Styler::style_entities pushes for it, in push order, and the text pool;
 *   node_labels_of_tile the host mirror of the device build: the osmt_label / osmt_string_run records and the chars of one
 *                       tile's node labels, written over GeodataReader::get_entities_in_tile_with_neighbors
 *                       (reader.rs:60-133) and sort_styled(.., true) (styler.rs:163) — it shares no code with the kernels
 *                       and is the yardstick of their tests.  The projection is a parameter: project_libm is
 *                       Point::from_node with the host's libm; a test hands in the device's own points instead, so that no
 *                       rounding tie can separate the two.
 */
#ifndef OSMT_TILELABELS_HPP
#define OSMT_TILELABELS_HPP

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_geodata.hpp"
#include "osmt_styled.hpp"
#include "osmt_tilequery.hpp" /* TilePyramid, entities_of_tile */

namespace osmt {

/* `desc` points into the vectors: valid as long as this object lives and is not copied from. */
struct NodeIndexDesc {
    std::vector<uint64_t> node_ids;
    std::vector<uint32_t> node_off{0u}, nodes;
    osmt_node_index_desc desc{};

    explicit NodeIndexDesc(const GeodataReader& r) {
        for (size_t i = 0; i < r.node_count(); ++i) node_ids.push_back(r.node_global_id(i));
        for (size_t i = 0; i < r.tile_count(); ++i) {
            const auto ids = r.tile_node_ids(i);
            nodes.insert(nodes.end(), ids.first, ids.first + ids.second);
            if (nodes.size() >= 0xFFFFFFFFull) throw std::runtime_error("node index too large for 32-bit offsets");
            node_off.push_back((uint32_t)nodes.size());
        }
        desc.node_ids = node_ids.data(), desc.n_nodes = node_ids.size();
        desc.node_off = node_off.data(), desc.nodes = nodes.data(), desc.n_node_refs = nodes.size();
    }
    NodeIndexDesc(const NodeIndexDesc&) = delete;
    NodeIndexDesc& operator=(const NodeIndexDesc&) = delete;
};

struct LabelStyle {
    osmt_label_style_rec rec{};
    uint32_t icon_height = 0; /* read when rec.has_icon */
};

/* Nodes are bound in ascending id, each at most once (a node that is skipped has no label style); desc() closes the table. */
class LabelBindings {
  public:
    LabelBindings(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_nodes) : n_nodes_(n_nodes) {
        desc_.geodata_id = geodata_id, desc_.zoom_lo = zoom_lo, desc_.zoom_hi = zoom_hi;
    }
    /* a text of the pool (Unicode scalar values); returns its id */
    uint32_t add_text(const std::vector<uint32_t>& chars) {
        chars_.insert(chars_.end(), chars.begin(), chars.end());
        if (chars_.size() >= 0xFFFFFFFFull || text_off_.size() >= 0xFFFFFFFEull) throw std::runtime_error("LabelBindings: text pool too large");
        text_off_.push_back((uint32_t)chars_.size());
        return (uint32_t)text_off_.size() - 2u;
    }
    void bind_node(size_t node, const std::vector<osmt_label_binding>& b) {
        if (node >= n_nodes_) throw std::out_of_range("LabelBindings: node id out of range");
        if (node_off_.size() > node + 1) throw std::logic_error("LabelBindings: nodes are bound in ascending id, each once");
        node_off_.resize(node + 1, (uint32_t)bindings_.size());
        bindings_.insert(bindings_.end(), b.begin(), b.end());
        if (bindings_.size() >= 0xFFFFFFFFull) throw std::runtime_error("LabelBindings: too many bindings for 32-bit offsets");
        node_off_.push_back((uint32_t)bindings_.size());
    }
    /* valid until the next bind_node / add_text call or the end of this object */
    const osmt_label_bindings_desc& desc() {
        node_off_.resize(n_nodes_ + 1, (uint32_t)bindings_.size());
        desc_.node_off = node_off_.data(), desc_.bindings = bindings_.data(), desc_.n_bindings = bindings_.size();
        desc_.text_off = text_off_.data(), desc_.n_texts = text_off_.size() - 1, desc_.chars = chars_.data(), desc_.n_chars = chars_.size();
        return desc_;
    }
    std::pair<const osmt_label_binding*, size_t> node(size_t i) const {
        if (i + 1 >= node_off_.size()) return {nullptr, 0}; /* behind the last bound node */
        return {bindings_.data() + node_off_[i], node_off_[i + 1] - node_off_[i]};
    }
    std::pair<const uint32_t*, size_t> text(uint32_t id) const { return {chars_.data() + text_off_.at(id), text_off_.at(id + 1) - text_off_.at(id)}; }

  private:
    size_t n_nodes_;
    std::vector<uint32_t> node_off_{0u}, text_off_{0u}, chars_;
    std::vector<osmt_label_binding> bindings_;
    osmt_label_bindings_desc desc_{};
};

/* Point::from_node (tile.rs:88-106 + point.rs:11-19) with the host's libm */
inline std::pair<int32_t, int32_t> project_libm(double lat, double lon, uint8_t zoom, uint32_t tx, uint32_t ty, double scale) {
    const double PI = 3.14159265358979323846264338327950288;
    const double lat_rad = lat * (PI / 180.0), lon_rad = lon * (PI / 180.0);
    const double x = lon_rad + PI;
    const double y = PI - std::log(std::tan((PI / 4.0) + (lat_rad / 2.0)));
    const double dim = (double)(OSMT_TILE_SIZE * (1u << zoom));
    const double rx = (x / (2.0 * PI)) * dim - (double)(uint32_t)(tx * OSMT_TILE_SIZE);
    const double ry = (y / (2.0 * PI)) * dim - (double)(uint32_t)(ty * OSMT_TILE_SIZE);
    auto as_i32 = [](double v) { return v != v ? 0 : v >= 2147483647.0 ? INT32_MAX : v <= -2147483648.0 ? INT32_MIN : (int32_t)v; };
    return {as_i32(std::round(rx * scale)), as_i32(std::round(ry * scale))};
}

/* the node labels of a batch, tile behind tile: label l reads chars[labels[l].seg_off .. + n_segs) */
struct NodeLabels {
    std::vector<osmt_label> labels;
    std::vector<osmt_string_run> runs;
    std::vector<uint32_t> chars;
};

/* What osmt_scene_build_tile_labels derives for tile (zoom, x, y), appended to `out`: the nodes of
 * get_entities_in_tile_with_neighbors in ascending local id, each expanded by its bindings in push order
 * (Styler::style_entities), stably sorted by compare_styled_entities(.., for_labels = true), and per element what
 * Labeler::label_entity does with a node.  project(node, lat, lon) -> Point::from_node of that node for this tile and scale.
 * pyramid: the levels registered for the file (nullptr: none) — the result does not depend on it.
 * Returns the number of labels appended. */
template <class Project>
size_t node_labels_of_tile(const GeodataReader& reader, uint8_t zoom, uint32_t x, uint32_t y, uint32_t scale, const std::vector<LabelStyle>& styles,
                           const LabelBindings& bindings, Project project, NodeLabels& out, const std::unordered_set<uint64_t>* osm_ids = nullptr,
                           const TilePyramid* pyramid = nullptr) {
    struct Bound : Style { /* one pushed element: the keys sort_styled reads, and what it carries */
        osmt_label_binding b;
    };
    const OsmEntityIds ids = entities_of_tile(reader, zoom, x, y, osm_ids, pyramid); /* osm_ids: the scene's id filter, nullptr: none */
    std::vector<Bound> bound;
    std::vector<uint32_t> node_of;
    for (uint32_t n : ids.nodes) {
        const auto bs = bindings.node(n);
        for (size_t k = 0; k < bs.second; ++k) {
            const osmt_label_style_rec& r = styles.at(bs.first[k].style).rec;
            Bound e;
            if (r.has_layer) e.layer = r.layer;
            e.z_index = r.z_index;
            e.b = bs.first[k];
            bound.push_back(e);
            node_of.push_back(n);
        }
    }
    std::vector<StyledEntity> v(bound.size());
    for (size_t i = 0; i < bound.size(); ++i) v[i] = StyledEntity{node_of[i], &bound[i]};
    sort_styled(v, [&](uint32_t i) { return reader.node_global_id(i); }, true);
    for (const StyledEntity& e : v) {
        const osmt_label_binding b = static_cast<const Bound*>(e.style)->b;
        const LabelStyle& s = styles[b.style];
        const std::pair<int32_t, int32_t> p = project(e.id, reader.node_lat(e.id), reader.node_lon(e.id));
        /* text_placer.rs:37-58: no font size or no such tag: nothing; a node's default position is Center (drawer.rs:256-260), Line draws nothing on a node */
        const bool has_text = s.rec.has_text_style && s.rec.has_font_size && b.text != OSMT_TEXT_NONE && s.rec.text_position != OSMT_LABEL_POSITION_LINE;
        osmt_label l{};
        l.has_icon = s.rec.has_icon ? 1 : 0;
        l.has_text = has_text ? 1 : 0;
        if (has_text && s.rec.has_text_color) l.text_color[0] = s.rec.text_color[0], l.text_color[1] = s.rec.text_color[1], l.text_color[2] = s.rec.text_color[2];
        if (s.rec.has_icon) l.image_id = s.rec.icon_image;
        l.seg_off = (uint32_t)out.chars.size();
        if (has_text) {
            const auto t = bindings.text(b.text);
            l.n_segs = (uint32_t)t.second;
            out.chars.insert(out.chars.end(), t.first, t.first + t.second);
        }
        l.icon_center_x = (double)p.first, l.icon_center_y = (double)p.second;
        osmt_string_run r{};
        r.position = OSMT_TEXT_CENTER;
        r.y_offset = s.rec.has_icon ? s.icon_height / 2u : 0u; /* labeler.rs:61-62 */
        if (has_text) r.font_id = s.rec.font_id, r.font_size = s.rec.font_size * (double)scale;
        r.center_x = l.icon_center_x, r.center_y = l.icon_center_y;
        out.labels.push_back(l);
        out.runs.push_back(r);
    }
    return v.size();
}

}  // namespace osmt
#endif
