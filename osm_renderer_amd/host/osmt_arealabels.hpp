/*
 * osmt_arealabels.hpp — host side of the area labels of tile-built scenes (include/osmtile.h, osmt_scene_build_tile_labels_all):
 *
 *   AreaLabelBindings   a CSR builder for osmt_register_area_label_bindings: per way and per multipolygon the (label style,
 *                       text) pairs Styler::style_entities pushes for it, in push order, and the text pool;
 *   HostAnchors         get_label_position of a (tile, entity) pair on this thread, from the arrays that were registered: what
 *                       TileScene::build_all_labels (host/osmt_draw.hpp) calls for the pairs the device declines;
 *   area_labels_of_tile the host mirror of the device build: the osmt_label / osmt_string_run records, chars, way points and
 *                       angles of one tile's way and multipolygon labels, written over
 *                       GeodataReader::get_entities_in_tile_with_neighbors (reader.rs:60-133), sort_styled(.., true) per kind
 *                       and the merge loop of Styler::style_areas (styler.rs:168-203), Labeler::label_entity
 *                       (labeler.rs:16-106) and TextPlacer::place (text_placer.rs:24-168) — it shares no code with the
 *                       kernels and is the yardstick of their tests.  Projection and anchors are parameters: project_libm and
 *                       HostAnchors are the reference's functions with the host's libm; a test hands in the device's own
 *                       points and anchors instead, so that no rounding tie can separate the two.
 */
#ifndef OSMT_AREALABELS_HPP
#define OSMT_AREALABELS_HPP

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_geodata.hpp"
#include "osmt_labelable.hpp"
#include "osmt_styled.hpp"
#include "osmt_tilelabels.hpp"

namespace osmt {

/* Entities of a kind are bound in ascending id, each at most once (one that is skipped has no label style); desc() closes the table. */
class AreaLabelBindings {
  public:
    AreaLabelBindings(uint32_t geodata_id, uint8_t zoom_lo, uint8_t zoom_hi, size_t n_ways, size_t n_multipolygons) : n_{n_ways, n_multipolygons} {
        desc_.geodata_id = geodata_id, desc_.zoom_lo = zoom_lo, desc_.zoom_hi = zoom_hi;
    }
    /* a text of the pool (Unicode scalar values); returns its id */
    uint32_t add_text(const std::vector<uint32_t>& chars) {
        chars_.insert(chars_.end(), chars.begin(), chars.end());
        if (chars_.size() >= 0xFFFFFFFFull || text_off_.size() >= 0xFFFFFFFEull) throw std::runtime_error("AreaLabelBindings: text pool too large");
        text_off_.push_back((uint32_t)chars_.size());
        return (uint32_t)text_off_.size() - 2u;
    }
    void bind_way(size_t way, const std::vector<osmt_label_binding>& b) { bind(0, way, b); }
    void bind_multipolygon(size_t mp, const std::vector<osmt_label_binding>& b) { bind(1, mp, b); }
    /* valid until the next bind_* / add_text call or the end of this object */
    const osmt_area_label_bindings_desc& desc() {
        for (int k = 0; k < 2; ++k) off_[k].resize(n_[k] + 1, (uint32_t)b_[k].size());
        desc_.way_off = off_[0].data(), desc_.way_bindings = b_[0].data(), desc_.n_way_bindings = b_[0].size();
        desc_.multipolygon_off = off_[1].data(), desc_.multipolygon_bindings = b_[1].data(), desc_.n_multipolygon_bindings = b_[1].size();
        desc_.text_off = text_off_.data(), desc_.n_texts = text_off_.size() - 1, desc_.chars = chars_.data(), desc_.n_chars = chars_.size();
        return desc_;
    }
    std::pair<const osmt_label_binding*, size_t> way(size_t i) const { return of(0, i); }
    std::pair<const osmt_label_binding*, size_t> multipolygon(size_t i) const { return of(1, i); }
    std::pair<const uint32_t*, size_t> text(uint32_t id) const { return {chars_.data() + text_off_.at(id), text_off_.at(id + 1) - text_off_.at(id)}; }

  private:
    void bind(int k, size_t id, const std::vector<osmt_label_binding>& b) {
        if (id >= n_[k]) throw std::out_of_range("AreaLabelBindings: entity id out of range");
        if (off_[k].size() > id + 1) throw std::logic_error("AreaLabelBindings: entities are bound in ascending id, each once");
        off_[k].resize(id + 1, (uint32_t)b_[k].size());
        b_[k].insert(b_[k].end(), b.begin(), b.end());
        if (b_[k].size() >= 0xFFFFFFFFull) throw std::runtime_error("AreaLabelBindings: too many bindings for 32-bit offsets");
        off_[k].push_back((uint32_t)b_[k].size());
    }
    std::pair<const osmt_label_binding*, size_t> of(int k, size_t i) const {
        if (i + 1 >= off_[k].size()) return {nullptr, 0}; /* behind the last bound entity */
        return {b_[k].data() + off_[k][i], off_[k][i + 1] - off_[k][i]};
    }
    size_t n_[2];
    std::vector<uint32_t> off_[2] = {{0u}, {0u}}, text_off_{0u}, chars_;
    std::vector<osmt_label_binding> b_[2];
    osmt_area_label_bindings_desc desc_{};
};

/* get_label_position (labelable.rs:191-204) of an entity under a tile, on this thread, from the registered arrays:
 * `geodata`, `factors` ([n_nodes][2], osmt::mercator_factors) and `tiles` (the scene's) must outlive this object. */
struct HostAnchors {
    const osmt_geodata_desc* geodata;
    const double* factors;
    const osmt_query_tile* tiles;
    uint32_t scale;
    osmt_label_position operator()(uint32_t tile, uint32_t entity) const {
        const LabelPosition r = get_label_position(label_rings_of(*geodata, factors, entity, tiles[tile], scale), (double)scale);
        return osmt_label_position{r.x, r.y, r.status, 0u};
    }
};

/* the area labels of a batch, tile behind tile: label l reads chars[labels[l].seg_off .. + n_segs); a text along a way walks
 * way_pts[2 * runs[l].pt_off ..] over n_pts points, with way_sincos beside them */
struct AreaLabels {
    std::vector<osmt_label> labels;
    std::vector<osmt_string_run> runs;
    std::vector<uint32_t> chars;
    std::vector<int32_t> way_pts;
    std::vector<double> way_sincos;
};

/* What osmt_scene_build_tile_labels_all derives for the areas of a tile from its entities (ids: what
 * get_entities_in_tile_with_neighbors returned for the tile), appended to `out`.
 * project(node, lat, lon) -> Point::from_node of that node for this tile and scale; anchor(entity) -> osmt_label_position:
 * get_label_position of the way (its local id) or the multipolygon (id | OSMT_STYLED_MULTIPOLYGON) under this tile, status
 * OSMT_LABEL_OK or OSMT_LABEL_NONE; it is asked once per label that draws an icon or centres a text.
 * Returns the number of labels appended. */
template <class Project, class Anchor>
size_t area_labels_of_entities(const GeodataReader& reader, const OsmEntityIds& ids, uint32_t scale, const std::vector<LabelStyle>& styles,
                               const AreaLabelBindings& bindings, Project project, Anchor anchor, AreaLabels& out) {
    struct Bound : Style { /* one pushed element: the keys sort_styled reads, and what it carries */
        osmt_label_binding b;
    };
    /* Styler::style_entities per kind (styler.rs:128-165): entities in ascending local id, bindings in push order, then sort_by */
    std::vector<Bound> bound[2];
    std::vector<uint32_t> id_of[2];
    for (int k = 0; k < 2; ++k)
        for (uint32_t e : k ? ids.multipolygons : ids.ways) {
            const auto bs = k ? bindings.multipolygon(e) : bindings.way(e);
            for (size_t j = 0; j < bs.second; ++j) {
                const osmt_label_style_rec& r = styles.at(bs.first[j].style).rec;
                Bound el;
                if (r.has_layer) el.layer = r.layer;
                el.z_index = r.z_index;
                el.b = bs.first[j];
                bound[k].push_back(el);
                id_of[k].push_back(e);
            }
        }
    std::vector<StyledEntity> ways(bound[0].size()), mps(bound[1].size());
    for (size_t i = 0; i < ways.size(); ++i) ways[i] = StyledEntity{id_of[0][i], &bound[0][i]};
    for (size_t i = 0; i < mps.size(); ++i) mps[i] = StyledEntity{id_of[1][i], &bound[1][i]};
    sort_styled(ways, [&](uint32_t i) { return reader.way_global_id(i); }, true);
    sort_styled(mps, [&](uint32_t i) { return reader.multipolygon_global_id(i); }, true);
    /* the merge of Styler::style_areas (styler.rs:176-200): the multipolygon goes first unless it compares Greater */
    struct Area {
        bool mp;
        uint32_t id;
        const Bound* el;
    };
    std::vector<Area> areas;
    size_t wi = 0, mi = 0;
    while (wi < ways.size() || mi < mps.size()) {
        bool is_rel_better;
        if (mi >= mps.size())
            is_rel_better = false;
        else if (wi >= ways.size())
            is_rel_better = true;
        else
            is_rel_better = compare_styled_entities(reader.multipolygon_global_id(mps[mi].id), *mps[mi].style, reader.way_global_id(ways[wi].id),
                                                    *ways[wi].style, true) <= 0;
        if (is_rel_better) {
            areas.push_back(Area{true, mps[mi].id, static_cast<const Bound*>(mps[mi].style)});
            ++mi;
        } else {
            areas.push_back(Area{false, ways[wi].id, static_cast<const Bound*>(ways[wi].style)});
            ++wi;
        }
    }
    for (const Area& a : areas) {
        const osmt_label_binding b = a.el->b;
        const LabelStyle& s = styles[b.style];
        /* drawer.rs:233-250: a way's default text position is Line, a multipolygon's Center */
        const bool line = s.rec.text_position == OSMT_LABEL_POSITION_NONE ? !a.mp : s.rec.text_position == OSMT_LABEL_POSITION_LINE;
        /* text_placer.rs:37-47 */
        const bool text = s.rec.has_text_style && s.rec.has_font_size && b.text != OSMT_TEXT_NONE;
        /* labeler.rs:55-57, text_placer.rs:113: the two callers of get_label_position */
        osmt_label_position pos{0.0, 0.0, OSMT_LABEL_NONE, 0u};
        if (s.rec.has_icon || (text && !line)) pos = anchor(a.id | (a.mp ? OSMT_STYLED_MULTIPOLYGON : 0u));
        const bool some = pos.status == OSMT_LABEL_OK;
        const bool icon = s.rec.has_icon && some;
        /* Center without a position and Line without way points (a multipolygon: labelable.rs:53-55) rasterize nothing */
        const bool has_text = text && (line ? !a.mp : some);
        osmt_label l{};
        l.has_icon = icon ? 1 : 0;
        l.has_text = has_text ? 1 : 0;
        if (has_text && s.rec.has_text_color) l.text_color[0] = s.rec.text_color[0], l.text_color[1] = s.rec.text_color[1], l.text_color[2] = s.rec.text_color[2];
        if (icon) l.image_id = s.rec.icon_image;
        l.seg_off = (uint32_t)out.chars.size();
        if (has_text) {
            const auto t = bindings.text(b.text);
            l.n_segs = (uint32_t)t.second;
            out.chars.insert(out.chars.end(), t.first, t.first + t.second);
        }
        if (some) l.icon_center_x = pos.x, l.icon_center_y = pos.y;
        osmt_string_run r{};
        r.position = has_text && line ? OSMT_TEXT_LINE : OSMT_TEXT_CENTER;
        r.y_offset = icon ? s.icon_height / 2u : 0u; /* labeler.rs:61-62 */
        if (has_text) r.font_id = s.rec.font_id, r.font_size = s.rec.font_size * (double)scale;
        r.center_x = l.icon_center_x, r.center_y = l.icon_center_y;
        if (has_text && line) {
            /* get_waypoints (labelable.rs:46-51): Point::from_node of every node; walked from the end when points[0].x > last.x
             * (text_placer.rs:65-67); angles (-atan2(dy, dx)).sin_cos() of the integer differences (:87-101, 256-262) */
            const auto nodes = reader.way_node_ids(a.id);
            std::vector<std::pair<int32_t, int32_t>> pts(nodes.second);
            for (size_t i = 0; i < nodes.second; ++i) pts[i] = project(nodes.first[i], reader.node_lat(nodes.first[i]), reader.node_lon(nodes.first[i]));
            if (!pts.empty() && pts.front().first > pts.back().first) std::reverse(pts.begin(), pts.end());
            r.pt_off = (uint32_t)(out.way_pts.size() / 2);
            r.n_pts = (uint32_t)pts.size();
            for (size_t i = 0; i < pts.size(); ++i) {
                out.way_pts.push_back(pts[i].first);
                out.way_pts.push_back(pts[i].second);
                double sn = 0.0, cs = 0.0;
                if (i + 1 < pts.size()) {
                    const double dy = (double)((int64_t)pts[i + 1].second - (int64_t)pts[i].second);
                    const double dx = (double)((int64_t)pts[i + 1].first - (int64_t)pts[i].first);
                    const double angle = -std::atan2(dy, dx);
                    sn = std::sin(angle), cs = std::cos(angle);
                }
                out.way_sincos.push_back(sn);
                out.way_sincos.push_back(cs);
            }
        }
        out.labels.push_back(l);
        out.runs.push_back(r);
    }
    return areas.size();
}

/* the same for tile (zoom, x, y), with the query; pyramid: the levels registered for the file (nullptr: none) */
template <class Project, class Anchor>
size_t area_labels_of_tile(const GeodataReader& reader, uint8_t zoom, uint32_t x, uint32_t y, uint32_t scale, const std::vector<LabelStyle>& styles,
                           const AreaLabelBindings& bindings, Project project, Anchor anchor, AreaLabels& out,
                           const std::unordered_set<uint64_t>* osm_ids = nullptr, const TilePyramid* pyramid = nullptr) {
    /* osm_ids: the scene's id filter (nullptr: none); an entity it removes is never asked for an anchor */
    return area_labels_of_entities(reader, entities_of_tile(reader, zoom, x, y, osm_ids, pyramid), scale, styles, bindings, project, anchor, out);
}

}  // namespace osmt
#endif
