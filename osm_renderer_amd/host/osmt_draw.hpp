/*
 * osmt_draw.hpp — C++ host-side mirror of the reference's draw interface, above the C ABI.
 *
 * The reference is Rust and no Rust toolchain exists in this image, so the host side that
 * would live in src/draw/{tile_pixels,fill,line,drawer}.rs is written here in C++ with the
 * SAME names, argument meaning and call order:
 *
 *   reference (Rust)                                         here (C++)
 *   tile::Tile {zoom,x,y}                 tile.rs:9-13       osmt::Tile
 *   draw::point::Point {x,y}              point.rs:5-8       osmt::Point
 *   mapcss::color::Color {r,g,b}          color.rs:2-6       osmt::Color
 *   mapcss::styler::LineCap               styler.rs:11-16    osmt::LineCap (+ std::optional)
 *   draw::fill::Filler                    fill.rs:11-14      osmt::Filler
 *   TilePixels::new/reset/bump_generation/
 *     blend_unfinished_pixels/to_rgb_triples/dimension
 *                                         tile_pixels.rs:57,89,150,154,164,183
 *                                                            osmt::TilePixels (same methods)
 *   fill_contour(points, &filler, opacity, &mut pixels)      fill.rs:16     osmt::fill_contour
 *   draw_lines(points, width, &color, opacity, &dashes,
 *              &line_cap, use_caps_for_dashes, &mut pixels)  line.rs:9-18   osmt::draw_lines
 *   TileRenderedPixels {triples, dimension}                  drawer.rs:27-30 osmt::TileRenderedPixels
 *
 * Semantics: the draw calls are RECORDED into a display list (one op per call, in order —
 * the generation order of drawer.rs:218); nothing is rasterised on the CPU.  The list is
 * executed on the GPU when pixels are requested (to_rgb_triples) or when a TileBatch of
 * several recorded tiles is flushed with one osmt_render_batch call.  Because pixels can only
 * be observed through to_rgb_triples(), deferred execution is indistinguishable from the
 * reference's eager canvas (labels — out of scope — are the one reader that would need
 * osmt_render_scene_f64 instead).
 *
 * Errors: the reference returns anyhow::Result up to the server; here every failing ABI call
 * throws osmt::Error(code, osmt_last_error()).
 */
#ifndef OSMT_DRAW_HPP
#define OSMT_DRAW_HPP

#include <algorithm>
#include <cstdint>
#include <cmath>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"

namespace osmt {

constexpr uint32_t TILE_SIZE = OSMT_TILE_SIZE; /* tile.rs:6 */
constexpr uint8_t MAX_ZOOM = OSMT_MAX_ZOOM;    /* tile.rs:5 */

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc != OSMT_OK) throw Error(rc, osmt_last_error());
}

struct Tile {
    uint8_t zoom;
    uint32_t x, y;
};
struct Point {
    int32_t x, y;
};
struct Color {
    uint8_t r, g, b;
};
enum class LineCap { Butt, Round, Square };
using PointPairs = std::vector<std::pair<Point, Point>>; /* PointPairIter (point_pairs.rs:5) */
using RgbTriples = std::vector<std::tuple<uint8_t, uint8_t, uint8_t>>; /* tile_pixels.rs:46 */
struct TileRenderedPixels {
    RgbTriples triples;
    size_t dimension;
};

/* Drawer + worker pool state: one per GPU. */
class Context {
  public:
    explicit Context(int device = 0) {
        osmt_config cfg{device, 0};
        check(osmt_create(&cfg, &ctx_));
    }
    ~Context() { osmt_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    osmt_ctx* raw() const { return ctx_; }
    /* IconCache entry (icon_cache.rs:21-45): straight-alpha RGBA8 pixels of a decoded PNG */
    uint32_t register_image(const uint8_t* rgba8, uint32_t w, uint32_t h) {
        uint32_t id = 0;
        check(osmt_register_image(ctx_, rgba8, w, h, &id));
        return id;
    }
    /* the font's outlines for glyph-run texts (Rasterizer::draw_glyph): glyph i of the call is v[vertex_off[i] ..
     * vertex_off[i + 1]) (stb_truetype's Vertex list of get_glyph_shape; empty for a glyph without shape) and gets the
     * returned id + i */
    uint32_t register_glyphs(const osmt_glyph_vertex* v, const uint32_t* vertex_off, uint32_t n_glyphs) {
        uint32_t id = 0;
        check(osmt_register_glyphs(ctx_, v, vertex_off, n_glyphs, &id));
        return id;
    }
    /* display lists built on the GPU: a geodata file's topology (osmt::GeodataDesc in osmt_geodata.hpp fills the desc) and
     * the stylesheet's Style records (osmt::style_rec_of in osmt_styled.hpp), registered once per context */
    uint32_t register_geodata(const osmt_geodata_desc& desc) {
        uint32_t id = 0;
        check(osmt_register_geodata(ctx_, &desc, &id));
        return id;
    }
    uint32_t register_styles(const std::vector<osmt_style_rec>& styles, const std::vector<double>& dash_pool) {
        uint32_t first = 0;
        check(osmt_register_styles(ctx_, styles.data(), styles.size(), dash_pool.data(), dash_pool.size(), &first));
        return first;
    }
    /* scenes built from tile coordinates: the z18 tile index of a registered file (osmt::TileIndexDesc in
     * osmt_tilequery.hpp) and a table entity -> style ids per zoom range (osmt::StyleBindings there) */
    void register_tile_index(uint32_t geodata_id, const osmt_tile_index_desc& desc) { check(osmt_register_tile_index(ctx_, geodata_id, &desc)); }
    uint32_t register_style_bindings(const osmt_style_bindings_desc& desc) {
        uint32_t id = 0;
        check(osmt_register_style_bindings(ctx_, &desc, &id));
        return id;
    }
    /* a font's lookup tables for string labels (text_placer.rs:170-197) */
    uint32_t register_font(const osmt_font_desc& font) {
        uint32_t id = 0;
        check(osmt_register_font(ctx_, &font, &id));
        return id;
    }
    /* node labels of tile-built scenes: the node lists of the registered tile index (osmt::NodeIndexDesc in
     * osmt_tilelabels.hpp), the label half of the Style records, and a table node -> (label style, text) per zoom range
     * (osmt::LabelBindings there) */
    void register_node_index(uint32_t geodata_id, const osmt_node_index_desc& desc) { check(osmt_register_node_index(ctx_, geodata_id, &desc)); }
    /* the z18 tile index built on the device from the registered Mercator factors (osmt_build_tile_index); node_ids: the nodes'
     * global ids, one per node of the geodata, registers the node index too; nullptr: the tile index alone */
    void build_tile_index(uint32_t geodata_id, const std::vector<uint64_t>* node_ids = nullptr) {
        static const uint64_t none = 0; /* a file of 0 nodes still asks for the node index with a non-NULL pointer */
        const uint64_t* ids = !node_ids ? nullptr : node_ids->empty() ? &none : node_ids->data();
        check(osmt_build_tile_index(ctx_, geodata_id, ids, node_ids ? node_ids->size() : 0));
    }
    /* multipolygon rings assembled on the device from relations' member ways (osmt_assemble_multipolygons).  `out` is the helper
     * osmt::AssembledPolygons (host/osmt_polygons.hpp, or anything with its vectors): out.into(geodata_desc) writes the arrays
     * into an osmt::GeodataDesc, and the chain goes on with register_geodata, register_node_mercator and build_tile_index */
    template <class Polygons>
    void assemble_multipolygons(const osmt_relations_desc& relations, Polygons& out) {
        check(osmt_validate_relations(&relations));
        osmt_polygons* p = nullptr;
        check(osmt_assemble_multipolygons(ctx_, &relations, &p));
        size_t n[4] = {0, 0, 0, 0};
        int rc = osmt_polygons_counts(p, n);
        if (rc == OSMT_OK) {
            out.polygon_node_off.assign(n[0] + 1, 0u), out.polygon_nodes.assign(n[1], 0u), out.multipolygon_ids.assign(n[2], 0u);
            out.multipolygon_polygon_off.assign(n[2] + 1, 0u), out.multipolygon_polygons.assign(n[3], 0u), out.multipolygon_relation.assign(n[2], 0u);
            out.status.assign(relations.n_relations, osmt_relation_status{0u, 0u, 0u});
            rc = osmt_polygons_read(ctx_, p, out.polygon_node_off.data(), out.polygon_nodes.data(), out.multipolygon_ids.data(), out.multipolygon_polygon_off.data(),
                                    out.multipolygon_polygons.data(), out.status.data(), out.multipolygon_relation.data());
        }
        osmt_polygons_free(p);
        check(rc);
    }
    /* OSM ids resolved to local indices on the device (osmt_resolve_refs): the step before assemble_multipolygons.  `out` is
     * osmt::ResolvedRefs (host/osmt_resolve.hpp, or anything with its vectors and counts) */
    template <class Resolved>
    void resolve_refs(const osmt_raw_osm_desc& raw, Resolved& out) {
        check(osmt_validate_resolve(&raw));
        osmt_resolved* r = nullptr;
        check(osmt_resolve_refs(ctx_, &raw, &r));
        size_t n[5] = {0, 0, 0, 0, 0};
        int rc = osmt_resolved_counts(r, n);
        if (rc == OSMT_OK) {
            out.way_node_off.assign(raw.n_ways + 1, 0u), out.way_nodes.assign(n[0], 0u), out.relation_way_off.assign(raw.n_relations + 1, 0u);
            out.relation_ways.assign(n[1], 0u), out.relation_way_inner.assign(n[1], 0u);
            for (int i = 0; i < 5; ++i) out.counts[i] = n[i];
            rc = osmt_resolved_read(ctx_, r, out.way_node_off.data(), out.way_nodes.data(), out.relation_way_off.data(), out.relation_ways.data(),
                                    out.relation_way_inner.data());
        }
        osmt_resolved_free(r);
        check(rc);
    }
    uint32_t register_label_styles(const std::vector<osmt_label_style_rec>& styles) {
        uint32_t first = 0;
        check(osmt_register_label_styles(ctx_, styles.data(), styles.size(), &first));
        return first;
    }
    uint32_t register_area_label_bindings(const osmt_area_label_bindings_desc& desc) {
        uint32_t id = 0;
        check(osmt_register_area_label_bindings(ctx_, &desc, &id));
        return id;
    }
    uint32_t register_label_bindings(const osmt_label_bindings_desc& desc) {
        uint32_t id = 0;
        check(osmt_register_label_bindings(ctx_, &desc, &id));
        return id;
    }
    /* the osm_ids filter of get_entities_in_tile_with_neighbors (reader.rs:60,95-99) as a registered set of global ids: any
     * order, repeats allowed, an empty set keeps nothing.  Register the node index first if the scenes' nodes are labelled. */
    uint32_t register_id_filter(uint32_t geodata_id, const std::vector<uint64_t>& osm_ids) {
        uint32_t id = 0;
        check(osmt_register_id_filter(ctx_, geodata_id, osm_ids.data(), osm_ids.size(), &id));
        return id;
    }
    /* tile coordinates in, PNG files out (defined behind TileScene); id_filter: from register_id_filter, or OSMT_ID_FILTER_NONE */
    template <class HostAnchor>
    std::vector<std::vector<uint8_t>> render_tiles_png(const osmt_tile_batch& batch, const uint32_t* area_bindings_of_zoom,
                                                       const uint32_t* node_bindings_of_zoom, HostAnchor host_anchor,
                                                       uint32_t id_filter = OSMT_ID_FILTER_NONE);

  private:
    osmt_ctx* ctx_ = nullptr;
};

/* Host output of any scene (osmt_render_scene_png / osmt_render_scene_host): what the scene classes below share.  The scene
 * is borrowed: it renders the same afterwards. */
inline std::vector<std::vector<uint8_t>> scene_render_png(osmt_ctx* ctx, osmt_scene* scene, size_t n_tiles, uint32_t scale) {
    const uint32_t dim = TILE_SIZE * scale;
    std::vector<uint8_t> blob(n_tiles * osmt_png_device_bound(dim, dim)); /* the worst case: the call cannot come back short */
    std::vector<uint64_t> off(n_tiles + 1, 0);
    check(osmt_render_scene_png(ctx, scene, blob.data(), blob.size(), off.data()));
    std::vector<std::vector<uint8_t>> files(n_tiles);
    for (size_t i = 0; i < n_tiles; ++i) files[i].assign(blob.begin() + (ptrdiff_t)off[i], blob.begin() + (ptrdiff_t)off[i + 1]);
    return files;
}
/* packed RGB8 (the memory of RgbTriples), or RGBA8 with rgb = false; tile i at [i * dim * dim * (3 or 4)) */
inline std::vector<uint8_t> scene_render_host(osmt_ctx* ctx, osmt_scene* scene, size_t n_tiles, uint32_t scale, bool rgb) {
    const size_t dim = (size_t)TILE_SIZE * scale, stride = dim * dim * (rgb ? 3 : 4);
    std::vector<uint8_t> out(n_tiles * stride + 4); /* never empty; operator new aligns far beyond the 4 bytes RGB8 asks for */
    check(osmt_render_scene_host(ctx, scene, rgb ? OSMT_PIXELS_RGB8 : OSMT_PIXELS_RGBA8, out.data(), stride));
    out.resize(n_tiles * stride);
    return out;
}

/* A scene whose display list the GPU built from a styled batch (osmt_scene_build_styled): what SceneBuilder::add_tile per
 * tile + osmt_scene_upload give, from 8 bytes per styled area.  Render it with osmt_render_scene on raw(), or straight to
 * files / host pixels with render_png() / render_host(). */
class StyledScene {
  public:
    StyledScene(Context& ctx, const osmt_styled_batch& batch) : ctx_(&ctx), n_tiles_(batch.n_tiles), scale_(batch.scale) {
        check(osmt_scene_build_styled(ctx.raw(), &batch, &scene_));
    }
    ~StyledScene() { osmt_scene_free(scene_); }
    StyledScene(const StyledScene&) = delete;
    StyledScene& operator=(const StyledScene&) = delete;
    osmt_scene* raw() const { return scene_; }
    size_t tile_count() const { return n_tiles_; }
    std::vector<std::vector<uint8_t>> render_png() const { return scene_render_png(ctx_->raw(), scene_, n_tiles_, scale_); }
    std::vector<uint8_t> render_host(bool rgb = true) const { return scene_render_host(ctx_->raw(), scene_, n_tiles_, scale_, rgb); }

  private:
    Context* ctx_;
    size_t n_tiles_;
    uint32_t scale_;
    osmt_scene* scene_ = nullptr;
};

/* One round of the TOO_LARGE retry loop: the pairs a call declined (`more`) are computed on this thread by
 * host_anchor(tile index, entity) -> osmt_label_position and merged into the anchors the next call hands in.  A declined pair
 * was not listed: the two lists are disjoint and each ascending by (tile, entity). */
template <class HostAnchor>
inline void add_computed_anchors(std::vector<osmt_area_anchor>& anchors, std::vector<osmt_area_anchor>& more, HostAnchor& host_anchor) {
    for (osmt_area_anchor& a : more) {
        const osmt_label_position p = host_anchor(a.tile, a.entity);
        a.x = p.x, a.y = p.y, a.status = p.status;
    }
    std::vector<osmt_area_anchor> merged(anchors.size() + more.size());
    std::merge(anchors.begin(), anchors.end(), more.begin(), more.end(), merged.begin(), [](const osmt_area_anchor& a, const osmt_area_anchor& b) {
        return a.tile < b.tile || (a.tile == b.tile && a.entity < b.entity);
    });
    anchors.swap(merged);
}
/* The loop itself for the tile-server calls, whose declined pairs are the calling thread's (osmt_last_declined_anchors):
 * call(anchors) -> the C call's return code.  Returns how many anchors the host computed. */
template <class Call, class HostAnchor>
inline size_t retry_with_host_anchors(Call call, HostAnchor host_anchor) {
    std::vector<osmt_area_anchor> anchors;
    for (;;) {
        const int rc = call(anchors);
        if (rc == OSMT_OK) return anchors.size();
        const std::string why = osmt_last_error();
        size_t n = 0;
        check(osmt_last_declined_anchors(nullptr, 0, &n));
        if (rc != OSMT_UNSUPPORTED || n == 0) throw Error(rc, why);
        std::vector<osmt_area_anchor> more(n);
        check(osmt_last_declined_anchors(more.data(), n, &n));
        add_computed_anchors(anchors, more, host_anchor);
    }
}

/* The node labels a TileScene built on the GPU, as read back: label l reads chars[labels[l].seg_off .. + n_segs), tile t owns
 * labels [job_label_off[t], job_label_off[t + 1]). */
struct TileLabels {
    std::vector<osmt_label> labels;
    std::vector<osmt_string_run> runs;
    std::vector<uint32_t> chars, job_label_off;
};

/* The area labels a TileScene built on the GPU, as read back: TileLabels plus the ways of the texts along a line — run l
 * walks way_pts[runs[l].pt_off .. + n_pts) ([n][2], in walking order) with the angles way_sincos ([n][2]). */
struct TileAreaLabels : TileLabels {
    std::vector<int32_t> way_pts;
    std::vector<double> way_sincos;
};

/* A scene built from tile coordinates (osmt_scene_build_tiles): 16 bytes per tile in, the scene StyledScene builds from the
 * same entities out.  build_tile_labels gives it the label pass of Drawer::draw_labels: the node labels are queried, ordered
 * and assembled on the GPU, the caller's way and multipolygon labels are drawn in front of them (drawer.rs:229-261). */
class TileScene {
  public:
    /* id_filter: from Context::register_id_filter — only listed entities are drawn and labelled; OSMT_ID_FILTER_NONE: all */
    TileScene(Context& ctx, const osmt_tile_batch& batch, uint32_t id_filter = OSMT_ID_FILTER_NONE)
        : ctx_(&ctx), n_tiles_(batch.n_tiles), scale_(batch.scale) {
        check(osmt_scene_build_tiles_filtered(ctx.raw(), &batch, id_filter, &scene_));
    }
    ~TileScene() { osmt_scene_free(scene_); }
    TileScene(const TileScene&) = delete;
    TileScene& operator=(const TileScene&) = delete;
    osmt_scene* raw() const { return scene_; }
    size_t tile_count() const { return n_tiles_; }
    /* label_bindings_of_zoom[z]: id from Context::register_label_bindings, or OSMT_BINDINGS_NONE */
    void build_tile_labels(const uint32_t (&label_bindings_of_zoom)[OSMT_MAX_ZOOM + 1], const osmt_string_label_batch* area_labels = nullptr) {
        check(osmt_scene_build_tile_labels(ctx_->raw(), scene_, label_bindings_of_zoom, area_labels));
    }
    /* The whole label pass of Drawer::draw_labels from the GPU: the labels of ways and multipolygons (nullptr: none), then of
     * nodes (nullptr: none).  Where the anchor search declines a pair as too large, host_anchor(tile index, entity) ->
     * osmt_label_position computes it on this thread (osmt::HostAnchors of host/osmt_arealabels.hpp) and the build is repeated
     * with the computed anchors; returns how many anchors the host computed. */
    template <class HostAnchor>
    size_t build_all_labels(const uint32_t* area_bindings_of_zoom, const uint32_t* node_bindings_of_zoom, HostAnchor host_anchor) {
        std::vector<osmt_area_anchor> anchors;
        for (;;) {
            const int rc = osmt_scene_build_tile_labels_all(ctx_->raw(), scene_, area_bindings_of_zoom, node_bindings_of_zoom, anchors.data(), anchors.size());
            if (rc == OSMT_OK) return anchors.size();
            const std::string why = osmt_last_error();
            size_t n = 0;
            check(osmt_scene_read_declined_anchors(ctx_->raw(), scene_, nullptr, 0, &n));
            if (rc != OSMT_UNSUPPORTED || n == 0) throw Error(rc, why);
            std::vector<osmt_area_anchor> more(n);
            check(osmt_scene_read_declined_anchors(ctx_->raw(), scene_, more.data(), n, &n));
            add_computed_anchors(anchors, more, host_anchor);
        }
    }
    /* Drawer::draw_tile's tail for every tile of the scene (drawer.rs:48-57): the PNG files, written by the GPU — with whatever
     * labels are attached; and the pixels themselves in host memory */
    std::vector<std::vector<uint8_t>> render_png() const { return scene_render_png(ctx_->raw(), scene_, n_tiles_, scale_); }
    std::vector<uint8_t> render_host(bool rgb = true) const { return scene_render_host(ctx_->raw(), scene_, n_tiles_, scale_, rgb); }
    /* the area batch the device built, before the splice */
    TileAreaLabels read_tile_area_labels() const {
        TileAreaLabels out;
        size_t n[3] = {0, 0, 0};
        check(osmt_scene_read_tile_area_labels(ctx_->raw(), scene_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n));
        out.labels.resize(n[0]), out.runs.resize(n[0]), out.chars.resize(n[1]), out.way_pts.resize(2 * n[2]), out.way_sincos.resize(2 * n[2]);
        out.job_label_off.resize(n_tiles_ + 1);
        check(osmt_scene_read_tile_area_labels(ctx_->raw(), scene_, out.labels.data(), out.runs.data(), out.chars.data(), out.way_pts.data(),
                                               out.way_sincos.data(), out.job_label_off.data(), n, n));
        return out;
    }
    /* the node batch the device built, before the area labels were put in front */
    TileLabels read_tile_labels() const {
        TileLabels out;
        size_t n[2] = {0, 0};
        check(osmt_scene_read_tile_labels(ctx_->raw(), scene_, nullptr, nullptr, nullptr, nullptr, nullptr, n));
        out.labels.resize(n[0]), out.runs.resize(n[0]), out.chars.resize(n[1]), out.job_label_off.resize(n_tiles_ + 1);
        check(osmt_scene_read_tile_labels(ctx_->raw(), scene_, out.labels.data(), out.runs.data(), out.chars.data(), out.job_label_off.data(), n, n));
        return out;
    }

  private:
    Context* ctx_;
    size_t n_tiles_;
    uint32_t scale_;
    osmt_scene* scene_ = nullptr;
};

/* Drawer::draw_tile (drawer.rs:40-58) for tile coordinates, in one call: build the scenes of `batch`, label them from the
 * registered bindings (nullptr: none of that kind; host_anchor as in TileScene::build_all_labels), render, PNG files out —
 * file i belongs to batch.tiles[i]. */
template <class HostAnchor>
inline std::vector<std::vector<uint8_t>> Context::render_tiles_png(const osmt_tile_batch& batch, const uint32_t* area_bindings_of_zoom,
                                                                   const uint32_t* node_bindings_of_zoom, HostAnchor host_anchor,
                                                                   uint32_t id_filter) {
    TileScene scene(*this, batch, id_filter);
    if (area_bindings_of_zoom || node_bindings_of_zoom) scene.build_all_labels(area_bindings_of_zoom, node_bindings_of_zoom, host_anchor);
    return scene.render_png();
}

/* What a server renders its requests with, stated once (osmt_tile_server): geodata, bindings per zoom, canvas, id filter.
 * Immutable; one instance serves every thread. */
class TileServer {
  public:
    TileServer(Context& ctx, const osmt_tile_server_desc& desc) { check(osmt_tile_server_create(ctx.raw(), &desc, &server_)); }
    ~TileServer() { osmt_tile_server_free(server_); }
    TileServer(const TileServer&) = delete;
    TileServer& operator=(const TileServer&) = delete;
    osmt_tile_server* raw() const { return server_; }
    /* a description with no bindings, no filter and the canvas given: fill in the ids per zoom */
    static osmt_tile_server_desc describe(uint32_t geodata_id, const std::optional<Color>& canvas = std::nullopt) {
        osmt_tile_server_desc d{};
        d.geodata_id = geodata_id, d.use_caps_for_dashes = 1, d.id_filter = OSMT_ID_FILTER_NONE;
        if (canvas) d.has_canvas = 1, d.canvas_rgb[0] = canvas->r, d.canvas_rgb[1] = canvas->g, d.canvas_rgb[2] = canvas->b;
        for (uint32_t z = 0; z <= OSMT_MAX_ZOOM; ++z)
            d.bindings_of_zoom[z] = d.area_label_bindings_of_zoom[z] = d.node_label_bindings_of_zoom[z] = OSMT_BINDINGS_NONE;
        return d;
    }
    /* Tiles in, files out (osmt_tile_server_render_png): file i belongs to tiles[i].  host_anchor(tile index, entity) computes
     * the anchors the device declines, as in TileScene::build_all_labels; *on_host (may be NULL) gets their number. */
    template <class HostAnchor>
    std::vector<std::vector<uint8_t>> render_png(const std::vector<osmt_tile_coord>& tiles, uint32_t scale, HostAnchor host_anchor,
                                                 size_t* on_host = nullptr) const {
        const uint32_t dim = TILE_SIZE * scale;
        std::vector<uint8_t> blob(tiles.size() * osmt_png_device_bound(dim, dim)); /* the worst case: the call cannot come back short */
        std::vector<uint64_t> off(tiles.size() + 1, 0);
        const size_t n = retry_with_host_anchors(
            [&](const std::vector<osmt_area_anchor>& anchors) {
                return osmt_tile_server_render_png(server_, tiles.data(), tiles.size(), scale, anchors.data(), anchors.size(), blob.data(), blob.size(),
                                                   off.data());
            },
            host_anchor);
        if (on_host) *on_host = n;
        std::vector<std::vector<uint8_t>> files(tiles.size());
        for (size_t i = 0; i < tiles.size(); ++i) files[i].assign(blob.begin() + (ptrdiff_t)off[i], blob.begin() + (ptrdiff_t)off[i + 1]);
        return files;
    }

  private:
    osmt_tile_server* server_ = nullptr;
};

/* The per-thread request handle of the reference's server loop (http_server.rs:50-83): concurrent render_tile_png calls of the
 * workers of one context, for the same server and scale, share launches (osmt_worker_render_tile_png). */
class Worker {
  public:
    explicit Worker(Context& ctx) { check(osmt_worker_create(ctx.raw(), &worker_)); }
    ~Worker() { osmt_worker_destroy(worker_); }
    Worker(const Worker&) = delete;
    Worker& operator=(const Worker&) = delete;
    osmt_worker* raw() const { return worker_; }
    /* One tile, one file.  host_anchor(0, entity) computes the anchors the device declines for THIS tile. */
    template <class HostAnchor>
    std::vector<uint8_t> render_tile_png(const TileServer& server, const osmt_tile_coord& tile, uint32_t scale, HostAnchor host_anchor,
                                         size_t* on_host = nullptr) {
        const uint32_t dim = TILE_SIZE * scale;
        std::vector<uint8_t> file(osmt_png_device_bound(dim, dim));
        size_t len = 0;
        const size_t n = retry_with_host_anchors(
            [&](const std::vector<osmt_area_anchor>& anchors) {
                return osmt_worker_render_tile_png(worker_, server.raw(), &tile, scale, anchors.data(), anchors.size(), file.data(), file.size(), &len);
            },
            host_anchor);
        if (on_host) *on_host = n;
        file.resize(len);
        return file;
    }

  private:
    osmt_worker* worker_ = nullptr;
};

struct Filler { /* fill.rs:11-14 */
    enum Kind { ColorFill, ImageFill } kind;
    Color color;
    uint32_t image_id;
    static Filler from_color(const Color& c) { return Filler{ColorFill, c, 0}; }
    static Filler from_image(uint32_t id) { return Filler{ImageFill, Color{0, 0, 0}, id}; }
};

class TileBatch;

/* The per-worker canvas of the reference (http_server.rs:25-28,69-72), as a recorder. */
class TilePixels {
  public:
    TilePixels(Context& ctx, size_t scale) : ctx_(&ctx), scale_(scale) {}

    /* tile_pixels.rs:89-105 */
    void reset(const std::optional<Color>& canvas_color) {
        ops_.clear();
        rings_.clear();
        points_.clear();
        dashes_.clear();
        canvas_ = canvas_color;
        pending_op_ = false;
        labels_.clear();
        label_segs_.clear();
        label_glyphs_.clear();
        pending_label_ = osmt_label{};
    }
    /* drawer.rs:218: closes the current area; an area that drew nothing still counts */
    void bump_generation() {
        if (!pending_op_) {
            osmt_op nop{};
            nop.kind = OSMT_OP_NONE;
            ops_.push_back(nop);
        }
        pending_op_ = false;
    }
    /* tile_pixels.rs:154-158: a no-op for a recorder (blending happens on the GPU, in order) */
    void blend_unfinished_pixels(bool /*for_labels*/) {}
    /* tile_pixels.rs:160-162: closes the current label (one Labeler::label_entity call, labeler.rs:16-38).
     * The verdict itself is computed on the GPU (set_label_pixel's collision rule needs every earlier label);
     * the argument is accepted for source compatibility and ignored. */
    void bump_label_generation(bool /*succeeded*/) {
        labels_.push_back(pending_label_);
        pending_label_ = osmt_label{};
    }
    size_t dimension() const { return TILE_SIZE * scale_; } /* tile_pixels.rs:183-185 */
    size_t scale() const { return scale_; }

    /* tile_pixels.rs:164-181: runs the recorded list for `tile` on the GPU */
    RgbTriples to_rgb_triples(const Tile& tile = Tile{0, 0, 0}) {
        osmt_tile_job job = make_job(tile, 0, 0);
        osmt_batch b = make_batch(&job, 1, ops_, rings_, points_, dashes_);
        const size_t dim = dimension();
        std::vector<uint8_t> rgb(dim * dim * 3); /* the reference's triples, packed (std::tuple's own layout is not) */
        const uint32_t off[2] = {0u, (uint32_t)labels_.size()};
        if (!label_glyphs_.empty()) { /* texts recorded as glyph runs (Rasterizer::draw_glyph): expanded on the GPU */
            if (!label_segs_.empty()) throw Error(OSMT_UNSUPPORTED, "a tile's texts are either draw_line calls or glyph runs, not both");
            osmt_glyph_label_batch gb{labels_.data(), labels_.size(), off, label_glyphs_.data(), label_glyphs_.size()};
            check(osmt_render_batch_rgb_glyphs(ctx_->raw(), &b, &gb, rgb.data(), rgb.size()));
        } else {
            osmt_label_batch lb{labels_.data(), labels_.size(), off, label_segs_.data(), label_segs_.size() / 4};
            check(osmt_render_batch_rgb(ctx_->raw(), &b, labels_.empty() ? nullptr : &lb, rgb.data(), rgb.size()));
        }
        RgbTriples out(dim * dim);
        for (size_t i = 0; i < dim * dim; ++i) out[i] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        return out;
    }

  private:
    friend class TileBatch;
    friend class Rasterizer;
    friend bool draw_icon(uint32_t, double, double, TilePixels&);
    friend void fill_contour(const PointPairs&, const Filler&, double, TilePixels&);
    friend void draw_lines(const PointPairs&, double, const Color&, double, const std::optional<std::vector<double>>&,
                           const std::optional<LineCap>&, bool, TilePixels&);

    /* PointPairIter -> rings: consecutive pairs that chain (p2 == next p1) form one ring, which
     * is how point_pairs.rs:11-41 produces them; a break starts the next ring of a multipolygon. */
    std::pair<uint32_t, uint32_t> add_rings(const PointPairs& pairs) {
        const uint32_t first_ring = (uint32_t)rings_.size();
        size_t i = 0;
        while (i < pairs.size()) {
            osmt_ring r{(uint32_t)(points_.size() / 2), 0};
            points_.push_back(pairs[i].first.x);
            points_.push_back(pairs[i].first.y);
            size_t j = i;
            for (;;) {
                points_.push_back(pairs[j].second.x);
                points_.push_back(pairs[j].second.y);
                if (j + 1 < pairs.size() && pairs[j + 1].first.x == pairs[j].second.x &&
                    pairs[j + 1].first.y == pairs[j].second.y)
                    ++j;
                else
                    break;
            }
            r.n_pts = (uint32_t)(j - i + 2);
            rings_.push_back(r);
            i = j + 1;
        }
        return {first_ring, (uint32_t)rings_.size() - first_ring};
    }
    void push(const osmt_op& op) {
        ops_.push_back(op);
        pending_op_ = true;
    }
    osmt_tile_job make_job(const Tile& t, uint32_t op_off, uint32_t pt_off) const {
        osmt_tile_job j{};
        j.x = t.x;
        j.y = t.y;
        j.zoom = t.zoom;
        j.has_canvas = canvas_ ? 1 : 0;
        if (canvas_) {
            j.canvas_rgb[0] = canvas_->r;
            j.canvas_rgb[1] = canvas_->g;
            j.canvas_rgb[2] = canvas_->b;
        }
        j.n_ops = (uint32_t)ops_.size();
        j.op_off = op_off;
        j.n_pts = (uint32_t)(points_.size() / 2);
        j.pt_off = pt_off;
        return j;
    }
    osmt_batch make_batch(const osmt_tile_job* jobs, size_t n_jobs, const std::vector<osmt_op>& ops,
                          const std::vector<osmt_ring>& rings, const std::vector<int32_t>& pts,
                          const std::vector<double>& dashes) const {
        osmt_batch b{};
        b.jobs = jobs;
        b.n_jobs = n_jobs;
        b.ops = ops.data();
        b.n_ops = ops.size();
        b.rings = rings.data();
        b.n_rings = rings.size();
        b.coord_kind = OSMT_COORD_POINT_I32;
        b.scale = (uint32_t)scale_;
        b.points = pts.data();
        b.n_pts = pts.size() / 2;
        b.dashes = dashes.data();
        b.n_dashes = dashes.size();
        return b;
    }

    Context* ctx_;
    size_t scale_;
    std::optional<Color> canvas_;
    std::vector<osmt_op> ops_;
    std::vector<osmt_ring> rings_;
    std::vector<int32_t> points_;
    std::vector<double> dashes_;
    bool pending_op_ = false;
    std::vector<osmt_label> labels_;
    std::vector<double> label_segs_; /* x0, y0, x1, y1 per Rasterizer::draw_line call */
    std::vector<osmt_glyph_instance> label_glyphs_; /* per Rasterizer::draw_glyph call */
    osmt_label pending_label_{};
};

/* Labeler::draw_icon (labeler.rs:91-106): the icon of the label being built, centred at
 * get_label_position.  Always true here: collisions are resolved on the GPU, in label order. */
inline bool draw_icon(uint32_t image_id, double center_x, double center_y, TilePixels& pixels) {
    pixels.pending_label_.has_icon = 1;
    pixels.pending_label_.image_id = image_id;
    pixels.pending_label_.icon_center_x = center_x;
    pixels.pending_label_.icon_center_y = center_y;
    return true;
}

/* font/rasterizer.rs: the glyph walk of TextPlacer::place calls draw_line / draw_quad exactly as in the
 * reference; the calls are recorded (curves flattened here, with the same libm hypot) and replayed on
 * the GPU, which owns the exact-area accumulation and save_to_figure's pixel loop. */
class Rasterizer {
  public:
    explicit Rasterizer(const Color& color) : color_(color) {}
    /* :27-88 */
    void draw_line(double x0, double y0, double x1, double y1) {
        segs_.push_back(x0);
        segs_.push_back(y0);
        segs_.push_back(x1);
        segs_.push_back(y1);
    }
    /* :90-113 */
    void draw_quad(double x0, double y0, double x1, double y1, double x2, double y2) {
        auto dist_between = [](double xa, double ya, double xb, double yb) { return std::hypot(std::fabs(xa - xb), std::fabs(ya - yb)); };
        const double d01 = dist_between(x0, y0, x1, y1);
        const double d12 = dist_between(x1, y1, x2, y2);
        const double d02 = dist_between(x0, y0, x2, y2);
        if ((d01 + d12) <= 1.0001 * d02) {
            draw_line(x0, y0, x2, y2);
            return;
        }
        auto midpoint = [](double c1, double c2) { return (c1 + c2) / 2.0; };
        const double m01_x = midpoint(x0, x1), m01_y = midpoint(y0, y1);
        const double m12_x = midpoint(x1, x2), m12_y = midpoint(y1, y2);
        const double m012_x = midpoint(m01_x, m12_x), m012_y = midpoint(m01_y, m12_y);
        draw_quad(x0, y0, m01_x, m01_y, m012_x, m012_y);
        draw_quad(m012_x, m012_y, m12_x, m12_y, x2, y2);
    }
    /* Glyph::rasterize (font/text_placer.rs:232-259) recorded as one glyph instance instead of its draw_line /
     * draw_quad calls: the GPU walks the outline (osmt_scene_set_glyph_labels).  glyph_id from osmt_register_glyphs,
     * scale = f64::from(scale_for_pixel_height(..)), form OSMT_GLYPH_CENTER with params {x_offset, baseline} or
     * OSMT_GLYPH_LINE with {glyph_center_x, glyph_center_y, angle_sin, angle_cos, way_x, way_y}.  A text is either
     * draw_line calls or glyph instances.  Only TilePixels::to_rgb_triples renders glyph-run texts so far: TileBatch
     * (and its PNG call) refuses a tile that holds one with OSMT_UNSUPPORTED. */
    void draw_glyph(uint32_t glyph_id, double scale, uint32_t form, const double* params) {
        osmt_glyph_instance g{};
        g.glyph_id = glyph_id;
        g.form = form;
        g.scale = scale;
        for (int k = 0; k < (form == OSMT_GLYPH_LINE ? 6 : 2); ++k) g.p[k] = params[k];
        glyphs_.push_back(g);
    }
    /* :115-147: hands the text of the label being built to the canvas.  Always true (see draw_icon). */
    bool save_to_figure(TilePixels& pixels) const {
        osmt_label& l = pixels.pending_label_;
        l.has_text = 1;
        l.text_color[0] = color_.r;
        l.text_color[1] = color_.g;
        l.text_color[2] = color_.b;
        if (!glyphs_.empty()) {
            if (!segs_.empty()) throw Error(OSMT_UNSUPPORTED, "a text is either draw_line calls or glyph runs, not both");
            l.seg_off = (uint32_t)pixels.label_glyphs_.size();
            l.n_segs = (uint32_t)glyphs_.size();
            pixels.label_glyphs_.insert(pixels.label_glyphs_.end(), glyphs_.begin(), glyphs_.end());
            return true;
        }
        l.seg_off = (uint32_t)(pixels.label_segs_.size() / 4);
        l.n_segs = (uint32_t)(segs_.size() / 4);
        pixels.label_segs_.insert(pixels.label_segs_.end(), segs_.begin(), segs_.end());
        return true;
    }

  private:
    Color color_;
    std::vector<double> segs_;
    std::vector<osmt_glyph_instance> glyphs_;
};

/* fill.rs:16 */
inline void fill_contour(const PointPairs& points, const Filler& filler, double opacity, TilePixels& pixels) {
    osmt_op op{};
    op.kind = filler.kind == Filler::ColorFill ? OSMT_OP_FILL_COLOR : OSMT_OP_FILL_IMAGE;
    op.color[0] = filler.color.r;
    op.color[1] = filler.color.g;
    op.color[2] = filler.color.b;
    op.opacity = opacity;
    op.image_id = filler.image_id;
    auto [off, n] = pixels.add_rings(points);
    op.ring_off = off;
    op.n_rings = n;
    pixels.push(op);
}

/* line.rs:9-18.  `width` and `dashes` arrive already multiplied by scale, as in drawer.rs:191,206,171. */
inline void draw_lines(const PointPairs& points, double width, const Color& color, double opacity,
                       const std::optional<std::vector<double>>& dashes, const std::optional<LineCap>& line_cap,
                       bool use_caps_for_dashes, TilePixels& pixels) {
    osmt_op op{};
    op.kind = OSMT_OP_STROKE;
    op.cap = !line_cap ? OSMT_CAP_NONE
             : *line_cap == LineCap::Butt  ? OSMT_CAP_BUTT
             : *line_cap == LineCap::Round ? OSMT_CAP_ROUND
                                           : OSMT_CAP_SQUARE;
    op.use_caps_for_dashes = use_caps_for_dashes ? 1 : 0;
    op.color[0] = color.r;
    op.color[1] = color.g;
    op.color[2] = color.b;
    op.opacity = opacity;
    op.width = width;
    if (dashes) {
        op.has_dashes = 1;
        op.n_dashes = (uint32_t)dashes->size();
        op.dashes_off = (uint32_t)pixels.dashes_.size();
        pixels.dashes_.insert(pixels.dashes_.end(), dashes->begin(), dashes->end());
    }
    auto [off, n] = pixels.add_rings(points);
    op.ring_off = off;
    op.n_rings = n;
    pixels.push(op);
}

/* Several recorded tiles -> ONE osmt_render_batch call (the GPU fast path the single-tile
 * server loop of http_server.rs:162-171 would grow into). */
class TileBatch {
  public:
    explicit TileBatch(Context& ctx, size_t scale) : ctx_(&ctx), scale_(scale) {}
    void add(const Tile& tile, const TilePixels& px) {
        /* the batch entries take draw_line calls only: a glyph-run label's seg_off / n_segs name glyph instances and
         * would be read as another label's calls */
        if (!px.label_glyphs_.empty()) throw Error(OSMT_UNSUPPORTED, "TileBatch takes no glyph-run texts (Rasterizer::draw_glyph) yet");
        const uint32_t op_off = (uint32_t)ops_.size(), pt_off = (uint32_t)(points_.size() / 2);
        const uint32_t ring_off = (uint32_t)rings_.size(), dash_off = (uint32_t)dashes_.size();
        jobs_.push_back(px.make_job(tile, op_off, pt_off));
        for (osmt_op op : px.ops_) {
            op.ring_off += ring_off;
            if (op.n_dashes) op.dashes_off += dash_off;
            ops_.push_back(op);
        }
        for (osmt_ring r : px.rings_) {
            r.first_pt += pt_off;
            rings_.push_back(r);
        }
        points_.insert(points_.end(), px.points_.begin(), px.points_.end());
        dashes_.insert(dashes_.end(), px.dashes_.begin(), px.dashes_.end());
        const uint32_t seg_off = (uint32_t)(label_segs_.size() / 4);
        for (osmt_label l : px.labels_) {
            if (l.n_segs) l.seg_off += seg_off;
            labels_.push_back(l);
        }
        label_segs_.insert(label_segs_.end(), px.label_segs_.begin(), px.label_segs_.end());
        label_off_.push_back((uint32_t)labels_.size());
    }
    std::vector<TileRenderedPixels> render() {
        const size_t dim = TILE_SIZE * scale_;
        std::vector<uint8_t> rgb(jobs_.size() * dim * dim * 3);
        osmt_batch b{};
        b.jobs = jobs_.data();
        b.n_jobs = jobs_.size();
        b.ops = ops_.data();
        b.n_ops = ops_.size();
        b.rings = rings_.data();
        b.n_rings = rings_.size();
        b.coord_kind = OSMT_COORD_POINT_I32;
        b.scale = (uint32_t)scale_;
        b.points = points_.data();
        b.n_pts = points_.size() / 2;
        b.dashes = dashes_.data();
        b.n_dashes = dashes_.size();
        osmt_label_batch lb{labels_.data(), labels_.size(), label_off_.data(), label_segs_.data(), label_segs_.size() / 4};
        check(osmt_render_batch_rgb(ctx_->raw(), &b, labels_.empty() ? nullptr : &lb, rgb.data(), dim * dim * 3));
        std::vector<TileRenderedPixels> out(jobs_.size());
        for (size_t t = 0; t < jobs_.size(); ++t) {
            out[t].dimension = dim;
            out[t].triples.resize(dim * dim);
            const uint8_t* p = rgb.data() + t * dim * dim * 3;
            for (size_t i = 0; i < dim * dim; ++i) out[t].triples[i] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        }
        return out;
    }

    /* Drawer::draw_tile for every added tile (drawer.rs:40-58): finished RGB8 PNG files, written by the GPU */
    std::vector<std::vector<uint8_t>> render_png() {
        const size_t dim = TILE_SIZE * scale_;
        osmt_batch b{};
        b.jobs = jobs_.data();
        b.n_jobs = jobs_.size();
        b.ops = ops_.data();
        b.n_ops = ops_.size();
        b.rings = rings_.data();
        b.n_rings = rings_.size();
        b.coord_kind = OSMT_COORD_POINT_I32;
        b.scale = (uint32_t)scale_;
        b.points = points_.data();
        b.n_pts = points_.size() / 2;
        b.dashes = dashes_.data();
        b.n_dashes = dashes_.size();
        osmt_label_batch lb{labels_.data(), labels_.size(), label_off_.data(), label_segs_.data(), label_segs_.size() / 4};
        std::vector<uint8_t> blob(jobs_.size() * osmt_png_device_bound((uint32_t)dim, (uint32_t)dim));
        std::vector<uint64_t> off(jobs_.size() + 1);
        check(osmt_render_batch_png(ctx_->raw(), &b, labels_.empty() ? nullptr : &lb, blob.data(), blob.size(), off.data()));
        std::vector<std::vector<uint8_t>> out(jobs_.size());
        for (size_t t = 0; t < jobs_.size(); ++t) out[t].assign(blob.begin() + (long)off[t], blob.begin() + (long)off[t + 1]);
        return out;
    }

  private:
    Context* ctx_;
    size_t scale_;
    std::vector<osmt_tile_job> jobs_;
    std::vector<osmt_op> ops_;
    std::vector<osmt_ring> rings_;
    std::vector<int32_t> points_;
    std::vector<double> dashes_;
    std::vector<osmt_label> labels_;
    std::vector<double> label_segs_;
    std::vector<uint32_t> label_off_{0u};
};

}  // namespace osmt
#endif
