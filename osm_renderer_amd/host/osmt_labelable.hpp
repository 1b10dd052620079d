/*
 * osmt_labelable.hpp — where a polygon's label goes: a scalar C++ statement of what the reference's
 * Labelable::get_label_position computes for ways and multipolygons (src/draw/labelable.rs:191-204 with filter_polygons,
 * :206-232, and the "polylabel" search, :125-189 — a pole of inaccessibility weighted towards the centroid).
 *
 * Three users: the CPU half of the tests, the CPU side of tools/bench_polylabel.py, and osmt::LabelPositions below — the
 * collector a host uses to batch the calls of one or many tiles for osmt_label_positions and to compute on the CPU the
 * requests the device declines (OSMT_LABEL_TOO_LARGE).  The device kernels (csrc/osmt_polylabel.hip) return the same bits.
 *
 * Every f64 expression keeps the reference's association; compile with -ffp-contract=off.
 *
 * What the reference leaves to its compiler and this file pins down:
 *   - f64::min / f64::max over a ring's coordinates: written here as `p < m ? p : m` in point order, so that of two zeros
 *     of different sign the FIRST one met stays.  It shows only in the (min_x, min_y) returned for a ring of zero width or
 *     height whose minimum is a zero of both signs.
 *   - the tie order of equal max_fitness keys: std::collections::BinaryHeap's, restated in label_heap below.
 */
#ifndef OSMT_LABELABLE_HPP
#define OSMT_LABELABLE_HPP

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/osmtile.h"

namespace osmt {

/* what a search did, for the tests and the caps: the device answers a request exactly when both stay <= OSMT_LABEL_MAX_CELLS */
struct LabelSearchStats {
    uint64_t queue_peak = 0; /* most cells in the queue at once */
    uint64_t pops = 0;       /* cells taken from the queue */
    uint64_t nan_to_min = 0; /* OSMT_LABELABLE_DEBUG: NaNs that reached the distance minimum or a queue key (must stay 0) */
};

namespace labelable_detail {

struct cell {
    double cx, cy, half, fitness, max_fitness;
};

/* std::collections::BinaryHeap<Cell> (Rust std 1.70 .. 1.80, library/alloc/src/collections/binary_heap/mod.rs) with the
 * reference's Ord: cells compare by max_fitness alone, an unordered pair counts as equal (labelable.rs:99-119).
 * `a <= b` of the std source is therefore !(a.max_fitness > b.max_fitness). */
struct label_heap {
    std::vector<cell> d;
    static bool le(const cell& a, const cell& b) { return !(a.max_fitness > b.max_fitness); }
    /* sift_up(start, pos): the element climbs while it is NOT <= its parent */
    void sift_up(size_t start, size_t pos) {
        const cell e = d[pos];
        while (pos > start) {
            const size_t parent = (pos - 1) / 2;
            if (le(e, d[parent])) break;
            d[pos] = d[parent];
            pos = parent;
        }
        d[pos] = e;
    }
    void push(const cell& c) {
        d.push_back(c);
        sift_up(0, d.size() - 1);
    }
    /* pop: the last element goes to the root, the hole walks to the bottom taking the RIGHT child when left <= right, a lone
     * last child is taken too, then the element sifts up from there (sift_down_to_bottom) */
    cell pop() {
        cell item = d.back();
        d.pop_back();
        if (!d.empty()) {
            std::swap(item, d[0]);
            const size_t end = d.size();
            const cell e = d[0];
            size_t pos = 0, child = 1;
            while (child + 1 < end) { /* child <= end.saturating_sub(2) */
                child += le(d[child], d[child + 1]) ? 1 : 0;
                d[pos] = d[child];
                pos = child;
                child = 2 * pos + 1;
            }
            if (child + 1 == end) {
                d[pos] = d[child];
                pos = child;
            }
            d[pos] = e;
            sift_up(0, pos);
        }
        return item;
    }
};

struct ring_view {
    const double* p; /* [n][2] */
    uint32_t n;
};

inline double segment_dist_sq(double px, double py, double sx, double sy, double ex, double ey) {
    double x = sx, y = sy;
    double dx = ex - x, dy = ey - y;
    if (dx != 0.0 || dy != 0.0) {
        /* may be NaN or infinite when dx*dx + dy*dy underflows to 0: both comparisons then decide as IEEE says */
        const double t = ((px - x) * dx + (py - y) * dy) / (dx * dx + dy * dy);
        if (t > 1.0) {
            x = ex;
            y = ey;
        } else if (t > 0.0) {
            x += dx * t;
            y += dy * t;
        }
    }
    dx = px - x;
    dy = py - y;
    return dx * dx + dy * dy;
}

/* signed distance of (px, py) to the rings: positive inside (even-odd over all edges), edge i = (a = P[i], b = P[i - 1]) */
inline double point_to_rings_dist(double px, double py, const ring_view* rings, size_t n_rings, LabelSearchStats* st) {
    bool inside = false;
    double min_sq = std::numeric_limits<double>::infinity();
    for (size_t r = 0; r < n_rings; ++r) {
        const double* p = rings[r].p;
        for (uint32_t i = 1; i < rings[r].n; ++i) {
            const double ax = p[2 * i], ay = p[2 * i + 1], bx = p[2 * i - 2], by = p[2 * i - 1];
            if ((ay > py) != (by > py) && (px < (bx - ax) * (py - ay) / (by - ay) + ax)) inside = !inside;
            const double d = segment_dist_sq(px, py, ax, ay, bx, by);
#ifdef OSMT_LABELABLE_DEBUG
            if (d != d && st) ++st->nan_to_min;
#endif
            min_sq = d < min_sq ? d : min_sq; /* f64::min over non-NaN values */
        }
    }
    (void)st;
    return (inside ? 1.0 : -1.0) * std::sqrt(min_sq);
}

inline double ring_area(const ring_view& r) {
    double s = 0.0;
    for (uint32_t i = 1; i < r.n; ++i) s += r.p[2 * i] * r.p[2 * i - 1] - r.p[2 * i - 2] * r.p[2 * i + 1];
    return std::fabs(s);
}

}  // namespace labelable_detail

struct LabelPosition {
    uint32_t status; /* OSMT_LABEL_OK / _NONE / _TOO_LARGE */
    double x, y;
};

/* get_label_position over `n_rings` rings (a way: one; a multipolygon: polygon_count() in file order) of already projected
 * and scaled points.  capped: give up with OSMT_LABEL_TOO_LARGE exactly where the device does (the queue would hold more
 * than OSMT_LABEL_MAX_CELLS cells, or more than OSMT_LABEL_MAX_CELLS cells would be popped); uncapped it is the reference's
 * function.  Ring i has n_pts[i] points at pts[i]. */
inline LabelPosition get_label_position(const double* const* pts, const uint32_t* n_pts, size_t n_rings, double scale, bool capped = false,
                                        LabelSearchStats* stats = nullptr) {
    using namespace labelable_detail;
    LabelSearchStats local;
    LabelSearchStats& st = stats ? *stats : local;
    st = LabelSearchStats();
    if (n_rings == 0 || n_pts[0] == 0) return {OSMT_LABEL_NONE, 0.0, 0.0};

    /* filter_polygons: the first ring of the largest area leads; a later ring stays when none of its points is outside it */
    std::vector<ring_view> rings(n_rings);
    for (size_t i = 0; i < n_rings; ++i) rings[i] = {pts[i], n_pts[i]};
    size_t largest = 0;
    double largest_area = ring_area(rings[0]);
    for (size_t i = 1; i < n_rings; ++i) {
        const double a = ring_area(rings[i]);
        if (a > largest_area) {
            largest = i;
            largest_area = a;
        }
    }
    std::swap(rings[0], rings[largest]);
    size_t good = 1;
    for (size_t i = 1; i < n_rings; ++i) {
        bool all = true;
        for (uint32_t k = 0; k < rings[i].n && all; ++k)
            all = point_to_rings_dist(rings[i].p[2 * k], rings[i].p[2 * k + 1], rings.data(), 1, &st) >= 0.0;
        if (all) std::swap(rings[i], rings[good++]);
    }
    rings.resize(good);

    const ring_view& r0 = rings[0];
    const double inf = std::numeric_limits<double>::infinity();
    double min_x = inf, max_x = -inf, min_y = inf, max_y = -inf;
    for (uint32_t i = 0; i < r0.n; ++i) {
        const double x = r0.p[2 * i], y = r0.p[2 * i + 1];
        min_x = x < min_x ? x : min_x;
        max_x = x > max_x ? x : max_x;
        min_y = y < min_y ? y : min_y;
        max_y = y > max_y ? y : max_y;
    }
    const double w = max_x - min_x, h = max_y - min_y;
    const double precision = (w > h ? w : h) / 100.0 * scale;

    const double cell_size = w < h ? w : h;
    const double max_size = w > h ? w : h;
    if (cell_size == 0.0) return {OSMT_LABEL_OK, min_x, min_y};

    /* get_centroid: running sums in edge order */
    double area = 0.0, sx = 0.0, sy = 0.0;
    for (uint32_t i = 1; i < r0.n; ++i) {
        const double ax = r0.p[2 * i], ay = r0.p[2 * i + 1], bx = r0.p[2 * i - 2], by = r0.p[2 * i - 1];
        const double c = ax * by - bx * ay;
        sx += (ax + bx) * c;
        sy += (ay + by) * c;
        area += c * 3.0;
    }
    const double cen_x = area == 0.0 ? r0.p[0] : sx / area;
    const double cen_y = area == 0.0 ? r0.p[1] : sy / area;

    auto fitness = [&](double cx, double cy, double d) {
        if (d <= 0.0) return d;
        const double dx = cx - cen_x, dy = cy - cen_y;
        return d * (1.0 - std::sqrt(dx * dx + dy * dy) / max_size);
    };
    auto make_cell = [&](double cx, double cy, double half) {
        const double d = point_to_rings_dist(cx, cy, rings.data(), rings.size(), &st);
        const double dmax = d + half * 1.4142135623730951 /* std::f64::consts::SQRT_2 */;
        cell c{cx, cy, half, fitness(cx, cy, d), fitness(cx, cy, dmax)};
#ifdef OSMT_LABELABLE_DEBUG
        if (c.max_fitness != c.max_fitness || c.fitness != c.fitness) ++st.nan_to_min;
#endif
        return c;
    };

    label_heap heap;
    auto push = [&](const cell& c) {
        if (capped && heap.d.size() >= OSMT_LABEL_MAX_CELLS) return false;
        heap.push(c);
        if (heap.d.size() > st.queue_peak) st.queue_peak = heap.d.size();
        return true;
    };
    double half = cell_size / 2.0;
    for (double x = min_x; x < max_x; x += cell_size)
        for (double y = min_y; y < max_y; y += cell_size)
            if (!push(make_cell(x + half, y + half, half))) return {OSMT_LABEL_TOO_LARGE, 0.0, 0.0};

    cell best = make_cell(cen_x, cen_y, 0.0);
    while (!heap.d.empty()) {
        if (capped && st.pops >= OSMT_LABEL_MAX_CELLS) return {OSMT_LABEL_TOO_LARGE, 0.0, 0.0};
        const cell cur = heap.pop();
        ++st.pops;
        if (cur.fitness > best.fitness) best = cur;
        if (cur.max_fitness - best.fitness <= precision) continue;
        half = cur.half / 2.0;
        for (int ix = 0; ix < 2; ++ix)
            for (int iy = 0; iy < 2; ++iy) {
                const double dx = ix ? 1.0 : -1.0, dy = iy ? 1.0 : -1.0;
                if (!push(make_cell(cur.cx + dx * half, cur.cy + dy * half, half))) return {OSMT_LABEL_TOO_LARGE, 0.0, 0.0};
            }
    }
    return {OSMT_LABEL_OK, best.cx, best.cy};
}

using LabelRing = std::vector<std::array<double, 2>>;

inline LabelPosition get_label_position(const std::vector<LabelRing>& polygons, double scale, bool capped = false,
                                        LabelSearchStats* stats = nullptr) {
    std::vector<const double*> p(polygons.size());
    std::vector<uint32_t> n(polygons.size());
    for (size_t i = 0; i < polygons.size(); ++i) {
        p[i] = polygons[i].empty() ? nullptr : polygons[i][0].data();
        n[i] = (uint32_t)polygons[i].size();
    }
    return get_label_position(p.data(), n.data(), polygons.size(), scale, capped, stats);
}

/* The label positions of many polygons in one device call.  The two call sites of the reference — the icon of
 * Labeler::label_entity (labeler.rs:56) and the centred text of TextPlacer::place (text_placer.rs:113) — each become one
 * add_way / add_multipolygon while the host walks a tile's (or a batch of tiles') labelled areas; run() answers all of them:
 * on the GPU through osmt_label_positions, and on this thread for the requests the device declines as too large, so the
 * caller always gets the reference's answer.  Points are what nodes_to_points produces (labelable.rs:61-68):
 * coords_to_xy_tile_relative(node, tile) * scale, unrounded. */
class LabelPositions {
   public:
    /* returns the request's index into run()'s result */
    size_t add_way(const LabelRing& ring, double scale) { return add_multipolygon(&ring, 1, scale); }
    size_t add_multipolygon(const std::vector<LabelRing>& rings, double scale) { return add_multipolygon(rings.data(), rings.size(), scale); }
    size_t add_multipolygon(const LabelRing* rings, size_t n, double scale) {
        osmt_label_request rq{};
        rq.ring_off = (uint32_t)rings_.size();
        rq.n_rings = (uint32_t)n;
        rq.scale = scale;
        for (size_t i = 0; i < n; ++i) {
            rings_.push_back({(uint32_t)(pts_.size() / 2), (uint32_t)rings[i].size()});
            for (const auto& p : rings[i]) {
                pts_.push_back(p[0]);
                pts_.push_back(p[1]);
            }
        }
        reqs_.push_back(rq);
        return reqs_.size() - 1;
    }
    size_t size() const { return reqs_.size(); }
    size_t cpu_fallbacks() const { return fallbacks_; } /* requests of the last run() computed on the host */
    void clear() {
        rings_.clear();
        pts_.clear();
        reqs_.clear();
    }
    /* status is OSMT_LABEL_OK or OSMT_LABEL_NONE for every request; throws std::runtime_error on an ABI error */
    std::vector<osmt_label_position> run(osmt_ctx* ctx) {
        std::vector<osmt_label_position> out(reqs_.size());
        osmt_label_request_batch b{};
        b.requests = reqs_.data();
        b.n_requests = reqs_.size();
        b.rings = rings_.data();
        b.n_rings = rings_.size();
        b.points = pts_.data();
        b.n_pts = pts_.size() / 2;
        const int rc = osmt_label_positions(ctx, &b, out.data());
        if (rc != OSMT_OK) throw std::runtime_error(std::string("osmt_label_positions: ") + osmt_last_error());
        fallbacks_ = 0;
        for (size_t i = 0; i < out.size(); ++i) {
            if (out[i].status != OSMT_LABEL_TOO_LARGE) continue;
            const osmt_label_request& rq = reqs_[i];
            std::vector<const double*> p(rq.n_rings);
            std::vector<uint32_t> n(rq.n_rings);
            for (uint32_t k = 0; k < rq.n_rings; ++k) {
                p[k] = pts_.data() + 2 * (size_t)rings_[rq.ring_off + k].first_pt;
                n[k] = rings_[rq.ring_off + k].n_pts;
            }
            const LabelPosition r = get_label_position(p.data(), n.data(), rq.n_rings, rq.scale);
            out[i].x = r.x;
            out[i].y = r.y;
            out[i].status = r.status;
            ++fallbacks_;
        }
        return out;
    }

   private:
    std::vector<osmt_ring> rings_;
    std::vector<double> pts_;
    std::vector<osmt_label_request> reqs_;
    size_t fallbacks_ = 0;
};

/* ---- anchors from tile coordinates (osmt_label_positions_tiles) ----------------------------------------------------- */
/* coords_to_xy_tile_relative(node, tile) * scale from the node's registered Mercator factors f[2] (osmt::mercator_factors,
 * host/osmt_geodata.hpp): what is left of tile.rs:94-106 and labelable.rs:64-65 once the libm step is in the factor — a
 * multiplication by a power of two, a subtraction, a multiplication, each a statement of its own (-ffp-contract=off).  The
 * tile offset is formed in u32 as the reference's `tile.x * TILE_SIZE`.  csrc/osmt_anchors.hip runs the same three operations. */
inline std::array<double, 2> project_factors(const double* f, const osmt_query_tile& tile, uint32_t scale) {
    const double dim = (double)(OSMT_TILE_SIZE * (1u << tile.zoom));
    const double s = (double)scale;
    const double off_x = (double)(uint32_t)(tile.x * OSMT_TILE_SIZE), off_y = (double)(uint32_t)(tile.y * OSMT_TILE_SIZE);
    double x = f[0] * dim, y = f[1] * dim;
    x = x - off_x;
    y = y - off_y;
    x = x * s;
    y = y * s;
    return {x, y};
}

/* The polygons get_label_position is given for `entity` (a way's local id, or a multipolygon's | OSMT_STYLED_MULTIPOLYGON)
 * under `tile`: a way is one ring of its nodes, a multipolygon ALL its polygons in file order, the empty and the one-node
 * ones included (labelable.rs:26-59).  factors: [n_nodes][2].  Throws std::out_of_range for an id the geodata does not have. */
inline std::vector<LabelRing> label_rings_of(const osmt_geodata_desc& g, const double* factors, uint32_t entity, const osmt_query_tile& tile,
                                             uint32_t scale) {
    const uint32_t id = entity & ~OSMT_STYLED_MULTIPOLYGON;
    auto ring_of = [&](const uint32_t* nodes, uint32_t n) {
        LabelRing r(n);
        for (uint32_t i = 0; i < n; ++i) r[i] = project_factors(factors + 2 * (size_t)nodes[i], tile, scale);
        return r;
    };
    std::vector<LabelRing> rings;
    if (entity & OSMT_STYLED_MULTIPOLYGON) {
        if (id >= g.n_multipolygons) throw std::out_of_range("label_rings_of: multipolygon id out of range");
        for (uint32_t k = g.multipolygon_polygon_off[id]; k < g.multipolygon_polygon_off[id + 1]; ++k) {
            const uint32_t p = g.multipolygon_polygons[k];
            rings.push_back(ring_of(g.polygon_nodes + g.polygon_node_off[p], g.polygon_node_off[p + 1] - g.polygon_node_off[p]));
        }
    } else {
        if (id >= g.n_ways) throw std::out_of_range("label_rings_of: way id out of range");
        rings.push_back(ring_of(g.way_nodes + g.way_node_off[id], g.way_node_off[id + 1] - g.way_node_off[id]));
    }
    return rings;
}

/* The twin of LabelPositions for callers that registered a geodata file and its Mercator factors: a request is an entity
 * and a tile (8 bytes go to the device), run() answers all of them through osmt_label_positions_tiles and computes on this
 * thread, from the same factors, the requests the device declines as too large.  `geodata` and `factors` are the arrays that
 * were registered under `geodata_id`; they must outlive this object. */
class TileLabelPositions {
   public:
    TileLabelPositions(const osmt_geodata_desc& geodata, const double* factors, uint32_t geodata_id, uint32_t scale)
        : g_(geodata), f_(factors), id_(geodata_id), scale_(scale) {}
    /* returns the tile's index for add() */
    uint32_t add_tile(uint8_t zoom, uint32_t x, uint32_t y) {
        osmt_query_tile t{};
        t.x = x, t.y = y, t.zoom = zoom;
        tiles_.push_back(t);
        return (uint32_t)(tiles_.size() - 1);
    }
    /* returns the request's index into run()'s result */
    size_t add_way(uint32_t way, uint32_t tile) { return add(way, tile); }
    size_t add_multipolygon(uint32_t mp, uint32_t tile) { return add(mp | OSMT_STYLED_MULTIPOLYGON, tile); }
    size_t size() const { return reqs_.size(); }
    size_t cpu_fallbacks() const { return fallbacks_; } /* requests of the last run() computed on the host */
    void clear() {
        tiles_.clear();
        reqs_.clear();
    }
    /* status is OSMT_LABEL_OK or OSMT_LABEL_NONE for every request; throws std::runtime_error on an ABI error */
    std::vector<osmt_label_position> run(osmt_ctx* ctx) {
        std::vector<osmt_label_position> out(reqs_.size());
        osmt_label_tile_batch b{};
        b.requests = reqs_.data();
        b.n_requests = reqs_.size();
        b.tiles = tiles_.data();
        b.n_tiles = tiles_.size();
        b.geodata_id = id_;
        b.scale = scale_;
        const int rc = osmt_label_positions_tiles(ctx, &b, out.data());
        if (rc != OSMT_OK) throw std::runtime_error(std::string("osmt_label_positions_tiles: ") + osmt_last_error());
        fallbacks_ = 0;
        for (size_t i = 0; i < out.size(); ++i) {
            if (out[i].status != OSMT_LABEL_TOO_LARGE) continue;
            const LabelPosition r = get_label_position(label_rings_of(g_, f_, reqs_[i].entity, tiles_[reqs_[i].tile], scale_), (double)scale_);
            out[i].x = r.x;
            out[i].y = r.y;
            out[i].status = r.status;
            ++fallbacks_;
        }
        return out;
    }

   private:
    size_t add(uint32_t entity, uint32_t tile) {
        reqs_.push_back(osmt_label_tile_request{entity, tile});
        return reqs_.size() - 1;
    }
    const osmt_geodata_desc& g_;
    const double* f_;
    uint32_t id_, scale_;
    std::vector<osmt_query_tile> tiles_;
    std::vector<osmt_label_tile_request> reqs_;
    size_t fallbacks_ = 0;
};

}  // namespace osmt
#endif
