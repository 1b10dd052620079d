/*
 * osmt_textplacer.hpp — where the glyphs of a label's text go: a scalar C++ statement of what the reference's
 * TextPlacer::place computes between text_to_glyphs and Glyph::rasterize (src/draw/font/text_placer.rs:24-168 with
 * compute_way_position, :270-296): text runs (osmt_text_label_batch) in, glyph instances (osmt_glyph_instance) out.
 *
 * Three users: the CPU half of the tests (tests/text_shim.cpp), an integrator without a device, and the library itself,
 * which runs validate_text_labels below before every upload.  The device kernel (csrc/osmt_textplace.hip) returns the
 * same bits.
 *
 * Every f64 expression keeps the reference's association and every sum its order; compile with -ffp-contract=off.
 * atan2 and sin_cos are not here: the caller's libm computes (-get_angle(points, e)).sin_cos() per edge (way_sincos).
 */
#ifndef OSMT_TEXTPLACER_HPP
#define OSMT_TEXTPLACER_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/osmtile.h"

namespace osmt {

namespace textplacer_detail {

/* MAX_TEXT_WIDTH = TILE_SIZE as f64 / 8.0 (text_placer.rs:298): not scaled by global_scale */
constexpr double MAX_TEXT_WIDTH = 32.0;

/* Glyph::width of text_to_glyphs (text_placer.rs:180-189) */
inline double glyph_width(const osmt_text_glyph& g, bool first, double scale) {
    double w = (double)g.advance * scale;
    if (!first) w += (double)g.kern * scale;
    return w;
}

/* Point::dist (point.rs:21-25) */
inline double point_dist(const int32_t* a, const int32_t* b) {
    const double dx = (double)(a[0] - b[0]);
    const double dy = (double)(a[1] - b[1]);
    return std::sqrt(dx * dx + dy * dy);
}

struct way_position {
    double x, y;
    uint32_t edge; /* get_angle's start_idx */
};

/* compute_way_position (text_placer.rs:270-296), n >= 2.  An advance <= 0 (or NaN) never enters the loop and returns the
 * LAST point with the last edge's angle, as running off the end does; zero-length edges never pass `seg_dist >=
 * to_travel` with to_travel > 0, so the division is safe. */
inline way_position compute_way_position(const int32_t* pts, uint32_t n, double advance_by) {
    uint32_t point_idx = 0;
    double to_travel = advance_by;
    while (to_travel > 0.0 && point_idx + 1 < n) {
        const int32_t* from = pts + 2 * (size_t)point_idx;
        const int32_t* to = from + 2;
        const double seg_dist = point_dist(from, to);
        if (seg_dist >= to_travel) {
            const double ratio = to_travel / point_dist(from, to);
            return way_position{(double)from[0] + ((double)(to[0] - from[0]) * ratio), (double)from[1] + ((double)(to[1] - from[1]) * ratio),
                                point_idx};
        }
        to_travel -= seg_dist;
        point_idx += 1;
    }
    const int32_t* last = pts + 2 * (size_t)(n - 1);
    return way_position{(double)last[0], (double)last[1], n - 2};
}

inline osmt_glyph_instance instance(uint32_t glyph_id, uint32_t form, double scale) {
    osmt_glyph_instance o{};
    o.glyph_id = glyph_id;
    o.form = form;
    o.scale = scale;
    return o;
}

}  // namespace textplacer_detail

/* TextPlacer::place for one label: g[0 .. n) are the text's glyphs, pts / sincos the run's own way (already offset by
 * pt_off; unused for OSMT_TEXT_CENTER), out[k] the instance of glyph k.  Returns false when place() returns before
 * rasterizing (every out[k].form is OSMT_GLYPH_NONE then). */
inline bool place_text(const osmt_text_run& r, const osmt_text_glyph* g, uint32_t n, const int32_t* pts, const double* sincos,
                       osmt_glyph_instance* out) {
    using namespace textplacer_detail;
    const double scale = r.scale;
    /* get_v_metrics (text_placer.rs:199-207) */
    const double descent = (double)r.descent * scale, ascent = (double)r.ascent * scale, line_gap = (double)r.line_gap * scale;
    double total_width = 0.0;
    for (uint32_t k = 0; k < n; ++k) total_width += glyph_width(g[k], k == 0, scale);
    if (r.position == OSMT_TEXT_LINE) {
        bool placed = r.n_pts >= 2;
        double total_way_length = 0.0;
        if (placed) {
            for (uint32_t e = 0; e + 1 < r.n_pts; ++e) total_way_length += point_dist(pts + 2 * (size_t)e, pts + 2 * (size_t)e + 2);
            placed = !(total_width > total_way_length);
        }
        if (!placed) {
            for (uint32_t k = 0; k < n; ++k) out[k] = instance(g[k].glyph_id, OSMT_GLYPH_NONE, scale);
            return false;
        }
        double cur_dist = (total_way_length - total_width) / 2.0;
        const double glyph_center_y = (descent + ascent) / 2.0;
        for (uint32_t k = 0; k < n; ++k) {
            const double width = glyph_width(g[k], k == 0, scale);
            const double glyph_center_x = width / 2.0;
            const way_position wp = compute_way_position(pts, r.n_pts, cur_dist + glyph_center_x);
            osmt_glyph_instance o = instance(g[k].glyph_id, OSMT_GLYPH_LINE, scale);
            o.p[0] = glyph_center_x;
            o.p[1] = glyph_center_y;
            o.p[2] = sincos[2 * (size_t)wp.edge];
            o.p[3] = sincos[2 * (size_t)wp.edge + 1];
            o.p[4] = wp.x;
            o.p[5] = wp.y;
            out[k] = o;
            cur_dist += width;
        }
        return true;
    }
    /* TextPosition::Center: rows (text_placer.rs:114-133) */
    std::vector<std::pair<uint32_t, double>> rows; /* (one past the row's last glyph, row width) */
    double current_row_width = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        const double width = glyph_width(g[k], k == 0, scale);
        current_row_width += width;
        const bool is_last_glyph = k + 1 == n;
        const bool should_break = (g[k].flags & 1u) && (current_row_width + width > MAX_TEXT_WIDTH);
        if (should_break || is_last_glyph) {
            rows.emplace_back(k + 1, current_row_width);
            current_row_width = 0.0;
        }
    }
    const double row_height = ascent - descent + line_gap;
    const double total_height = row_height * (double)rows.size();
    double cur_y = r.center_y;
    if (r.y_offset > 0)
        cur_y += (double)r.y_offset;
    else
        cur_y -= total_height / 2.0;
    uint32_t k = 0;
    for (const auto& row : rows) {
        double cur_x = r.center_x - row.second / 2.0;
        for (; k < row.first; ++k) {
            osmt_glyph_instance o = instance(g[k].glyph_id, OSMT_GLYPH_CENTER, scale);
            o.p[0] = cur_x;
            o.p[1] = cur_y + ascent;
            out[k] = o;
            cur_x += glyph_width(g[k], k == 0, scale);
        }
        cur_y += row_height;
    }
    return true;
}

/* The whole batch: out[n_glyphs], slot seg_off + k = glyph k of its label; slots no has_text label names are zero.
 * The batch must have passed validate_text_labels. */
inline void place_text_labels(const osmt_text_label_batch& b, osmt_glyph_instance* out) {
    for (size_t i = 0; i < b.n_glyphs; ++i) out[i] = osmt_glyph_instance{};
    for (size_t l = 0; l < b.n_labels; ++l) {
        const osmt_label& in = b.labels[l];
        if (!in.has_text || in.n_segs == 0) continue;
        const osmt_text_run& r = b.runs[l];
        const bool line = r.position == OSMT_TEXT_LINE && r.n_pts > 0;
        (void)place_text(r, b.glyphs + in.seg_off, in.n_segs, line ? b.way_pts + 2 * (size_t)r.pt_off : nullptr,
                         line ? b.way_sincos + 2 * (size_t)r.pt_off : nullptr, out + in.seg_off);
    }
}

namespace textplacer_detail {

/* The body of validate_text_labels.  have_glyphs == false: the batch is the placement half of a string-label batch
 * (host/osmt_textshaper.hpp) — b->glyphs is not there yet (the device shapes it), b->n_glyphs is the number of chars, and
 * the limits on advance and kern were checked when the font was registered. */
inline int validate_runs(const osmt_text_label_batch* b, size_t n_jobs, std::string* why, bool have_glyphs) {
    char buf[256];
    auto bad = [&](int code, const char* fmt, auto... a) {
        std::snprintf(buf, sizeof buf, fmt, a...);
        if (why) *why = buf;
        return code;
    };
    if (!b) return bad(OSMT_INVALID_ARG, "%s", "NULL text label batch");
    if (b->n_labels == 0) return OSMT_OK;
    if (!b->labels || !b->job_label_off || !b->runs || (have_glyphs && b->n_glyphs && !b->glyphs) || (b->n_way_pts && (!b->way_pts || !b->way_sincos)))
        return bad(OSMT_INVALID_ARG, "%s", "NULL text label pool");
    if (b->n_labels >= 0xFFFFFFFFull || b->n_glyphs >= 0xFFFFFFFFull || b->n_way_pts >= 0xFFFFFFFFull)
        return bad(OSMT_INVALID_ARG, "%s", "text label batch too large");
    if (b->job_label_off[0] != 0 || b->job_label_off[n_jobs] != b->n_labels)
        return bad(OSMT_INVALID_ARG, "%s", "job_label_off must run from 0 to n_labels over n_jobs + 1 entries");
    for (size_t j = 0; j < n_jobs; ++j)
        if (b->job_label_off[j] > b->job_label_off[j + 1]) return bad(OSMT_INVALID_ARG, "%s", "job_label_off is not monotonic");
    const double LIM = 1048576.0; /* 2^20 */
    std::vector<std::pair<uint32_t, uint32_t>> slots; /* (seg_off, n_segs) of the labels that get slots */
    for (size_t l = 0; l < b->n_labels; ++l) {
        const osmt_label& in = b->labels[l];
        if (!in.has_text) continue;
        const osmt_text_run& r = b->runs[l];
        if ((size_t)in.seg_off + in.n_segs > b->n_glyphs && in.n_segs) return bad(OSMT_INVALID_ARG, "label %zu: glyph range out of bounds", l);
        if (r.position != OSMT_TEXT_CENTER && r.position != OSMT_TEXT_LINE)
            return bad(OSMT_INVALID_ARG, "label %zu: unknown text position %u", l, r.position);
        if (!std::isfinite(r.scale)) return bad(OSMT_INVALID_ARG, "label %zu: scale is not finite", l);
        for (uint32_t k = 0; have_glyphs && k < in.n_segs; ++k) {
            const osmt_text_glyph& g = b->glyphs[(size_t)in.seg_off + k];
            if (g.advance > 65535 || g.advance < -65535 || g.kern > 65535 || g.kern < -65535)
                return bad(OSMT_INVALID_ARG, "label %zu, glyph %u: |advance| or |kern| > 65535", l, k);
        }
        if (in.n_segs) slots.emplace_back(in.seg_off, in.n_segs);
        if (r.position == OSMT_TEXT_CENTER) {
            if (r.y_offset > (1u << 20)) return bad(OSMT_INVALID_ARG, "label %zu: y_offset > 2^20", l);
            if (!(std::fabs(r.center_x) <= LIM) || !(std::fabs(r.center_y) <= LIM))
                return bad(OSMT_INVALID_ARG, "label %zu: centre not finite or |v| > 2^20", l);
            continue;
        }
        if (r.n_pts == 0) continue;
        if ((size_t)r.pt_off + r.n_pts > b->n_way_pts) return bad(OSMT_INVALID_ARG, "label %zu: way point range out of bounds", l);
        for (uint32_t i = 0; i < r.n_pts; ++i) {
            const int32_t* p = b->way_pts + 2 * ((size_t)r.pt_off + i);
            const int32_t L28 = 1 << 28;
            if (p[0] > L28 || p[0] < -L28 || p[1] > L28 || p[1] < -L28) return bad(OSMT_UNSUPPORTED, "label %zu: way point %u has |v| > 2^28", l, i);
        }
        for (uint32_t e = 0; e + 1 < r.n_pts; ++e) {
            const double* sc = b->way_sincos + 2 * ((size_t)r.pt_off + e);
            if (!std::isfinite(sc[0]) || !std::isfinite(sc[1])) return bad(OSMT_INVALID_ARG, "label %zu: way_sincos of edge %u is not finite", l, e);
        }
    }
    /* every slot belongs to ONE label: the device writes a label's slots from a wave of its own.  Ranges in label order
     * (what every builder produces) cost one linear pass; only a batch that names them out of order is sorted */
    if (!std::is_sorted(slots.begin(), slots.end())) std::sort(slots.begin(), slots.end());
    for (size_t i = 1; i < slots.size(); ++i)
        if ((uint64_t)slots[i - 1].first + slots[i - 1].second > slots[i].first)
            return bad(OSMT_INVALID_ARG, "the glyph ranges of two labels overlap at glyph %u", slots[i].first);
    return OSMT_OK;
}

}  // namespace textplacer_detail

/* What osmt_validate_text_labels checks (the list is in include/osmtile.h).  Returns an OSMT_* status; *why gets the
 * reason. */
inline int validate_text_labels(const osmt_text_label_batch* b, size_t n_jobs, std::string* why) {
    return textplacer_detail::validate_runs(b, n_jobs, why, true);
}

}  // namespace osmt

#endif /* OSMT_TEXTPLACER_HPP */
