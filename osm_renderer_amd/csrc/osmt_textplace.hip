/*
 * osmt_textplace.hip — label text given as text runs (osmt_scene_set_text_labels): TextPlacer::place of the reference
 * (font/text_placer.rs:24-168, compute_way_position :270-296) on the GPU, writing the osmt_glyph_instance array that the
 * glyph-run form uploads from the host.  k_glyph_count / k_glyph_emit (osmt_glyphs.hip) expand it on the same stream.
 * gfx950 only; -ffp-contract=off: every f64 operation is the reference's, and every sum is made in its order.
 *
 *   k_text_place   one wave per label.  Lanes compute what is a pure function of one glyph or one edge — the width
 *                  f64(advance) * scale (+ f64(kern) * scale), the edge length sqrt(dx*dx + dy*dy) — 64 at a time; the
 *                  running sums (total_width, current_row_width, cur_x, total_way_length, cur_dist) are made serially,
 *                  the terms handed round with v_readlane, because their order changes bits.  Texts and ways of any
 *                  length are worked through in chunks of 64; nothing is truncated.
 *                    CENTER: a pass that counts the rows (total_height needs the count before the first glyph is
 *                            placed), then per row a scan to its end (row_width) and a pass that places its glyphs.
 *                    LINE:   total_width, total_way_length, then per chunk of 64 glyphs the serial cur_dist and
 *                            compute_way_position for all 64 at once: the wave walks the edge lengths together, every
 *                            lane keeping a to_travel of its own, until the last lane has found its edge.
 *
 * The host twin is host/osmt_textplacer.hpp (the same bits; it also holds the validation every call runs first, so that
 * all ranges read here are inside their tables).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osmt_internal.h"

namespace {

constexpr uint32_t TEXT_WAVES = 4; /* waves (labels) per workgroup */
constexpr double MAX_TEXT_WIDTH = 32.0; /* TILE_SIZE as f64 / 8.0 (text_placer.rs:298): not scaled */

/* the value lane `src` holds, in every lane (src uniform): two v_readlane_b32 */
__device__ __forceinline__ double bcast(double v, uint32_t src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), (int)src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), (int)src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src); }
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

/* glyphs [c0, c0 + 64) of a text, one per lane: Glyph::width of text_to_glyphs (text_placer.rs:180-189) */
struct glyph_chunk {
    double w;
    uint32_t ws, id;
};
__device__ __forceinline__ glyph_chunk load_glyphs(const osmt_text_glyph* __restrict__ g, uint32_t c0, uint32_t end, uint32_t lane, double scale) {
    glyph_chunk c{0.0, 0u, 0u};
    const uint32_t k = c0 + lane;
    if (k < end) {
        const osmt_text_glyph t = g[k];
        c.w = (double)t.advance * scale;
        if (k != 0u) c.w += (double)t.kern * scale;
        c.ws = t.flags & 1u;
        c.id = t.glyph_id;
    }
    return c;
}

/* Point::dist (point.rs:21-25) of edge e -> e + 1 */
__device__ __forceinline__ double edge_length(const int2* __restrict__ pts, uint32_t e) {
    const int2 from = pts[e], to = pts[e + 1u];
    const double dx = (double)(from.x - to.x);
    const double dy = (double)(from.y - to.y);
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ void store_instance(osmt_glyph_instance* __restrict__ out, uint32_t id, uint32_t form, double scale, double p0,
                                               double p1, double p2, double p3, double p4, double p5) {
    osmt_glyph_instance o;
    o.glyph_id = id;
    o.form = form;
    o.scale = scale;
    o.p[0] = p0, o.p[1] = p1, o.p[2] = p2, o.p[3] = p3, o.p[4] = p4, o.p[5] = p5;
    *out = o;
}

__device__ __forceinline__ void place_line(const osmt_text_run& r, const osmt_text_glyph* __restrict__ g, uint32_t n, const int2* __restrict__ pts,
                                           const double2* __restrict__ sincos, osmt_glyph_instance* __restrict__ out, uint32_t lane,
                                           double descent, double ascent) {
    const double scale = r.scale;
    const uint32_t np = uniform(r.n_pts);
    double total_width = 0.0;
    for (uint32_t c0 = 0u; c0 < n; c0 += 64u) {
        const glyph_chunk c = load_glyphs(g, c0, n, lane, scale);
        const uint32_t cnt = min(64u, n - c0);
        for (uint32_t j = 0u; j < cnt; ++j) total_width += bcast(c.w, j);
    }
    bool placed = np >= 2u;
    double total_way_length = 0.0;
    if (placed) {
        const uint32_t ne = np - 1u;
        for (uint32_t base = 0u; base < ne; base += 64u) {
            const uint32_t e = base + lane;
            const double d = e < ne ? edge_length(pts, e) : 0.0;
            const uint32_t cnt = min(64u, ne - base);
            for (uint32_t j = 0u; j < cnt; ++j) total_way_length += bcast(d, j);
        }
        placed = !(total_width > total_way_length);
    }
    if (!placed) { /* place() returns true before rasterizing (text_placer.rs:62-64, 76-78) */
        for (uint32_t c0 = 0u; c0 < n; c0 += 64u) {
            const glyph_chunk c = load_glyphs(g, c0, n, lane, scale);
            if (c0 + lane < n) store_instance(out + c0 + lane, c.id, OSMT_GLYPH_NONE, scale, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
        }
        return;
    }
    const uint32_t ne = np - 1u;
    double cur_dist = (total_way_length - total_width) / 2.0;
    const double glyph_center_y = (descent + ascent) / 2.0;
    for (uint32_t c0 = 0u; c0 < n; c0 += 64u) {
        const glyph_chunk c = load_glyphs(g, c0, n, lane, scale);
        const uint32_t cnt = min(64u, n - c0);
        double my_dist = 0.0;
        for (uint32_t j = 0u; j < cnt; ++j) {
            if (lane == j) my_dist = cur_dist;
            cur_dist += bcast(c.w, j);
        }
        /* compute_way_position(points, cur_dist + glyph_center_x) of 64 glyphs at once */
        const bool mine = c0 + lane < n;
        const double glyph_center_x = c.w / 2.0;
        double to_travel = my_dist + glyph_center_x;
        bool walking = mine && to_travel > 0.0; /* an advance <= 0 never enters the loop: the last point */
        bool hit = false;
        uint32_t edge = ne - 1u;
        double ratio = 0.0;
        for (uint32_t base = 0u; base < ne && __any(walking); base += 64u) {
            const uint32_t e = base + lane;
            const double d = e < ne ? edge_length(pts, e) : 0.0;
            const uint32_t ecnt = min(64u, ne - base);
            for (uint32_t j = 0u; j < ecnt; ++j) {
                const double seg_dist = bcast(d, j);
                if (walking) {
                    if (seg_dist >= to_travel) {
                        ratio = to_travel / seg_dist;
                        edge = base + j;
                        hit = true;
                        walking = false;
                    } else {
                        to_travel -= seg_dist;
                        walking = to_travel > 0.0;
                    }
                }
            }
        }
        if (mine) {
            double x, y;
            if (hit) {
                const int2 from = pts[edge], to = pts[edge + 1u];
                x = (double)from.x + ((double)(to.x - from.x) * ratio);
                y = (double)from.y + ((double)(to.y - from.y) * ratio);
            } else { /* ran off the end, or never started */
                const int2 last = pts[ne];
                x = (double)last.x;
                y = (double)last.y;
            }
            const double2 sc = sincos[edge];
            store_instance(out + c0 + lane, c.id, OSMT_GLYPH_LINE, scale, glyph_center_x, glyph_center_y, sc.x, sc.y, x, y);
        }
    }
}

__device__ __forceinline__ void place_center(const osmt_text_run& r, const osmt_text_glyph* __restrict__ g, uint32_t n,
                                             osmt_glyph_instance* __restrict__ out, uint32_t lane, double descent, double ascent, double line_gap) {
    const double scale = r.scale;
    /* the rows (text_placer.rs:119-133): current_row_width restarts at 0.0 in every row and already holds the glyph's
     * width when the break is tested */
    uint32_t rows = 0u;
    {
        double current_row_width = 0.0;
        for (uint32_t c0 = 0u; c0 < n; c0 += 64u) {
            const glyph_chunk c = load_glyphs(g, c0, n, lane, scale);
            const uint32_t cnt = min(64u, n - c0);
            for (uint32_t j = 0u; j < cnt; ++j) {
                const double w = bcast(c.w, j);
                current_row_width += w;
                const bool is_last_glyph = c0 + j + 1u == n;
                const bool should_break = bcast(c.ws, j) != 0u && (current_row_width + w > MAX_TEXT_WIDTH);
                if (should_break || is_last_glyph) {
                    ++rows;
                    current_row_width = 0.0;
                }
            }
        }
    }
    const double row_height = ascent - descent + line_gap;
    const double total_height = row_height * (double)rows;
    double cur_y = r.center_y;
    if (r.y_offset > 0u)
        cur_y += (double)r.y_offset;
    else
        cur_y -= total_height / 2.0;
    for (uint32_t row_start = 0u; row_start < n;) {
        /* to the row's end: its width is needed before its first glyph is placed */
        uint32_t row_end = n;
        double row_width = 0.0;
        bool closed = false;
        for (uint32_t c0 = row_start; c0 < n && !closed; c0 += 64u) {
            const glyph_chunk c = load_glyphs(g, c0, n, lane, scale);
            const uint32_t cnt = min(64u, n - c0);
            for (uint32_t j = 0u; j < cnt && !closed; ++j) {
                const double w = bcast(c.w, j);
                row_width += w;
                const bool is_last_glyph = c0 + j + 1u == n;
                const bool should_break = bcast(c.ws, j) != 0u && (row_width + w > MAX_TEXT_WIDTH);
                if (should_break || is_last_glyph) {
                    row_end = c0 + j + 1u;
                    closed = true;
                }
            }
        }
        double cur_x = r.center_x - row_width / 2.0;
        const double baseline = cur_y + ascent;
        for (uint32_t c0 = row_start; c0 < row_end; c0 += 64u) {
            const glyph_chunk c = load_glyphs(g, c0, row_end, lane, scale);
            const uint32_t cnt = min(64u, row_end - c0);
            double x_offset = 0.0;
            for (uint32_t j = 0u; j < cnt; ++j) {
                if (lane == j) x_offset = cur_x;
                cur_x += bcast(c.w, j);
            }
            if (c0 + lane < row_end) store_instance(out + c0 + lane, c.id, OSMT_GLYPH_CENTER, scale, x_offset, baseline, 0.0, 0.0, 0.0, 0.0);
        }
        cur_y += row_height;
        row_start = row_end;
    }
}

__global__ __launch_bounds__(256) void k_text_place(osmt_text_pass a) {
    const uint32_t l = uniform(blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (l >= a.n_labels) return; /* whole wave */
    const osmt_label& lab = a.labels[l];
    const uint32_t n = uniform(lab.n_segs);
    if (!uniform(lab.has_text) || n == 0u) return;
    const uint32_t first = uniform(lab.seg_off);
    const osmt_text_run r = a.runs[l];
    /* get_v_metrics (text_placer.rs:199-207) */
    const double descent = (double)r.descent * r.scale, ascent = (double)r.ascent * r.scale, line_gap = (double)r.line_gap * r.scale;
    if (uniform(r.position) == OSMT_TEXT_LINE) {
        const uint32_t pt_off = uniform(r.pt_off);
        place_line(r, a.glyphs + first, n, reinterpret_cast<const int2*>(a.way_pts) + pt_off, reinterpret_cast<const double2*>(a.way_sincos) + pt_off,
                   a.inst + first, lane, descent, ascent);
    } else {
        place_center(r, a.glyphs + first, n, a.inst + first, lane, descent, ascent, line_gap);
    }
}

}  // namespace

hipError_t osmt_launch_text_place(const osmt_text_pass& a, hipStream_t st) {
    if (!a.n_labels) return hipSuccess;
    hipLaunchKernelGGL(k_text_place, dim3((a.n_labels + TEXT_WAVES - 1) / TEXT_WAVES), dim3(256), 0, st, a);
    return hipGetLastError();
}
