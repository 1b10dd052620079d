/*
 * osmt_glyph.h — the glyph walk of the reference (Glyph::rasterize, font/text_placer.rs:232-259, with
 * Rasterizer::draw_quad, font/rasterizer.rs:90-113) as straight-line host/device code, shared by the HIP glyph kernels
 * (osmt_glyphs.hip), the host side of the library (the window summary of a draw_line call) and a host test shim
 * (tests/glyph_shim.cpp).  -ffp-contract=off everywhere: every f64 operation below is the reference's, in its order.
 */
#ifndef OSMT_GLYPH_H
#define OSMT_GLYPH_H

#include <math.h>
#include <stdint.h>

#include "../../include/osmtile.h"
#include "osmt_geom.h" /* OSMT_HD */

/* ---- hypot ------------------------------------------------------------------------------------------------------
 * f64::hypot is the platform libm's hypot.  glibc's (>= 2.35) is NOT correctly rounded, so neither sqrt(x*x + y*y)
 * nor ocml's hypot reproduces it.  This is its algorithm, restated: Borges, "An Improved Algorithm for hypot(a,b)"
 * (2019), the variant without FMA that glibc builds for baseline x86-64 (sysdeps/ieee754/dbl-64/e_hypot.c): one
 * sqrt, one correction term, scaling by 2^-600 beyond 2^511 / below 2^-511, and the 2^-54 early-outs.  Only + - * /
 * and sqrt, all correctly rounded on the host and on gfx950 when nothing is contracted.  tests/test_glyph_hypot.py
 * (host build) and tests/test_gpu_glyph_labels.py (device) check it against the running libm bit for bit. */
OSMT_HD double osmt_hypot_kernel(double ax, double ay) {
    double h = sqrt(ax * ax + ay * ay);
    double t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}

OSMT_HD double osmt_hypot(double x, double y) {
    if (!isfinite(x) || !isfinite(y)) {
        if (isinf(x) || isinf(y)) return INFINITY;
        return x + y;
    }
    x = fabs(x);
    y = fabs(y);
    const double ax = x < y ? y : x;
    const double ay = x < y ? x : y;
    if (ax > 0x1p+511) {
        if (ay <= ax * 0x1p-54) return ax + ay;
        return osmt_hypot_kernel(ax * 0x1p-600, ay * 0x1p-600) / 0x1p-600;
    }
    if (ay < 0x1p-511) {
        if (ax >= ay / 0x1p-54) return ax + ay;
        return osmt_hypot_kernel(ax / 0x1p-600, ay / 0x1p-600) * 0x1p-600;
    }
    if (ay <= ax * 0x1p-54) return ax + ay;
    return osmt_hypot_kernel(ax, ay);
}

/* ---- the window summary of a label's draw_line calls ---------------------------------------------------------------
 * What osmt_scene_set_labels sizes a label's coverage window from (rows its calls can create inside labels_bb, columns
 * with -2 / +3 cells of slack for the rounding of eval_x_at_y, font/rasterizer.rs:37).  Integer min / max: the same
 * result in any order, so the device can reduce it with atomics. */
struct osmt_label_extent {
    uint32_t n_segs; /* draw_line calls, horizontal ones included */
    int32_t ry0, ry1, cx0, cx1;
};

OSMT_HD void osmt_label_extent_init(osmt_label_extent* e) {
    e->n_segs = 0;
    e->ry0 = INT32_MAX;
    e->ry1 = INT32_MIN;
    e->cx0 = INT32_MAX;
    e->cx1 = INT32_MIN;
}

/* one draw_line(x0, y0, x1, y1) call; W = tile width in pixels (labels_bb = [-W, 2W)).  The operations of the
 * segment form's loop, unchanged (osmt_scene_set_labels). */
OSMT_HD void osmt_label_extent_add(osmt_label_extent* e, double x0, double y0, double x1, double y1, int32_t W) {
    e->n_segs += 1;
    if (y1 - y0 == 0.0) return; /* draw_line returns (font/rasterizer.rs:30-32) */
    int32_t a = (int32_t)floor(fmin(y0, y1)), b = (int32_t)floor(fmax(y0, y1));
    a = a > -W ? a : -W;
    b = b < 2 * W - 1 ? b : 2 * W - 1;
    if (a > b) return; /* no stripe inside labels_bb */
    const int32_t c0 = (int32_t)floor(fmin(x0, x1)) - 2, c1 = (int32_t)floor(fmax(x0, x1)) + 3;
    e->ry0 = a < e->ry0 ? a : e->ry0;
    e->ry1 = b > e->ry1 ? b : e->ry1;
    e->cx0 = c0 < e->cx0 ? c0 : e->cx0;
    e->cx1 = c1 > e->cx1 ? c1 : e->cx1;
}

/* ---- the glyph walk --------------------------------------------------------------------------------------------- */
#define OSMT_GLYPH_ERR_COORD 1u /* a draw_line coordinate that is not finite or has |v| > 2^20 */
#define OSMT_GLYPH_ERR_DEPTH 2u /* a curve subdivided deeper than OSMT_QUAD_MAX_DEPTH */
#define OSMT_GLYPH_ERR_ARENA 4u /* internal: the emit pass found a call beyond the arena the count pass sized */

/* Depth cap of the subdivision walk: the path from the root is a bit mask, one bit per level.  Every quadratic is flat
 * (by draw_quad's own test) after a few levels, except for a control point collinear with and beyond the end points —
 * a cusp the curve turns back at — whose piece stays folded until the coordinates run out of precision. */
#define OSMT_QUAD_MAX_DEPTH 62

/* TextPlacer::place's `tr` (text_placer.rs:87-101 for OSMT_GLYPH_LINE, :150-153 for OSMT_GLYPH_CENTER) */
OSMT_HD void osmt_glyph_tr(uint32_t form, const double* p, double x, double y, double* ox, double* oy) {
    if (form == OSMT_GLYPH_LINE) {
        const double translated_x = x - p[0];
        const double translated_y = y - p[1];
        const double rotated_x = translated_x * p[3] - translated_y * p[2];
        const double rotated_y = translated_y * p[3] + translated_x * p[2];
        *ox = p[4] + rotated_x;
        *oy = p[5] - rotated_y;
    } else {
        *ox = p[0] + x;
        *oy = p[1] - y;
    }
}

/* Rasterizer::draw_quad (font/rasterizer.rs:90-113) without recursion: depth first, left half first, the node's three
 * points recomputed from the root along its path (a child is a pure function of its parent's points, so the values are
 * bit-identical to the recursive ones).  emit(x0, y0, x1, y1) receives the draw_line calls in the reference's order.
 * Returns 0 or OSMT_GLYPH_ERR_DEPTH (then the calls emitted so far are a prefix only). */
template <class Emit>
OSMT_HD uint32_t osmt_quad_walk(double x0, double y0, double x1, double y1, double x2, double y2, Emit& emit) {
    uint64_t path = 0; /* bit k: half taken at level k (0 = left) */
    int depth = 0;
    for (;;) {
        double a0 = x0, b0 = y0, a1 = x1, b1 = y1, a2 = x2, b2 = y2;
        for (int k = 0; k < depth; ++k) {
            const double m01_x = (a0 + a1) / 2.0, m01_y = (b0 + b1) / 2.0;
            const double m12_x = (a1 + a2) / 2.0, m12_y = (b1 + b2) / 2.0;
            const double m012_x = (m01_x + m12_x) / 2.0, m012_y = (m01_y + m12_y) / 2.0;
            if ((path >> k) & 1u) {
                a0 = m012_x, b0 = m012_y, a1 = m12_x, b1 = m12_y;
            } else {
                a1 = m01_x, b1 = m01_y, a2 = m012_x, b2 = m012_y;
            }
        }
        const double d01 = osmt_hypot(fabs(a0 - a1), fabs(b0 - b1));
        const double d12 = osmt_hypot(fabs(a1 - a2), fabs(b1 - b2));
        const double d02 = osmt_hypot(fabs(a0 - a2), fabs(b0 - b2));
        if ((d01 + d12) <= 1.0001 * d02) {
            emit(a0, b0, a2, b2);
            while (depth > 0 && ((path >> (depth - 1)) & 1u)) {
                path &= ~((uint64_t)1 << (depth - 1));
                --depth;
            }
            if (depth == 0) return 0;
            path |= (uint64_t)1 << (depth - 1);
        } else {
            if (depth == OSMT_QUAD_MAX_DEPTH) return OSMT_GLYPH_ERR_DEPTH;
            ++depth; /* left child: bit depth - 1 is clear */
        }
    }
}

/* Glyph::rasterize's body for vertex i of an outline (text_placer.rs:238-257): `from` is the previous vertex's point
 * (whatever its type; (0, 0) for the first), a MoveTo only moves, a LineTo is draw_line(tr(to), tr(from)), a CurveTo is
 * draw_quad(tr(to), tr(mid), tr(from)). */
template <class Emit>
OSMT_HD uint32_t osmt_glyph_vertex_walk(const osmt_glyph_vertex* v, uint32_t i, double scale, uint32_t form, const double* p,
                                        Emit& emit) {
    const osmt_glyph_vertex cur = v[i];
    if (cur.type != OSMT_GLYPH_LINE_TO && cur.type != OSMT_GLYPH_CURVE_TO) return 0;
    double fx = 0.0, fy = 0.0;
    if (i > 0) {
        fx = (double)v[i - 1].x * scale;
        fy = (double)v[i - 1].y * scale;
    }
    const double tx = (double)cur.x * scale, ty = (double)cur.y * scale;
    double p0x, p0y, p2x, p2y;
    osmt_glyph_tr(form, p, fx, fy, &p2x, &p2y);
    osmt_glyph_tr(form, p, tx, ty, &p0x, &p0y);
    if (cur.type == OSMT_GLYPH_LINE_TO) {
        emit(p0x, p0y, p2x, p2y);
        return 0;
    }
    double p1x, p1y;
    osmt_glyph_tr(form, p, (double)cur.cx * scale, (double)cur.cy * scale, &p1x, &p1y);
    return osmt_quad_walk(p0x, p0y, p1x, p1y, p2x, p2y, emit);
}

/* |v| <= 2^20 and finite, for all four coordinates of a call (the segment form's rule, osmt_scene_set_labels) */
OSMT_HD bool osmt_label_seg_in_range(double x0, double y0, double x1, double y1) {
    const double LIM = 1048576.0;
    return fabs(x0) <= LIM && fabs(y0) <= LIM && fabs(x1) <= LIM && fabs(y1) <= LIM;
}

#endif /* OSMT_GLYPH_H */
