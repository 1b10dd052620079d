// The glyph-run path of the C++ host mirror (osm_renderer_amd/host/osmt_draw.hpp): the same labels drawn twice, once with
// Rasterizer::draw_glyph (one instance per Glyph::rasterize call, expanded on the GPU by osmt_render_batch_rgb_glyphs)
// and once with the reference's own glyph walk on the host (Glyph::rasterize, font/text_placer.rs:232-259, calling
// draw_line / draw_quad with libm's hypot).  Writes three tiles of RGB triples to argv[1] — glyph runs, draw_line
// calls, no labels — for tests/test_gpu_host_mirror_glyphs.py.  TileBatch must refuse a glyph-run tile (exit code 4).
#include <cmath>
#include <cstdio>
#include <functional>

#include "../osm_renderer_amd/host/osmt_draw.hpp"

using namespace osmt;

namespace {

using Outline = std::vector<osmt_glyph_vertex>;

osmt_glyph_vertex vx(uint8_t type, int16_t x, int16_t y, int16_t cx = 0, int16_t cy = 0) { return osmt_glyph_vertex{x, y, cx, cy, type, 0}; }

std::vector<Outline> outlines() {
    /* outer contours clockwise with y up, as TrueType draws them (the other way round the coverage is negative) */
    Outline ring = {vx(1, 560, 360)}; /* an "o": 8 quadratic arcs around (310, 360) */
    const double k = 1.0 / std::cos(M_PI / 8);
    for (int i = 1; i <= 8; ++i) {
        const double a = -2 * M_PI * i / 8, m = -2 * M_PI * (i - 0.5) / 8;
        ring.push_back(vx(3, (int16_t)(310 + 250 * std::cos(a)), (int16_t)(360 + 370 * std::sin(a)), (int16_t)(310 + k * 250 * std::cos(m)),
                          (int16_t)(360 + k * 370 * std::sin(m))));
    }
    Outline poly = {vx(1, 80, 0), vx(2, 80, 720), vx(2, 180, 720), vx(2, 180, 90), vx(2, 500, 90), vx(2, 500, 0), vx(2, 80, 0)}; /* "L" */
    return {ring, poly, Outline{}};
}

/* Glyph::rasterize on the host: the reference's walk with the mirror's draw_line / draw_quad */
void rasterize_host(Rasterizer& r, const Outline& o, double scale, const std::function<std::pair<double, double>(double, double)>& tr) {
    double fx = 0.0, fy = 0.0;
    for (const osmt_glyph_vertex& v : o) {
        const double tx = (double)v.x * scale, ty = (double)v.y * scale;
        if (v.type == 2) {
            auto p1 = tr(fx, fy), p0 = tr(tx, ty);
            r.draw_line(p0.first, p0.second, p1.first, p1.second);
        } else if (v.type == 3) {
            auto p2 = tr(fx, fy), p1 = tr((double)v.cx * scale, (double)v.cy * scale), p0 = tr(tx, ty);
            r.draw_quad(p0.first, p0.second, p1.first, p1.second, p2.first, p2.second);
        }
        fx = tx;
        fy = ty;
    }
}

struct Placed {
    uint32_t glyph;
    uint32_t form;
    double p[6];
};

/* one label: a text of several glyphs, recorded as instances or as calls */
void label(TilePixels& px, const std::vector<Outline>& ol, uint32_t first_id, Color c, double scale, const std::vector<Placed>& glyphs, bool as_runs) {
    Rasterizer r(c);
    for (const Placed& g : glyphs) {
        if (as_runs) {
            r.draw_glyph(first_id + g.glyph, scale, g.form, g.p);
            continue;
        }
        const double* p = g.p;
        if (g.form == OSMT_GLYPH_CENTER) {
            rasterize_host(r, ol[g.glyph], scale, [p](double x, double y) { return std::make_pair(p[0] + x, p[1] - y); });
        } else { /* text_placer.rs:87-101 */
            rasterize_host(r, ol[g.glyph], scale, [p](double x, double y) {
                const double translated_x = x - p[0], translated_y = y - p[1];
                const double rotated_x = translated_x * p[3] - translated_y * p[2];
                const double rotated_y = translated_y * p[3] + translated_x * p[2];
                return std::make_pair(p[4] + rotated_x, p[5] - rotated_y);
            });
        }
    }
    r.save_to_figure(px);
    px.bump_label_generation(true);
}

void draw(TilePixels& px, const std::vector<Outline>& ol, uint32_t first_id, bool with_labels, bool as_runs) {
    px.reset(Color{241, 238, 232});
    PointPairs sq = {{{20, 20}, {230, 40}}, {{230, 40}, {200, 230}}, {{200, 230}, {20, 20}}};
    fill_contour(sq, Filler::from_color(Color{180, 200, 160}), 0.7, px);
    px.bump_generation();
    px.blend_unfinished_pixels(false);
    if (!with_labels) return;
    const double s1 = 0.03, s2 = 0.035;
    /* TextPosition::Center: x_offset advances by the glyph widths (620, 560, 260 units) */
    label(px, ol, first_id, Color{102, 102, 255}, s1, {{0, OSMT_GLYPH_CENTER, {60.25, 80.5}}, {1, OSMT_GLYPH_CENTER, {60.25 + 620 * s1, 80.5}},
          {2, OSMT_GLYPH_CENTER, {60.25 + 1180 * s1, 80.5}}, {0, OSMT_GLYPH_CENTER, {60.25 + 1440 * s1, 80.5}}}, as_runs);
    /* TextPosition::Line along a way from (120, 160) at 0.4 rad: (sin, cos) of -angle, way position at each glyph's centre */
    const double sn = std::sin(-0.4), cs = std::cos(-0.4), gcy = 300 * s2, w1 = 560 * s2, w0 = 620 * s2;
    const double d1 = w1 / 2, d0 = w1 + w0 / 2;
    label(px, ol, first_id, Color{20, 20, 20}, s2, {{1, OSMT_GLYPH_LINE, {w1 / 2, gcy, sn, cs, 120.0 + d1 * std::cos(0.4), 160.0 + d1 * std::sin(0.4)}},
          {0, OSMT_GLYPH_LINE, {w0 / 2, gcy, sn, cs, 120.0 + d0 * std::cos(0.4), 160.0 + d0 * std::sin(0.4)}}}, as_runs);
    /* collides with the first label: fails as a whole */
    label(px, ol, first_id, Color{255, 0, 0}, s2, {{0, OSMT_GLYPH_CENTER, {64.0, 84.0}}}, as_runs);
    px.blend_unfinished_pixels(true);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        Context ctx(0);
        const std::vector<Outline> ol = outlines();
        std::vector<osmt_glyph_vertex> v;
        std::vector<uint32_t> off = {0};
        for (const Outline& o : ol) {
            v.insert(v.end(), o.begin(), o.end());
            off.push_back((uint32_t)v.size());
        }
        const uint32_t first = ctx.register_glyphs(v.data(), off.data(), (uint32_t)ol.size());
        TilePixels runs(ctx, 1), calls(ctx, 1), plain(ctx, 1);
        draw(runs, ol, first, true, true);
        draw(calls, ol, first, true, false);
        draw(plain, ol, first, false, false);
        const Tile t{15, 19807, 10243};
        RgbTriples a = runs.to_rgb_triples(t), b = calls.to_rgb_triples(t), c = plain.to_rgb_triples(t);
        FILE* f = fopen(argv[1], "wb");
        if (!f) return 3;
        for (const RgbTriples* tile : {&a, &b, &c})
            for (auto& [r, g, bl] : *tile) {
                const unsigned char px[3] = {r, g, bl};
                fwrite(px, 1, 3, f);
            }
        fclose(f);
        TileBatch batch(ctx, 1);
        try {
            batch.add(t, runs);
            return 4;
        } catch (const Error& e) {
            if (e.code != OSMT_UNSUPPORTED) return 5;
        }
    } catch (const Error& e) {
        fprintf(stderr, "osmt error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
