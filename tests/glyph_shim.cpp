// Host build of the glyph walk the HIP glyph kernels run (osm_renderer_amd/csrc/osmt_glyph.h: the device hypot, the
// subdivision walk, the two transforms, the window summary) plus sizeof / offsetof probes of the glyph-run ABI structs,
// for the CPU-side tests.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../include/osmtile.h"
#include "../osm_renderer_amd/csrc/osmt_glyph.h"

namespace {
struct collect {
    double* out;
    size_t cap, n;
    void operator()(double x0, double y0, double x1, double y1) {
        if (n < cap) {
            out[4 * n + 0] = x0;
            out[4 * n + 1] = y0;
            out[4 * n + 2] = x1;
            out[4 * n + 3] = y1;
        }
        ++n;
    }
};
}  // namespace

extern "C" {
void shim_hypot(const double* xy, size_t n, double* out) {
    for (size_t i = 0; i < n; ++i) out[i] = osmt_hypot(xy[2 * i], xy[2 * i + 1]);
}
// pairs whose osmt_hypot differs in any bit from this process's libm hypot
size_t shim_hypot_mismatches(const double* xy, size_t n) {
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const double g = osmt_hypot(xy[2 * i], xy[2 * i + 1]), w = ::hypot(xy[2 * i], xy[2 * i + 1]);
        bad += std::memcmp(&g, &w, sizeof g) != 0;
    }
    return bad;
}
// the draw_line calls of instances [0, n_inst) in order, as the device walk makes them (vertex by vertex); returns the
// number of calls (out holds the first `cap`), or -(OSMT_GLYPH_ERR_*) on error
int64_t shim_glyph_expand(const osmt_glyph_vertex* verts, const uint32_t* voff, const osmt_glyph_instance* inst, size_t n_inst,
                          double* out, size_t cap) {
    collect c{out, cap, 0};
    for (size_t k = 0; k < n_inst; ++k) {
        const osmt_glyph_instance& g = inst[k];
        const uint32_t v0 = voff[g.glyph_id], nv = voff[g.glyph_id + 1] - v0;
        for (uint32_t i = 0; i < nv; ++i) {
            const uint32_t e = osmt_glyph_vertex_walk(verts + v0, i, g.scale, g.form, g.p, c);
            if (e) return -(int64_t)e;
        }
    }
    return (int64_t)c.n;
}
// the window summary of n calls: {n_segs, ry0, ry1, cx0, cx1}
void shim_label_extent(const double* segs, size_t n, int32_t W, int32_t* out) {
    osmt_label_extent e;
    osmt_label_extent_init(&e);
    for (size_t i = 0; i < n; ++i) osmt_label_extent_add(&e, segs[4 * i], segs[4 * i + 1], segs[4 * i + 2], segs[4 * i + 3], W);
    out[0] = (int32_t)e.n_segs;
    out[1] = e.ry0;
    out[2] = e.ry1;
    out[3] = e.cx0;
    out[4] = e.cx1;
}
size_t shim_glyph_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_glyph_vertex);
        case 1: return sizeof(osmt_glyph_instance);
        case 2: return sizeof(osmt_glyph_label_batch);
        case 10: return offsetof(osmt_glyph_vertex, type);
        case 11: return offsetof(osmt_glyph_instance, scale);
        case 12: return offsetof(osmt_glyph_instance, p);
        case 13: return offsetof(osmt_glyph_label_batch, glyphs);
        case 14: return offsetof(osmt_glyph_label_batch, n_glyphs);
        case 20: return OSMT_GLYPH_CENTER;
        case 21: return OSMT_GLYPH_LINE;
        case 22: return OSMT_QUAD_MAX_DEPTH;
    }
    return 0;
}
}
