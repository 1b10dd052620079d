/*
 * osmt_textshaper.hpp — from a label's code points to the glyphs of its text: a scalar C++ statement of the reference's
 * TextPlacer::text_to_glyphs (src/draw/font/text_placer.rs:170-197) over the flat font tables of osmt_register_font:
 * string labels (osmt_string_label_batch) in, the osmt_text_glyph records of the text-run form out.
 *
 * Three users: the CPU half of the tests (tests/shape_shim.cpp), an integrator without a device, and the library itself,
 * which runs validate_font at every osmt_register_font and validate_string_labels before every upload.  The device kernel
 * (csrc/osmt_textshape.hip) returns the same records.
 *
 * Integer work throughout; the one floating-point operation is the f32 division of scale_for_pixel_height, made on the
 * host by the library too (string_scale).
 */
#ifndef OSMT_TEXTSHAPER_HPP
#define OSMT_TEXTSHAPER_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/osmtile.h"
#include "osmt_textplacer.hpp"

namespace osmt {

namespace textshaper_detail {

/* a Rust `char`: a Unicode scalar value */
inline bool is_char(uint32_t cp) { return cp <= 0x10FFFFu && !(cp >= 0xD800u && cp <= 0xDFFFu); }

/* char::is_whitespace: the Unicode White_Space set.  Not isspace: U+001C-001F, 180E, 200B and FEFF are not in it. */
inline bool is_whitespace(uint32_t cp) {
    return (cp >= 0x0009u && cp <= 0x000Du) || cp == 0x0020u || cp == 0x0085u || cp == 0x00A0u || cp == 0x1680u ||
           (cp >= 0x2000u && cp <= 0x200Au) || cp == 0x2028u || cp == 0x2029u || cp == 0x202Fu || cp == 0x205Fu || cp == 0x3000u;
}

/* find_glyph_index: the entry of `cp` by bisection, glyph 0 when there is none */
inline uint32_t find_glyph(const osmt_cmap_entry* cmap, size_t n, uint32_t cp) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (cmap[mid].code_point < cp)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && cmap[lo].code_point == cp ? cmap[lo].glyph : 0u;
}

/* get_glyph_kern_advance: the value of (left, right) by bisection on the 64-bit key, 0 when the pair is not listed */
inline int32_t find_kern(const osmt_kern_pair* kern, size_t n, uint32_t left, uint32_t right) {
    const uint64_t key = ((uint64_t)left << 32) | right;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if ((((uint64_t)kern[mid].left << 32) | kern[mid].right) < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && kern[lo].left == left && kern[lo].right == right ? kern[lo].value : 0;
}

}  // namespace textshaper_detail

/* f64::from(font.scale_for_pixel_height(font_size as f32)): ONE f32 division, widened */
inline double string_scale(const osmt_font_desc& f, double font_size) {
    return (double)((float)font_size / (float)(f.ascent - f.descent));
}

/* text_to_glyphs of one text: chars[0 .. n) in, out[k] = the record of char k.  The predecessor of char k is char k - 1 of
 * THIS text; the first char has kern 0. */
inline void shape_text(const osmt_font_desc& f, const uint32_t* chars, uint32_t n, osmt_text_glyph* out) {
    using namespace textshaper_detail;
    uint32_t prev = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = find_glyph(f.cmap, f.n_cmap, chars[k]);
        osmt_text_glyph o;
        o.glyph_id = f.outline_id[g];
        o.advance = f.advance[g];
        o.kern = k ? find_kern(f.kern, f.n_kern, prev, g) : 0;
        o.flags = is_whitespace(chars[k]) ? 1u : 0u;
        out[k] = o;
        prev = g;
    }
}

/* The whole batch: out[n_chars], slot seg_off + k = char k of its label; slots no has_text label names are zero.  The
 * batch must have passed validate_string_labels against the same fonts. */
inline void shape_string_labels(const osmt_string_label_batch& b, const osmt_font_desc* const* fonts, osmt_text_glyph* out) {
    for (size_t i = 0; i < b.n_chars; ++i) out[i] = osmt_text_glyph{};
    for (size_t l = 0; l < b.n_labels; ++l) {
        const osmt_label& in = b.labels[l];
        if (!in.has_text || in.n_segs == 0) continue;
        shape_text(*fonts[b.runs[l].font_id], b.chars + in.seg_off, in.n_segs, out + in.seg_off);
    }
}

/* What osmt_register_font checks (the list is in include/osmtile.h); n_outlines = the size of the context's glyph table. */
inline int validate_font(const osmt_font_desc* f, size_t n_outlines, std::string* why) {
    char buf[256];
    auto bad = [&](const char* fmt, auto... a) {
        std::snprintf(buf, sizeof buf, fmt, a...);
        if (why) *why = buf;
        return (int)OSMT_INVALID_ARG;
    };
    if (!f) return bad("%s", "NULL font");
    if (f->n_glyphs == 0) return bad("%s", "a font needs glyph 0 (n_glyphs == 0)");
    if (!f->advance || !f->outline_id || (f->n_cmap && !f->cmap) || (f->n_kern && !f->kern)) return bad("%s", "NULL font table");
    if (f->n_glyphs >= 0xFFFFFFFFull || f->n_cmap >= 0xFFFFFFFFull || f->n_kern >= 0xFFFFFFFFull) return bad("%s", "font table too large");
    if ((int64_t)f->ascent - (int64_t)f->descent == 0) return bad("%s", "ascent - descent == 0: the font has no height to scale by");
    for (size_t i = 0; i < f->n_cmap; ++i) {
        const osmt_cmap_entry& c = f->cmap[i];
        if (!textshaper_detail::is_char(c.code_point)) return bad("cmap entry %zu: U+%X is not a Unicode scalar value", i, c.code_point);
        if (i && f->cmap[i - 1].code_point >= c.code_point) return bad("cmap entry %zu: code points are not strictly increasing", i);
        if (c.glyph >= f->n_glyphs) return bad("cmap entry %zu: glyph %u >= n_glyphs (%zu)", i, c.glyph, f->n_glyphs);
    }
    for (size_t g = 0; g < f->n_glyphs; ++g) {
        if (f->advance[g] > 65535 || f->advance[g] < -65535) return bad("glyph %zu: |advance| > 65535", g);
        if (f->outline_id[g] >= n_outlines)
            return bad("glyph %zu: outline id %u is not in the glyph table (%zu glyphs)", g, f->outline_id[g], n_outlines);
    }
    for (size_t i = 0; i < f->n_kern; ++i) {
        const osmt_kern_pair& k = f->kern[i];
        if (k.left >= f->n_glyphs || k.right >= f->n_glyphs) return bad("kern pair %zu: glyph (%u, %u) >= n_glyphs (%zu)", i, k.left, k.right, f->n_glyphs);
        if (i && (((uint64_t)f->kern[i - 1].left << 32) | f->kern[i - 1].right) >= (((uint64_t)k.left << 32) | k.right))
            return bad("kern pair %zu: (left, right) is not strictly increasing", i);
        if (k.value > 65535 || k.value < -65535) return bad("kern pair %zu: |value| > 65535", i);
    }
    return OSMT_OK;
}

/* What osmt_validate_string_labels checks (the list is in include/osmtile.h); fonts[i] = font id i, as registered.
 * Returns an OSMT_* status; *why gets the reason.  runs_out (optional) receives the osmt_text_run of every label — the
 * placement half of the batch as k_text_place reads it, the scale and the v-metrics filled in from the font. */
inline int validate_string_labels(const osmt_string_label_batch* b, size_t n_jobs, const osmt_font_desc* const* fonts, size_t n_fonts,
                                  std::string* why, std::vector<osmt_text_run>* runs_out = nullptr) {
    char buf[256];
    auto bad = [&](const char* fmt, auto... a) {
        std::snprintf(buf, sizeof buf, fmt, a...);
        if (why) *why = buf;
        return (int)OSMT_INVALID_ARG;
    };
    if (runs_out) runs_out->clear();
    if (!b) return bad("%s", "NULL string label batch");
    if (b->n_labels == 0) return OSMT_OK;
    if (!b->labels || !b->job_label_off || !b->runs || (b->n_chars && !b->chars) || (b->n_way_pts && (!b->way_pts || !b->way_sincos)))
        return bad("%s", "NULL string label pool");
    if (b->n_labels >= 0xFFFFFFFFull || b->n_chars >= 0xFFFFFFFFull || b->n_way_pts >= 0xFFFFFFFFull)
        return bad("%s", "string label batch too large");
    std::vector<osmt_text_run> runs(b->n_labels, osmt_text_run{});
    for (size_t l = 0; l < b->n_labels; ++l) {
        const osmt_label& in = b->labels[l];
        if (!in.has_text) continue;
        const osmt_string_run& s = b->runs[l];
        if (s.font_id >= n_fonts) return bad("label %zu: font id %u is not registered (%zu fonts)", l, s.font_id, n_fonts);
        if (!std::isfinite(s.font_size)) return bad("label %zu: font_size is not finite", l);
        const osmt_font_desc& f = *fonts[s.font_id];
        osmt_text_run& r = runs[l];
        r.position = s.position;
        r.y_offset = s.y_offset;
        r.pt_off = s.pt_off;
        r.n_pts = s.n_pts;
        r.scale = string_scale(f, s.font_size);
        r.ascent = f.ascent;
        r.descent = f.descent;
        r.line_gap = f.line_gap;
        r.center_x = s.center_x;
        r.center_y = s.center_y;
        if (!std::isfinite(r.scale)) return bad("label %zu: the scale of font_size %g is not finite", l, s.font_size);
        if (in.n_segs && (size_t)in.seg_off + in.n_segs > b->n_chars) return bad("label %zu: char range out of bounds", l);
        for (uint32_t k = 0; k < in.n_segs; ++k) {
            const uint32_t cp = b->chars[(size_t)in.seg_off + k];
            if (!textshaper_detail::is_char(cp)) return bad("label %zu, char %u: U+%X is not a Unicode scalar value", l, k, cp);
        }
    }
    osmt_text_label_batch t{};
    t.labels = b->labels;
    t.n_labels = b->n_labels;
    t.job_label_off = b->job_label_off;
    t.runs = runs.data();
    t.n_glyphs = b->n_chars;
    t.way_pts = b->way_pts;
    t.way_sincos = b->way_sincos;
    t.n_way_pts = b->n_way_pts;
    const int rc = textplacer_detail::validate_runs(&t, n_jobs, why, false);
    if (rc == OSMT_OK && runs_out) runs_out->swap(runs);
    return rc;
}

}  // namespace osmt

#endif /* OSMT_TEXTSHAPER_HPP */
