// Host build of the text shaper (osm_renderer_amd/host/osmt_textshaper.hpp: TextPlacer::text_to_glyphs as the device runs
// it, and the validation of osmt_register_font / osmt_validate_string_labels) plus sizeof / offsetof probes of the
// string-label ABI structs, for the CPU-side tests.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../include/osmtile.h"
#include "../osm_renderer_amd/host/osmt_textshaper.hpp"

static void put(const std::string& s, char* why, size_t cap) {
    if (why && cap) {
        std::strncpy(why, s.c_str(), cap - 1);
        why[cap - 1] = 0;
    }
}

extern "C" {
// osmt::shape_text: out[n]
void shim_shape_text(const osmt_font_desc* f, const uint32_t* chars, uint32_t n, osmt_text_glyph* out) { osmt::shape_text(*f, chars, n, out); }
// osmt::shape_string_labels of a validated batch: out[n_chars] in slot order
void shim_shape_labels(const osmt_string_label_batch* b, const osmt_font_desc* const* fonts, osmt_text_glyph* out) {
    osmt::shape_string_labels(*b, fonts, out);
}
double shim_string_scale(const osmt_font_desc* f, double font_size) { return osmt::string_scale(*f, font_size); }
// osmt::validate_font: the status; the reason (truncated to cap - 1 chars) in why
int shim_font_validate(const osmt_font_desc* f, size_t n_outlines, char* why, size_t cap) {
    std::string s;
    const int rc = osmt::validate_font(f, n_outlines, &s);
    put(s, why, cap);
    return rc;
}
// osmt::validate_string_labels; runs_out (optional, [n_labels]) gets the text runs it builds when it passes
int shim_string_validate(const osmt_string_label_batch* b, size_t n_jobs, const osmt_font_desc* const* fonts, size_t n_fonts, char* why,
                         size_t cap, osmt_text_run* runs_out) {
    std::string s;
    std::vector<osmt_text_run> runs;
    const int rc = osmt::validate_string_labels(b, n_jobs, fonts, n_fonts, &s, &runs);
    put(s, why, cap);
    if (rc == OSMT_OK && runs_out && !runs.empty()) std::memcpy(runs_out, runs.data(), runs.size() * sizeof(osmt_text_run));
    return rc;
}
size_t shim_shape_abi_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_cmap_entry);
        case 1: return sizeof(osmt_kern_pair);
        case 2: return sizeof(osmt_font_desc);
        case 3: return sizeof(osmt_string_run);
        case 4: return sizeof(osmt_string_label_batch);
        case 10: return offsetof(osmt_font_desc, advance);
        case 11: return offsetof(osmt_font_desc, outline_id);
        case 12: return offsetof(osmt_font_desc, kern);
        case 13: return offsetof(osmt_font_desc, ascent);
        case 14: return offsetof(osmt_font_desc, line_gap);
        case 15: return offsetof(osmt_string_run, font_id);
        case 16: return offsetof(osmt_string_run, font_size);
        case 17: return offsetof(osmt_string_run, center_x);
        case 18: return offsetof(osmt_string_label_batch, chars);
        case 19: return offsetof(osmt_string_label_batch, n_way_pts);
    }
    return 0;
}
}
