// Host build of the text placer (osm_renderer_amd/host/osmt_textplacer.hpp: TextPlacer::place as the device runs it, and
// the validation of osmt_validate_text_labels) plus sizeof / offsetof probes of the text-run ABI structs, for the
// CPU-side tests.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../include/osmtile.h"
#include "../osm_renderer_amd/host/osmt_textplacer.hpp"

extern "C" {
// the glyph instances of a validated batch, out[n_glyphs] in slot order
void shim_text_place(const osmt_text_label_batch* b, osmt_glyph_instance* out) { osmt::place_text_labels(*b, out); }
// osmt::validate_text_labels: the status; the reason (truncated to cap - 1 chars) in why
int shim_text_validate(const osmt_text_label_batch* b, size_t n_jobs, char* why, size_t cap) {
    std::string s;
    const int rc = osmt::validate_text_labels(b, n_jobs, &s);
    if (why && cap) {
        std::strncpy(why, s.c_str(), cap - 1);
        why[cap - 1] = 0;
    }
    return rc;
}
size_t shim_text_abi_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_text_glyph);
        case 1: return sizeof(osmt_text_run);
        case 2: return sizeof(osmt_text_label_batch);
        case 10: return offsetof(osmt_text_glyph, kern);
        case 11: return offsetof(osmt_text_glyph, flags);
        case 12: return offsetof(osmt_text_run, scale);
        case 13: return offsetof(osmt_text_run, ascent);
        case 14: return offsetof(osmt_text_run, center_x);
        case 15: return offsetof(osmt_text_label_batch, runs);
        case 16: return offsetof(osmt_text_label_batch, way_pts);
        case 17: return offsetof(osmt_text_label_batch, n_way_pts);
        case 20: return OSMT_TEXT_CENTER;
        case 21: return OSMT_TEXT_LINE;
        case 22: return OSMT_GLYPH_NONE;
    }
    return 0;
}
}
