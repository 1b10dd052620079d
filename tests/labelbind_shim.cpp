// C entry points over host/osmt_selmatch.hpp and csrc/osmt_utf8.h for tests/_labelbind.py (ctypes): the host mirrors
// osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host, osmt::ClassLabelBindings and the UTF-8 decoder.
// Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_selmatch.hpp"

using namespace osmt;

extern "C" {
void* lb_table_new(const osmt_tags_desc* tags, const uint32_t* entity_class, const osmt_class_label_bindings_desc* d, int area) {
    return new HostLabelTable(area ? area_label_bindings_matched_host(*tags, entity_class, *d) : label_bindings_matched_host(*tags, entity_class, *d));
}
void lb_table_free(void* t) { delete (HostLabelTable*)t; }
// ok; counts = { off 0, bindings 0, off 1, bindings 1, text_off, chars } in entries
int lb_table_counts(void* t, size_t counts[6]) {
    const HostLabelTable& h = *(const HostLabelTable*)t;
    counts[0] = h.off[0].size(), counts[1] = h.bindings[0].size(), counts[2] = h.off[1].size(), counts[3] = h.bindings[1].size();
    counts[4] = h.text_off.size(), counts[5] = h.chars.size();
    return h.ok ? 1 : 0;
}
// the six arrays, each sized by lb_table_counts
void lb_table_copy(void* t, uint32_t* off0, osmt_label_binding* bind0, uint32_t* off1, osmt_label_binding* bind1, uint32_t* text_off, uint32_t* chars) {
    const HostLabelTable& h = *(const HostLabelTable*)t;
    auto put = [](void* dst, const void* src, size_t bytes) {
        if (bytes) memcpy(dst, src, bytes);
    };
    put(off0, h.off[0].data(), h.off[0].size() * 4), put(bind0, h.bindings[0].data(), h.bindings[0].size() * sizeof(osmt_label_binding));
    put(off1, h.off[1].data(), h.off[1].size() * 4), put(bind1, h.bindings[1].data(), h.bindings[1].size() * sizeof(osmt_label_binding));
    put(text_off, h.text_off.data(), h.text_off.size() * 4), put(chars, h.chars.data(), h.chars.size() * 4);
}
// of a refused table: the kind's name; out = { entity, tag, v_off, v_len }
const char* lb_table_bad(void* t, size_t out[4]) {
    const HostLabelTable& h = *(const HostLabelTable*)t;
    out[0] = h.bad_entity, out[1] = h.bad_tag, out[2] = h.bad_v_off, out[3] = h.bad_v_len;
    return h.bad_kind;
}

void* lb_builder_new(uint8_t zoom_lo, uint8_t zoom_hi) { return new ClassLabelBindings(zoom_lo, zoom_hi); }
void lb_builder_add_class(void* b) { ((ClassLabelBindings*)b)->add_class(); }
void lb_builder_bind(void* b, uint32_t style, const char* key, size_t key_len, int has_key) {
    ((ClassLabelBindings*)b)->bind(style, std::string_view(key, key_len), has_key != 0);
}
const osmt_class_label_bindings_desc* lb_builder_get(void* b) { return &((ClassLabelBindings*)b)->desc(); }
void lb_builder_free(void* b) { delete (ClassLabelBindings*)b; }

// osmt_utf8_validate, and the scalars when the string is well-formed (out has room for n)
uint32_t lb_utf8(const uint8_t* s, uint32_t n, uint32_t* out, uint32_t* n_scalars) {
    const uint32_t bad = osmt_utf8_validate(s, n, n_scalars);
    if (bad == n && out) *n_scalars = osmt_utf8_decode(s, n, out);
    return bad;
}
// `count` strings of `len` bytes each, back to back: bad[i] and n_scalars[i]; scalars[i * len ..] when well-formed
void lb_utf8_many(const uint8_t* s, uint32_t len, size_t count, uint32_t* bad, uint32_t* n_scalars, uint32_t* scalars) {
    for (size_t i = 0; i < count; ++i) bad[i] = lb_utf8(s + i * len, len, scalars + i * len, n_scalars + i);
}

size_t lb_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_class_label_binding);
        case 1: return sizeof(osmt_class_label_bindings_desc);
        case 10: return offsetof(osmt_class_label_bindings_desc, class_off);
        case 11: return offsetof(osmt_class_label_bindings_desc, n_classes);
        case 12: return offsetof(osmt_class_label_bindings_desc, key_off);
        case 13: return offsetof(osmt_class_label_bindings_desc, n_key_bytes);
    }
    return 0;
}
}
