// C entry points over host/osmt_cascade.hpp for tests/_cascade.py (ctypes): the host mirror osmt::cascade_host and the layout
// of the descriptor.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_cascade.hpp"

using namespace osmt;

extern "C" {
void* cs_host_new(const osmt_rules_desc* rules, const osmt_selectors_desc* selectors, const osmt_match_class* classes, size_t n_classes,
                  const uint32_t* class_selectors, int labels_all) {
    return new HostCascade(cascade_host(*rules, *selectors, classes, n_classes, class_selectors, labels_all != 0));
}
void cs_host_free(void* h) { delete (HostCascade*)h; }
// the counts of osmt_cascade_read, the class count left to the caller
void cs_host_counts(void* p, size_t counts[8]) {
    const HostCascade& h = *(const HostCascade*)p;
    counts[0] = h.styles.size(), counts[1] = h.dashes.size(), counts[2] = h.label_styles.size(), counts[3] = h.key_bytes.size();
    counts[4] = h.key_off.size() - 1, counts[5] = h.zoom_lo.size(), counts[6] = h.class_styles.size(), counts[7] = h.bindings.size();
}
// the thirteen arrays in the order of osmt_cascade_read, each sized by the counts
void cs_host_copy(void* p, void** out) {
    const HostCascade& h = *(const HostCascade*)p;
    auto put = [](void* dst, const void* src, size_t bytes) {
        if (bytes) memcpy(dst, src, bytes);
    };
    put(out[0], h.styles.data(), h.styles.size() * sizeof(osmt_style_rec));
    put(out[1], h.dashes.data(), h.dashes.size() * 8);
    put(out[2], h.label_styles.data(), h.label_styles.size() * sizeof(osmt_label_style_rec));
    put(out[3], h.key_bytes.data(), h.key_bytes.size());
    put(out[4], h.key_off.data(), h.key_off.size() * 4);
    put(out[5], h.zoom_lo.data(), h.zoom_lo.size());
    put(out[6], h.zoom_hi.data(), h.zoom_hi.size());
    put(out[7], h.class_style_off.data(), h.class_style_off.size() * 4);
    put(out[8], h.class_styles.data(), h.class_styles.size() * 4);
    put(out[9], h.range_style_base.data(), h.range_style_base.size() * 4);
    put(out[10], h.class_off.data(), h.class_off.size() * 4);
    put(out[11], h.bindings.data(), h.bindings.size() * sizeof(osmt_class_label_binding));
    put(out[12], h.range_binding_base.data(), h.range_binding_base.size() * 4);
}
size_t cs_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_rule_prop);
        case 1: return sizeof(osmt_rules_desc);
        case 2: return sizeof(osmt_cs_prop);
        case 10: return offsetof(osmt_rule_prop, image);
        case 11: return offsetof(osmt_rule_prop, delta);
        case 12: return offsetof(osmt_rules_desc, layer_off);
        case 13: return offsetof(osmt_rules_desc, numbers);
        case 14: return offsetof(osmt_rules_desc, casing_width_multiplier);
        case 15: return offsetof(osmt_rules_desc, has_font_size_multiplier);
    }
    return 0;
}
}
