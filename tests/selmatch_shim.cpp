// C entry points over host/osmt_selmatch.hpp for tests/_selmatch.py (ctypes): osmt::TagsDesc, osmt::SelectorSet, the host
// mirror osmt::match_selectors_host, the number parsers, osmt::HostNumbers and osmt::selectors_at_zoom.  Host only.
#include <cstddef>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_selmatch.hpp"

using namespace osmt;

extern "C" {
void* sm_tags_new(void* reader) { return new TagsDesc(*(const GeodataReader*)reader); }
const osmt_tags_desc* sm_tags_get(void* d) { return &((TagsDesc*)d)->desc; }
void sm_tags_free(void* d) { delete (TagsDesc*)d; }

void* sm_set_new() { return new SelectorSet(); }
void sm_set_add(void* s, uint8_t type, int min_zoom, int max_zoom) { ((SelectorSet*)s)->add(type, min_zoom, max_zoom); }
void sm_set_test(void* s, uint32_t kind, const char* key, size_t key_len, const char* value, size_t value_len, double number) {
    ((SelectorSet*)s)->test(kind, std::string_view(key, key_len), std::string_view(value, value_len), number);
}
const osmt_selectors_desc* sm_set_get(void* s) { return &((SelectorSet*)s)->desc(); }
void sm_set_free(void* s) { delete (SelectorSet*)s; }

// counts = { entities, classes, pooled ids }; nothing is written beyond caps
void sm_match_host(void* reader, const osmt_selectors_desc* d, uint32_t* ent_class, osmt_match_class* classes, uint32_t* sels, const size_t caps[3],
                   size_t counts[3]) {
    const HostMatch m = match_selectors_host(*(const GeodataReader*)reader, *d);
    counts[0] = m.entity_class.size(), counts[1] = m.classes.size(), counts[2] = m.class_selectors.size();
    if (ent_class && caps[0] >= counts[0] && counts[0]) memcpy(ent_class, m.entity_class.data(), counts[0] * 4);
    if (classes && caps[1] >= counts[1] && counts[1]) memcpy(classes, m.classes.data(), counts[1] * sizeof(osmt_match_class));
    if (sels && caps[2] >= counts[2] && counts[2]) memcpy(sels, m.class_selectors.data(), counts[2] * 4);
}

int sm_parse_f64(const char* s, size_t n, double* out) { return parse_f64(std::string_view(s, n), out) ? 1 : 0; }
int sm_fast_path(const char* s, size_t n, double* out) { return number_fast_path(std::string_view(s, n), out); }
int sm_parse_i64(const char* s, size_t n, int64_t* out) { return parse_i64(std::string_view(s, n), out) ? 1 : 0; }
int sm_device_i64(const char* s, size_t n, int64_t* out) { return osmt_parse_i64((const uint8_t*)s, (uint32_t)n, out) ? 1 : 0; }

void sm_host_numbers(const uint8_t* strings, const osmt_declined_number* declined, size_t n, osmt_number_override* out) {
    const HostNumbers h(strings, declined, n);
    if (n) memcpy(out, h.overrides.data(), n * sizeof(osmt_number_override));
}

size_t sm_at_zoom(const osmt_selectors_desc* d, const uint32_t* sels, size_t n, uint8_t zoom, uint32_t* out) {
    const std::vector<uint32_t> v = selectors_at_zoom(*d, sels, n, zoom);
    if (!v.empty()) memcpy(out, v.data(), v.size() * 4);
    return v.size();
}

size_t sm_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_tags_desc);
        case 1: return sizeof(osmt_selector_test);
        case 2: return sizeof(osmt_selector_rec);
        case 3: return sizeof(osmt_selectors_desc);
        case 4: return sizeof(osmt_number_override);
        case 5: return sizeof(osmt_declined_number);
        case 6: return sizeof(osmt_match_class);
        case 10: return offsetof(osmt_tags_desc, strings);
        case 11: return offsetof(osmt_selector_test, value);
        case 12: return offsetof(osmt_selector_rec, test_off);
        case 13: return offsetof(osmt_number_override, value);
        case 14: return offsetof(osmt_match_class, first_entity);
        case 15: return offsetof(osmt_match_class, has_layer);
    }
    return 0;
}
}
