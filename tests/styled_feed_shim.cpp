// C entry points over the host helpers of the styled feed (osmt::style_rec_of in host/osmt_styled.hpp, osmt::GeodataDesc in
// host/osmt_geodata.hpp) for tests/test_styled_feed_cpu.py (ctypes).  Host only.  The Style records arrive in the layout of
// tests/styled_shim.cpp, whose conversion to osmt::Style is reused as it is.
#include <cstddef>

#include "styled_shim.cpp"

extern "C" {
// ShimStyle -> osmt::Style -> osmt_style_rec; the dash pool the records index is written to pool_out (capacity cap)
size_t sf_style_recs(const ShimStyle* styles, size_t n, const double* pool_in, osmt_style_rec* out, double* pool_out, size_t cap) {
    const std::vector<Style> st = styles_of(styles, n, pool_in);
    std::vector<double> pool;
    for (size_t i = 0; i < n; ++i) out[i] = style_rec_of(st[i], pool);
    if (pool.size() <= cap && !pool.empty()) memcpy(pool_out, pool.data(), pool.size() * sizeof(double));
    return pool.size();
}
void* sf_desc_new(void* reader) { return new GeodataDesc(*(const GeodataReader*)reader); }
const osmt_geodata_desc* sf_desc_get(void* d) { return &((GeodataDesc*)d)->desc; }
void sf_desc_free(void* d) { delete (GeodataDesc*)d; }
size_t sf_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_style_rec);
        case 1: return sizeof(osmt_styled_area);
        case 2: return sizeof(osmt_styled_tile);
        case 3: return sizeof(osmt_styled_batch);
        case 4: return sizeof(osmt_geodata_desc);
        case 10: return offsetof(osmt_style_rec, fill_image);
        case 11: return offsetof(osmt_style_rec, has_layer);
        case 12: return offsetof(osmt_style_rec, line_cap);
        case 13: return offsetof(osmt_style_rec, has_fill_image);
        case 14: return offsetof(osmt_style_rec, background_color);
        case 20: return offsetof(osmt_styled_tile, area_off);
        case 30: return offsetof(osmt_styled_batch, geodata_id);
        case 40: return offsetof(osmt_geodata_desc, multipolygon_polygons);
    }
    return 0;
}
}
