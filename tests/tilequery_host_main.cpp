// A host program of its own over host/osmt_tilequery.hpp: reads a geodata file, binds styles by a fixed rule, runs
// osmt::styled_areas_of_tile over a list of tiles and prints, per tile, the number of areas and a checksum of them.
// tests/test_tile_query_cpu.py builds it with -fsanitize=address,undefined and compares its output with the Python
// restatement of the query.   usage: tilequery_host_main FILE ZOOM X Y [ZOOM X Y ...]
#include <cstdio>
#include <cstdlib>

#include "../osm_renderer_amd/host/osmt_tilequery.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 3 != 0) {
        fprintf(stderr, "usage: %s FILE ZOOM X Y [ZOOM X Y ...]\n", argv[0]);
        return 2;
    }
    try {
        osmt::GeodataReader r(argv[1]);
        osmt::TileIndexDesc index(r);
        osmt::StyleBindings b(0, 0, 18, r.way_count(), r.multipolygon_count());
        // way i: i % 3 styles, falling ids; multipolygon m: (m + 1) % 3 styles
        for (size_t i = 0; i < r.way_count(); ++i) {
            std::vector<uint32_t> st;
            for (size_t k = 0; k < i % 3; ++k) st.push_back((uint32_t)(7 * i + 5 - k));
            if (!st.empty()) b.bind_way(i, st);
        }
        for (size_t m = 0; m < r.multipolygon_count(); ++m) {
            std::vector<uint32_t> st;
            for (size_t k = 0; k < (m + 1) % 3; ++k) st.push_back((uint32_t)(11 * m + 9 - k));
            if (!st.empty()) b.bind_multipolygon(m, st);
        }
        const osmt_style_bindings_desc& d = b.desc();
        printf("index %zu %zu %zu bindings %zu %zu\n", index.desc.n_tiles, index.desc.n_way_refs, index.desc.n_multipolygon_refs, d.n_way_styles,
               d.n_multipolygon_styles);
        for (int a = 2; a + 2 < argc; a += 3) {
            const std::vector<osmt_styled_area> areas =
                osmt::styled_areas_of_tile(r, b, (uint8_t)atoi(argv[a]), (uint32_t)strtoul(argv[a + 1], nullptr, 10), (uint32_t)strtoul(argv[a + 2], nullptr, 10));
            unsigned long long sum = 0;
            for (size_t i = 0; i < areas.size(); ++i) sum = sum * 1000003ull + areas[i].entity * 31ull + areas[i].style;
            printf("%zu %llu\n", areas.size(), sum);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
