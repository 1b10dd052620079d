// osmt::LabelPositions (osm_renderer_amd/host/osmt_labelable.hpp) against libosmtile.so: a batch with one request the
// device declines (a 5000 x 0.01 strip: its initial grid alone is 500 000 cells) between ordinary ones.  Prints, per
// request, the collector's answer and the host mirror's as hex bit patterns, and how many requests fell back to the CPU.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../osm_renderer_amd/host/osmt_labelable.hpp"

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

int main() {
    osmt_ctx* ctx = nullptr;
    if (osmt_create(nullptr, &ctx) != OSMT_OK) {
        std::fprintf(stderr, "osmt_create: %s\n", osmt_last_error());
        return 2;
    }
    const osmt::LabelRing square = {{10.5, 20.25}, {50.5, 20.25}, {50.5, 60.25}, {10.5, 60.25}, {10.5, 20.25}};
    const osmt::LabelRing strip = {{0.0, 0.0}, {5000.0, 0.0}, {5000.0, 0.01}, {0.0, 0.01}, {0.0, 0.0}};
    const osmt::LabelRing ell = {{1.5, 2.5}, {81.5, 2.5}, {81.5, 32.25}, {31.75, 32.25}, {31.75, 92.5}, {1.5, 92.5}, {1.5, 2.5}};
    const std::vector<osmt::LabelRing> hole = {square, {{20.5, 30.25}, {20.5, 40.25}, {30.5, 40.25}, {30.5, 30.25}, {20.5, 30.25}}};
    osmt::LabelPositions lp;
    lp.add_way(square, 1.0);
    lp.add_way(strip, 1.0);
    lp.add_way(ell, 2.0);
    lp.add_multipolygon(hole, 1.0);
    std::vector<osmt_label_position> got;
    try {
        got = lp.run(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    const osmt::LabelPosition want[4] = {osmt::get_label_position({square}, 1.0), osmt::get_label_position({strip}, 1.0),
                                         osmt::get_label_position({ell}, 2.0), osmt::get_label_position(hole, 1.0)};
    for (int i = 0; i < 4; ++i)
        std::printf("%d %u %016" PRIx64 " %016" PRIx64 " %u %016" PRIx64 " %016" PRIx64 "\n", i, got[i].status, bits(got[i].x), bits(got[i].y),
                    want[i].status, bits(want[i].x), bits(want[i].y));
    std::printf("fallbacks %zu\n", lp.cpu_fallbacks());
    osmt_destroy(ctx);
    return 0;
}
