// Host build of osm_renderer_amd/csrc/osmt_u8_over_255.h for tests/test_u8_over_255_cpu.py: the table k_raster looks
// colours up in and the quotient it computes for the canvas and the entries' colours, as 64-bit patterns.
#include <cstdint>
#include <cstring>

#include "../osm_renderer_amd/csrc/osmt_u8_over_255.h"

extern "C" {

// out[3 * c + 0] = the table's entry, [1] = osmt_u8_over_255(c), [2] = f64::from(c) / 255.0 divided here at run time
void shim_u8_over_255(uint64_t* out) {
    for (uint32_t c = 0; c < 256u; ++c) {
        volatile double num = (double)c, den = 255.0; // (volatile: a division the compiler cannot fold)
        const double v[3] = {k_u8_over_255[c], osmt_u8_over_255(c), num / den};
        for (int k = 0; k < 3; ++k) std::memcpy(&out[3u * c + (uint32_t)k], &v[k], 8);
    }
}
}
