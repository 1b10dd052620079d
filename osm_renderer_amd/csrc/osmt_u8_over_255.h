/* osmt_u8_over_255.h — f64::from(c) / 255.0 for a u8 (tile_pixels.rs:226-228), two ways that give the same bits:
 * the table (one load, for values that arrive per lane) and three fused corrections of c * RN(1/255) (no load, for
 * values a wave needs before anything else can start).  Host and device; tests/test_u8_over_255_cpu.py compares all
 * 256 values of both as 64-bit patterns. */
#ifndef OSMT_U8_OVER_255_H
#define OSMT_U8_OVER_255_H

#include <stdint.h>

#include "osmt_geom.h"

/* The compiler folds each entry with a correctly rounded IEEE division, so a lookup returns exactly what the reference
 * computes — without three f64 divisions per op. */
#define OSMT_C4(i) (double)(i) / 255.0, (double)((i) + 1) / 255.0, (double)((i) + 2) / 255.0, (double)((i) + 3) / 255.0
#define OSMT_C16(i) OSMT_C4(i), OSMT_C4((i) + 4), OSMT_C4((i) + 8), OSMT_C4((i) + 12)
#define OSMT_C64(i) OSMT_C16(i), OSMT_C16((i) + 16), OSMT_C16((i) + 32), OSMT_C16((i) + 48)
#if defined(__HIPCC__)
static __constant__
#else
static const
#endif
    double k_u8_over_255[256] = {OSMT_C64(0), OSMT_C64(64), OSMT_C64(128), OSMT_C64(192)};

/* The same quotient without the table: osmt_div_exact with d = 255 and r = RN(1/255), folded at compile time.  Its
 * conditions hold (n = 0 gives +0.0 through every step; any other quotient is >= 2^-8), and there are only 256 inputs:
 * the test tries them all. */
OSMT_HD double osmt_u8_over_255(uint32_t c) { return osmt_div_exact((double)c, 255.0, 1.0 / 255.0); }

#endif
