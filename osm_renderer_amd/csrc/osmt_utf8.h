/*
 * osmt_utf8.h — UTF-8 of tag values into Unicode scalar values, shared by the kernels of osmt_labelbind.hip and by the host
 * mirror (host/osmt_selmatch.hpp; tests hold it against Python's strict decoder and against a literal statement of the table):
 *
 *   osmt_utf8_step      one well-formed sequence at s[i], or 0
 *   osmt_utf8_validate  the index of the first byte that starts no well-formed sequence (n: none) and the scalar count
 *   osmt_utf8_decode    the scalars of a well-formed string
 *
 * Well-formed is Table 3-7 of the Unicode Standard:
 *
 *   00..7F
 *   C2..DF  80..BF
 *   E0      A0..BF  80..BF          (no overlong 3-byte forms)
 *   E1..EC  80..BF  80..BF
 *   ED      80..9F  80..BF          (no surrogates)
 *   EE..EF  80..BF  80..BF
 *   F0      90..BF  80..BF  80..BF  (no overlong 4-byte forms)
 *   F1..F3  80..BF  80..BF  80..BF
 *   F4      80..8F  80..BF  80..BF  (nothing above U+10FFFF)
 *
 * C0, C1 and F5..FF start nothing.  A sequence the end of the string cuts off is ill-formed, and no byte at or past s + n is
 * read: the length of a sequence is known from its first byte and is compared with what is left before the second is loaded.
 */
#ifndef OSMT_UTF8_H
#define OSMT_UTF8_H

#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

/* the length of the well-formed sequence that starts at s[i] (i < n) and its scalar value, or 0 */
OSMT_HD uint32_t osmt_utf8_step(const uint8_t* s, uint32_t i, uint32_t n, uint32_t* cp) {
    const uint32_t b0 = s[i];
    if (b0 < 0x80u) {
        *cp = b0;
        return 1u;
    }
    if (b0 < 0xC2u || b0 > 0xF4u) return 0u;
    const uint32_t len = b0 < 0xE0u ? 2u : (b0 < 0xF0u ? 3u : 4u);
    if (n - i < len) return 0u;
    uint32_t lo = 0x80u, hi = 0xBFu; /* the range of the second byte */
    if (b0 == 0xE0u) lo = 0xA0u;
    if (b0 == 0xEDu) hi = 0x9Fu;
    if (b0 == 0xF0u) lo = 0x90u;
    if (b0 == 0xF4u) hi = 0x8Fu;
    const uint32_t b1 = s[i + 1u];
    if (b1 < lo || b1 > hi) return 0u;
    uint32_t v = ((b0 & (0x7Fu >> len)) << 6) | (b1 & 0x3Fu);
    for (uint32_t k = 2u; k < len; ++k) {
        const uint32_t b = s[i + k];
        if ((b & 0xC0u) != 0x80u) return 0u;
        v = (v << 6) | (b & 0x3Fu);
    }
    *cp = v;
    return len;
}

/* n when s[0 .. n) is well-formed, else the index of the first byte that starts no well-formed sequence; *n_scalars: the
 * scalars in front of that index */
OSMT_HD uint32_t osmt_utf8_validate(const uint8_t* s, uint32_t n, uint32_t* n_scalars) {
    uint32_t i = 0u, count = 0u;
    while (i < n) {
        uint32_t cp;
        const uint32_t k = osmt_utf8_step(s, i, n, &cp);
        if (k == 0u) break;
        i += k;
        ++count;
    }
    *n_scalars = count;
    return i;
}

/* the scalars of s[0 .. n), which osmt_utf8_validate found well-formed, to out; returns their number */
OSMT_HD uint32_t osmt_utf8_decode(const uint8_t* s, uint32_t n, uint32_t* out) {
    uint32_t i = 0u, count = 0u;
    while (i < n) {
        uint32_t cp = 0u;
        const uint32_t k = osmt_utf8_step(s, i, n, &cp);
        if (k == 0u) break; /* not reached for a validated string */
        out[count++] = cp;
        i += k;
    }
    return count;
}

#endif
