/*
 * osmt_numparse.h — the string work of selector matching (mapcss/styler.rs:450-499, 367-370), shared by the kernels of
 * osmt_selmatch.hip and by the host mirror (host/osmt_selmatch.hpp; tests hold it against Python's float() and int()):
 *
 *   osmt_parse_f64_fast   str::parse::<f64> where the conversion is exact by construction, else "declined"
 *   osmt_parse_i64        str::parse::<i64> in full
 *   osmt_is_true_value    "yes" | "true" | "1"
 *   osmt_bytes_cmp        &str ordering: unsigned bytes, then length
 *
 * Grammar of str::parse::<f64>:  Sign? ( inf | infinity | nan | Number ),  Number ::= (Digit+ | Digit+ '.' Digit* |
 * Digit* '.' Digit+) Exp?,  Exp ::= 'e' Sign? Digit+, ASCII case-insensitive in the words and in 'e'; no whitespace, no '_'.
 *
 * The fast path (Clinger's): all digits of the number, without leading zeros and without trailing zeros, form an integer w;
 * the value is w * 10^e with e = exponent - fraction digits + trailing zeros removed.  When w <= 2^53 and |e| <= 22, both w
 * and 10^|e| are doubles exactly (10^22 = 2^22 * 5^22, 5^22 < 2^53), so RN(w * 10^e) resp. RN(w / 10^-e) is ONE correctly
 * rounded IEEE operation on exact operands: the correctly rounded value of the decimal string.  w == 0 is +-0 whatever the
 * exponent.  Anything else is declined, never approximated.  Compile with -ffp-contract=off (nothing here can fuse, but
 * the rule of the library holds).
 */
#ifndef OSMT_NUMPARSE_H
#define OSMT_NUMPARSE_H

#include <stdint.h>

#if !defined(OSMT_HD)
#if defined(__HIPCC__)
#define OSMT_HD __host__ __device__ __forceinline__
#else
#define OSMT_HD inline
#endif
#endif

enum { OSMT_NUM_ERROR = 0, OSMT_NUM_OK = 1, OSMT_NUM_DECLINED = 2 };

OSMT_HD int osmt_bytes_cmp(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    const uint32_t n = na < nb ? na : nb;
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : (na > nb ? 1 : 0);
}

OSMT_HD bool osmt_is_true_value(const uint8_t* s, uint32_t n) {
    if (n == 1u) return s[0] == '1';
    if (n == 3u) return s[0] == 'y' && s[1] == 'e' && s[2] == 's';
    if (n == 4u) return s[0] == 't' && s[1] == 'r' && s[2] == 'u' && s[3] == 'e';
    return false;
}

/* s[0 .. n) against an all-lower-case ASCII word, ignoring the case of s */
OSMT_HD bool osmt_word_is(const uint8_t* s, uint32_t n, const char* word, uint32_t nw) {
    if (n != nw) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t c = s[i];
        const uint8_t lower = (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32u) : c;
        if (lower != (uint8_t)word[i]) return false;
    }
    return true;
}

OSMT_HD int osmt_parse_f64_fast(const uint8_t* s, uint32_t n, double* out) {
    uint32_t i = 0u;
    bool neg = false;
    if (n && (s[0] == '+' || s[0] == '-')) {
        neg = s[0] == '-';
        i = 1u;
    }
    if (i == n) return OSMT_NUM_ERROR; /* empty, or a lone sign */
    if (osmt_word_is(s + i, n - i, "inf", 3u) || osmt_word_is(s + i, n - i, "infinity", 8u)) {
        const double inf = __builtin_huge_val();
        *out = neg ? -inf : inf;
        return OSMT_NUM_OK;
    }
    if (osmt_word_is(s + i, n - i, "nan", 3u)) {
        *out = __builtin_nan("");
        return OSMT_NUM_OK;
    }
    uint64_t w = 0u;      /* the digits so far without leading zeros and without the pending zeros */
    uint32_t nd = 0u;     /* its digits */
    uint64_t pending = 0u; /* zeros seen behind the last non-zero digit */
    uint64_t n_int = 0u, n_frac = 0u;
    bool big = false;     /* more than 19 significant digits: w no longer holds them */
    bool frac = false;
    for (; i < n; ++i) {
        const uint8_t c = s[i];
        if (c == '.' && !frac) {
            frac = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        if (frac)
            ++n_frac;
        else
            ++n_int;
        const uint32_t d = (uint32_t)(c - '0');
        if (d == 0u) {
            if (nd) ++pending;
            continue;
        }
        if (big || (uint64_t)nd + pending + 1u > 19u) {
            big = true;
            pending = 0u;
            continue;
        }
        for (; pending; --pending) w *= 10u, ++nd;
        w = w * 10u + d;
        ++nd;
    }
    if (n_int + n_frac == 0u) return OSMT_NUM_ERROR; /* ".", "e5", a letter */
    int64_t ex = 0;
    if (i < n) {
        if (s[i] != 'e' && s[i] != 'E') return OSMT_NUM_ERROR;
        ++i;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) {
            eneg = s[i] == '-';
            ++i;
        }
        if (i == n) return OSMT_NUM_ERROR;
        for (; i < n; ++i) {
            if (s[i] < '0' || s[i] > '9') return OSMT_NUM_ERROR;
            if (ex < 1000000) ex = ex * 10 + (int64_t)(s[i] - '0'); /* saturates: far outside +-22 either way */
        }
        if (eneg) ex = -ex;
    }
    if (nd == 0u && !big) { /* every digit is a zero */
        *out = neg ? -0.0 : 0.0;
        return OSMT_NUM_OK;
    }
    if (big || w > ((uint64_t)1 << 53)) return OSMT_NUM_DECLINED;
    const int64_t e = ex - (int64_t)n_frac + (int64_t)pending;
    if (e < -22 || e > 22) return OSMT_NUM_DECLINED;
    double p = 1.0;
    for (int64_t k = e < 0 ? -e : e; k > 0; --k) p *= 10.0; /* exact up to 10^22 */
    const double v = e < 0 ? (double)w / p : (double)w * p;
    *out = neg ? -v : v;
    return OSMT_NUM_OK;
}

/* str::parse::<i64>: [+-]? Digit+, an error on overflow */
OSMT_HD bool osmt_parse_i64(const uint8_t* s, uint32_t n, int64_t* out) {
    uint32_t i = 0u;
    bool neg = false;
    if (n && (s[0] == '+' || s[0] == '-')) {
        neg = s[0] == '-';
        i = 1u;
    }
    if (i == n) return false;
    const uint64_t limit = neg ? ((uint64_t)1 << 63) : (((uint64_t)1 << 63) - 1u);
    uint64_t u = 0u;
    for (; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (u > (limit - d) / 10u) return false;
        u = u * 10u + d;
    }
    *out = (int64_t)(neg ? (uint64_t)0 - u : u);
    return true;
}

#endif
