// Stand-alone program: csrc/osmt_utf8.h over EVERY string of 1, 2 and 3 bytes against a literal statement of Table 3-7 of the
// Unicode Standard (well-formed UTF-8 byte sequences), written here without any arithmetic shared with the decoder: accept or
// reject, the index of the first byte that starts no well-formed sequence, the scalars.  Prints "OK <strings>" or the first
// difference.
#include <cstdint>
#include <cstdio>

#include "../osm_renderer_amd/csrc/osmt_utf8.h"

namespace {
struct Row {
    uint8_t lo[4], hi[4]; // byte ranges; len bytes used
    int len;
};
// Table 3-7, row by row
const Row TABLE[] = {
    {{0x00}, {0x7F}, 1},
    {{0xC2, 0x80}, {0xDF, 0xBF}, 2},
    {{0xE0, 0xA0, 0x80}, {0xE0, 0xBF, 0xBF}, 3},
    {{0xE1, 0x80, 0x80}, {0xEC, 0xBF, 0xBF}, 3},
    {{0xED, 0x80, 0x80}, {0xED, 0x9F, 0xBF}, 3},
    {{0xEE, 0x80, 0x80}, {0xEF, 0xBF, 0xBF}, 3},
    {{0xF0, 0x90, 0x80, 0x80}, {0xF0, 0xBF, 0xBF, 0xBF}, 4},
    {{0xF1, 0x80, 0x80, 0x80}, {0xF3, 0xBF, 0xBF, 0xBF}, 4},
    {{0xF4, 0x80, 0x80, 0x80}, {0xF4, 0x8F, 0xBF, 0xBF}, 4},
};

// the length of the row that matches s[i ..) inside s[0 .. n), or 0; the scalar by the definition of UTF-8 (D92)
int match(const uint8_t* s, uint32_t i, uint32_t n, uint32_t* cp) {
    for (const Row& r : TABLE) {
        if ((uint32_t)r.len > n - i) continue;
        bool ok = true;
        for (int k = 0; k < r.len; ++k) ok = ok && s[i + k] >= r.lo[k] && s[i + k] <= r.hi[k];
        if (!ok) continue;
        switch (r.len) {
            case 1: *cp = s[i]; break;
            case 2: *cp = (uint32_t)(s[i] - 0xC0) * 64 + (s[i + 1] - 0x80); break;
            case 3: *cp = (uint32_t)(s[i] - 0xE0) * 4096 + (uint32_t)(s[i + 1] - 0x80) * 64 + (s[i + 2] - 0x80); break;
            default: *cp = (uint32_t)(s[i] - 0xF0) * 262144 + (uint32_t)(s[i + 1] - 0x80) * 4096 + (uint32_t)(s[i + 2] - 0x80) * 64 + (s[i + 3] - 0x80);
        }
        return r.len;
    }
    return 0;
}

bool check(const uint8_t* s, uint32_t n) {
    uint32_t want[4], n_want = 0, i = 0;
    while (i < n) {
        uint32_t cp;
        const int k = match(s, i, n, &cp);
        if (!k) break;
        want[n_want++] = cp;
        i += (uint32_t)k;
    }
    uint32_t n_got = 0, got[4] = {};
    const uint32_t bad = osmt_utf8_validate(s, n, &n_got);
    bool ok = bad == i && n_got == n_want;
    if (ok && bad == n) {
        ok = osmt_utf8_decode(s, n, got) == n_want;
        for (uint32_t k = 0; ok && k < n_want; ++k) ok = got[k] == want[k];
    }
    if (!ok) printf("DIFFERENT at %02X %02X %02X (n = %u): first bad byte %u against %u, %u scalars against %u\n", s[0], n > 1 ? s[1] : 0, n > 2 ? s[2] : 0, n, bad, i, n_got, n_want);
    return ok;
}
}  // namespace

int main() {
    // each string sits at the END of an allocation of its own size: a read past it is what the sanitizer build of the other program
    // would catch; here the bytes behind it are a continuation byte that would complete a cut-off sequence
    uint8_t buf[8];
    size_t count = 0;
    for (uint32_t n = 1; n <= 3; ++n)
        for (uint32_t v = 0; v < (1u << (8 * n)); ++v) {
            for (uint32_t k = 0; k < n; ++k) buf[k] = (uint8_t)(v >> (8 * k));
            for (uint32_t k = n; k < 8; ++k) buf[k] = 0x80;
            if (!check(buf, n)) return 1;
            ++count;
        }
    // the 4-byte rows at their corners and one step outside them
    const uint8_t four[][4] = {{0xF0, 0x90, 0x80, 0x80}, {0xF0, 0x8F, 0xBF, 0xBF}, {0xF0, 0xBF, 0xBF, 0xBF}, {0xF1, 0x80, 0x80, 0x80}, {0xF3, 0xBF, 0xBF, 0xBF},
                               {0xF4, 0x80, 0x80, 0x80}, {0xF4, 0x8F, 0xBF, 0xBF}, {0xF4, 0x90, 0x80, 0x80}, {0xF5, 0x80, 0x80, 0x80}, {0xF0, 0x90, 0x80, 0x7F},
                               {0xF0, 0x90, 0xC0, 0x80}, {0xF1, 0x7F, 0x80, 0x80}, {0xF4, 0x8F, 0xBF, 0xC0}, {0xF8, 0x88, 0x80, 0x80}};
    for (const auto& s : four) {
        if (!check(s, 4)) return 1;
        ++count;
    }
    printf("OK %zu\n", count);
    return 0;
}
